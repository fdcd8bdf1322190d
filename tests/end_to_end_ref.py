"""Test helper: numpy-float32 restatement of the task side of the end-to-end motor-command set-point task (the agx_end_to_end_*
kernels and agx_post_step_end_to_end's observation and bookkeeping) and of the order in which its step() touches the task's state.
It is the comparator of the GPU tests (the reference's code does not exist where they run) and is itself pinned to the reference bit
for bit by tests/test_end_to_end_task.py (tests/golden/end_to_end_cr/*.npz: the reference's own code with correctly rounded
elementary functions).

Every array is float32 and every + - * / sqrt one rounded float32 operation; exp / sin / cos / atan2 / asin are evaluated in float64
and rounded once; the fused multiply-adds inside torch.cross and torch.norm are explicit (sim2real_ref.fma).  torch.matmul of the
3 x 3 rotation factors sums its three rounded products left to right."""
import numpy as np
from sim2real_ref import _el, f32, norm3, quat_rotate

F = np.float32
STD_POS, STD_EULER, STD_LINVEL, STD_ANGVEL = F(0.001), F(np.pi / 1032), F(0.002), F(0.001)
LIMIT_MIN, LIMIT_MAX = np.full(4, 0.2, np.float32), np.full(4, 1.2, np.float32)
CRASH_DIST = 1.5
# compute_reward's constants (position_setpoint_task_sim2real_end_to_end.py:267-309)
K = dict(z_error_weight=11.0, pos=((10.0, 10.0), (2.0, 2.0)), upright=(2.5, 5.0), alignment=(6.0, 5.0), angvel=(0.3, 10.0), vel=(1.0, 5.0),
         hover_thrust=9.81 * 0.372 / 4, action=(0.01, 10.0), closer_gain=10.0, farther_gain=15.0, diff=(1.3, 6.0), divisor=100.0)


def _exp(x, gain, e):
    return F(gain) * _el(np.exp, (F(-e) * x) * x)


def _exp_penalty(x, gain, e):
    return F(gain) * (_el(np.exp, (F(-e) * x) * x) - F(1.0))


def _sum(x):
    """torch.sum(x, dim=1), left to right"""
    s = x[:, 0]
    for c in range(1, x.shape[1]):
        s = s + x[:, c]
    return s


def rescale(actions, lo=LIMIT_MIN, hi=LIMIT_MAX):
    """task_config.process_actions_for_task (config :28-33); np.clip passes NaN through like torch.clamp"""
    with np.errstate(invalid="ignore"):
        c = np.clip(f32(actions), F(-1.0), F(1.0))
    return ((c * (f32(hi) - f32(lo))) / F(2.0) + (f32(hi) + f32(lo)) / F(2.0)).astype(np.float32)


def reward(target, position, orientation, linvel, body_angvel, crashes, sim_steps, actions, prev_actions, prev_pos_error, episode_len,
           crash_dist=CRASH_DIST, reset_on_collision=True):
    """agx_end_to_end_reward -> dict(reward, crashes, truncations, reset_mask, dist)"""
    err = f32(target) - f32(position)
    dist, prev_dist = norm3(err), norm3(f32(prev_pos_error))
    e = err.copy()
    e[:, 2] = e[:, 2] * F(K["z_error_weight"])
    pos = _sum(_exp(e, *K["pos"][0])) + _sum(_exp(e, *K["pos"][1]))
    q = f32(orientation)
    n = q.shape[0]
    axis = lambda c: np.tile(np.eye(3, dtype=np.float32)[c], (n, 1))  # noqa: E731
    upright = _exp(F(1.0) - quat_rotate(q, axis(2))[:, 2], *K["upright"])
    alignment = _exp(F(1.0) - quat_rotate(q, axis(0))[:, 0], *K["alignment"])
    angvel = _sum(_exp(f32(body_angvel), *K["angvel"]))
    vel = _sum(_exp(f32(linvel), *K["vel"]))
    a, pa = f32(actions), f32(prev_actions)
    action_cost = _sum(_exp_penalty(a - F(K["hover_thrust"]), *K["action"]))
    closer = prev_dist - dist
    towards = np.where(closer >= 0, F(K["closer_gain"]) * closer, F(K["farther_gain"]) * closer).astype(np.float32)
    diff = _sum(_exp_penalty(a - pa, *K["diff"]))
    total = towards + (pos * (((alignment + vel) + angvel) + diff) + ((((angvel + vel) + upright) + pos) + action_cost)) / F(K["divisor"])
    crash = np.asarray(crashes).astype(bool) | (dist > F(crash_dist))
    trunc = np.asarray(sim_steps) > episode_len
    return dict(reward=total.astype(np.float32), crashes=crash, truncations=trunc, reset_mask=(crash & bool(reset_on_collision)) | trunc,
                dist=dist)


def euler_zyx(orientation):
    """quaternion_to_matrix(q_wxyz) -> matrix_to_euler_angles(., "ZYX")[:, [2, 1, 0]]: roll, pitch, yaw; no clamp in front of asin"""
    q = f32(orientation)
    i, j, k, r = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    two_s = F(2.0) / (((r * r + i * i) + j * j) + k * k)
    m00 = F(1.0) - two_s * (j * j + k * k)
    m10 = two_s * (i * j + k * r)
    m20 = two_s * (i * k - j * r)
    m21 = two_s * (j * k + i * r)
    m22 = F(1.0) - two_s * (i * i + j * j)
    return np.stack([_el(np.arctan2, m21, m22), _el(np.arcsin, -m20), _el(np.arctan2, m10, m00)], axis=1), m20


def rotation_6d(euler):
    """euler_angles_to_matrix((yaw, pitch, roll), "ZYX") -> matrix_to_rotation_6d: rows 0 and 1 of (Rz Ry) Rx"""
    roll, pitch, yaw = euler[:, 0], euler[:, 1], euler[:, 2]
    sz, cz, sy, cy = _el(np.sin, yaw), _el(np.cos, yaw), _el(np.sin, pitch), _el(np.cos, pitch)
    sx, cx = _el(np.sin, roll), _el(np.cos, roll)
    a00, a01, a02 = cz * cy, -sz, cz * sy
    a10, a11, a12 = sz * cy, cz, sz * sy
    return np.stack([a00, a01 * cx + a02 * sx, a01 * -sx + a02 * cx, a10, a11 * cx + a12 * sx, a11 * -sx + a12 * cx], axis=1)


def observation(target, position, orientation, linvel, body_angvel, z):
    """agx_end_to_end_obs.  z: [4, N, 3] standard normals (position, orientation, linvel, angvel) -> obs [N, 15]"""
    z = f32(z)
    with np.errstate(invalid="ignore"):
        e, _ = euler_zyx(orientation)
        e = e + z[1] * STD_EULER
        obs = np.concatenate([(f32(target) - f32(position)) + z[0] * STD_POS, rotation_6d(e), f32(linvel) + z[2] * STD_LINVEL,
                              f32(body_angvel) + z[3] * STD_ANGVEL], axis=1)
    return obs.astype(np.float32)


class TaskRef:
    """The task-side state and the order in which step() touches it."""

    def __init__(self, n):
        self.n = n
        self.actions = np.zeros((n, 4), np.float32)
        self.prev_actions = np.zeros((n, 4), np.float32)
        self.prev_pos_error = np.zeros((n, 3), np.float32)
        self.prev_position = np.zeros((n, 3), np.float32)
        self.target = np.zeros((n, 3), np.float32)

    def pre_step(self, position, actions_in):
        self.actions = rescale(actions_in)
        self.prev_position = f32(position).copy()

    def reward(self, position, orientation, linvel, body_angvel, crashes, sim_steps, episode_len, crash_dist=CRASH_DIST, reset_on_collision=True):
        return reward(self.target, position, orientation, linvel, body_angvel, crashes, sim_steps, self.actions, self.prev_actions,
                      self.prev_pos_error, episode_len, crash_dist, reset_on_collision)

    def observation(self, position, orientation, linvel, body_angvel, z):
        return observation(self.target, position, orientation, linvel, body_angvel, z)

    def after_reset(self, any_reset):
        """the task's own reset_idx(reset_envs) (:146-153, called when some env resets): the target of EVERY env goes back to zero"""
        if any_reset:
            self.target = np.zeros_like(self.target)

    def end_of_step(self, position):
        """:189-190, on the post-reset position"""
        self.prev_actions = self.actions.copy()
        self.prev_pos_error = (self.target - f32(position)).astype(np.float32)
