"""Test helper: numpy-float32 restatement of the three agx_sim2real_* kernels and of the step ordering of the two lmf2 sim2real
set-point tasks.  It is the comparator of the GPU tests (the reference's code does not exist where they run) and is itself pinned
to the reference bit for bit by tests/test_sim2real_tasks.py (tests/golden/sim2real_cr/*.npz: the reference's own code with
correctly rounded elementary functions).

Every array is float32 and every + - * / sqrt one rounded float32 operation; exp / sin / cos / atan2 / asin are evaluated in
float64 and rounded once; the fused multiply-adds inside torch.cross and torch.norm are made explicit (`fma`)."""
import numpy as np

F = np.float32
VELOCITY, ACCELERATION = 0, 1
PI, TWO_PI = F(np.pi), F(2 * np.pi)


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def fma(a, b, c):
    """fmaf: the product of two float32 is exact in float64; one float64 addition, rounded to float32"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _el(fn, *x):
    with np.errstate(invalid="ignore"):
        return fn(*[np.asarray(v, np.float64) for v in x]).astype(np.float32)


def cross(a, b):
    """torch.cross: fma(a_j, b_k, -(a_k b_j))"""
    ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
    bx, by, bz = b[:, 0], b[:, 1], b[:, 2]
    return np.stack([fma(ay, bz, -(az * by)), fma(az, bx, -(ax * bz)), fma(ax, by, -(ay * bx))], axis=1)


def norm3(v):
    """torch.norm(v, dim=1) of [N, 3]: acc = fma(x_k, x_k, acc) from x_0^2"""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.sqrt(fma(z, z, fma(y, y, x * x)))


def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def quat_rotate(q, v):
    w = q[:, 3:4]
    s = F(2.0) * (w * w) - F(1.0)
    c = cross(q[:, 0:3], v)
    d = dot3(q[:, 0:3], v)[:, None]
    return (v * s + c * w * F(2.0)) + q[:, 0:3] * d * F(2.0)


def quat_apply(q, v):
    t = cross(q[:, 0:3], v) * F(2.0)
    u = cross(q[:, 0:3], t)
    return (v + q[:, 3:4] * t) + u


def quat_apply_inverse(q, v):
    return quat_apply(np.concatenate([-q[:, 0:3], q[:, 3:4]], axis=1), v)


def pymod(a, m):
    """torch `%` / torch.remainder with a positive modulus"""
    r = np.fmod(a, m)
    return np.where((r != 0) & (r < 0), r + m, r).astype(np.float32)


def ssa(a):
    return pymod(a + PI, TWO_PI) - PI


def euler_xyz(q):
    """get_euler_xyz_tensor: angles in [0, 2 pi)"""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    roll = _el(np.arctan2, F(2.0) * (w * x + y * z), w * w - x * x - y * y + z * z)
    sinp = F(2.0) * (w * y - z * x)
    pitch = np.where(np.abs(sinp) >= 1, (PI / F(2.0)) * np.sign(sinp), _el(np.arcsin, np.clip(sinp, -1, 1))).astype(np.float32)
    yaw = _el(np.arctan2, F(2.0) * (w * z + x * y), w * w + x * x - y * y - z * z)
    return np.stack([pymod(roll, TWO_PI), pymod(pitch, TWO_PI), pymod(yaw, TWO_PI)], axis=1)


def quat_from_euler_xyz(e):
    roll, pitch, yaw = e[:, 0], e[:, 1], e[:, 2]
    cy, sy = _el(np.cos, yaw * F(0.5)), _el(np.sin, yaw * F(0.5))
    cr, sr = _el(np.cos, roll * F(0.5)), _el(np.sin, roll * F(0.5))
    cp, sp = _el(np.cos, pitch * F(0.5)), _el(np.sin, pitch * F(0.5))
    qw = cy * cr * cp + sy * sr * sp
    qx = cy * sr * cp - sy * cr * sp
    qy = cy * cr * sp + sy * sr * cp
    qz = sy * cr * cp - cy * sr * sp
    return np.stack([qx, qy, qz, qw], axis=1)


def sign0(w):
    """torch.sign: (0 < w) - (w < 0), +0.0 at +-0 and at NaN"""
    return (w > 0).astype(np.float32) - (w < 0).astype(np.float32)


def _exp(x, gain, e):
    return F(gain) * _el(np.exp, (F(-e) * x) * x)


def _abs_exp(x, gain, e):
    return F(gain) * _el(np.exp, F(-e) * np.abs(x))


def _abs_exp_penalty(x, gain, e):
    return F(gain) * (_el(np.exp, F(-e) * np.abs(x)) - F(1.0))


def _sum4(x):
    return ((x[:, 0] + x[:, 1]) + x[:, 2]) + x[:, 3]


def compute_reward(kind, dist, prev_dist, yaw_error, speed, act, prev_act):
    """the two compute_reward functions before the crash handling"""
    pos = (_exp(dist, 2.0, 1.0) + _exp(dist, 3.0, 10.0)) + _abs_exp(dist, 3.0, 50.0)
    if kind == VELOCITY:
        speed_r = _exp(speed, 1.0, 3.0)
        dist_r = (F(20.0) - dist) / F(40.0)
        ap = _sum4(_abs_exp_penalty(act, 0.2, 4.0))
        dp = _sum4(_abs_exp_penalty(act - prev_act, 0.3, 6.0))
        closer = F(400.0) * (prev_dist - dist)
        yaw_r = _abs_exp(yaw_error, 2.0, 3.0)
        total = (pos + dist_r) + pos * ((speed_r + ap) + closer / F(10.0))
        total = (((total + ap) + dp) + closer) + yaw_r
    else:
        close_pos = _exp(dist, 2.0, 1.0)
        speed_r = _exp(speed, 2.0, 2.5)
        ap = _sum4(_abs_exp_penalty(act, 0.3, 4.0))
        dp = _sum4(_abs_exp_penalty(act - prev_act, 0.4, 6.0))
        diff = prev_dist - dist
        closer = np.where(dist < prev_dist, F(400.0) * diff, F(1200.0) * diff).astype(np.float32)
        yaw_r = _abs_exp(yaw_error, 3.0, 5.0)
        total = pos + pos * ((closer / F(9.0) + ap / F(3.0)) + speed_r / F(1.5))
        total = (((((total + ap) + dp) + closer) + yaw_r) + close_pos) + speed_r * F(0.2)
    return (F(1.0) * total).astype(np.float32)


def pre_step(kind, target, position, orientation, actions_before, actions):
    """agx_sim2real_pre_step.  `actions` is changed IN PLACE for the acceleration kind (after `actions_before`, possibly the same
    array, has been read).  -> prev_actions, prev_dist, prev_actions_vehicle_frame (None for the velocity kind)"""
    prev_actions = f32(actions_before).copy()
    prev_dist = norm3(f32(target) - f32(position))
    pavf = None
    if kind == ACCELERATION:
        pavf = np.concatenate([quat_rotate(f32(orientation), prev_actions[:, 0:3]), prev_actions[:, 3:4]], axis=1)
        actions[:, 0:3] = F(2.0) * actions[:, 0:3]
    return prev_actions, prev_dist, pavf


def reward(kind, target, position, orientation, vehicle_orientation, body_linvel, crashes, sim_steps, actions, prev_actions,
           prev_dist, prev_actions_vehicle_frame, episode_len, reset_on_collision=True):
    """agx_sim2real_reward -> dict(reward, crashes, truncations, reset_mask, actions_vehicle_frame)"""
    q, qveh = f32(orientation), f32(vehicle_orientation)
    err = f32(target) - f32(position)
    yaw_error = F(0.0) - ssa(euler_xyz(q))[:, 2]
    speed = norm3(f32(body_linvel))
    avf = None
    if kind == ACCELERATION:
        dist = norm3(quat_apply_inverse(q, err))
        avf = np.concatenate([quat_rotate(qveh, f32(actions)[:, 0:3]), f32(actions)[:, 3:4]], axis=1)
        total = compute_reward(kind, dist, f32(prev_dist), yaw_error, speed, avf, f32(prev_actions_vehicle_frame))
    else:
        dist = norm3(quat_apply_inverse(qveh, err))
        total = compute_reward(kind, dist, f32(prev_dist), yaw_error, speed, f32(actions), f32(prev_actions))
    crash = np.asarray(crashes).astype(bool) | (dist > F(10.0))
    total = np.where(crash, F(-50.0), total).astype(np.float32)
    trunc = np.asarray(sim_steps) > episode_len
    return dict(reward=total, crashes=crash, truncations=trunc, reset_mask=(crash & bool(reset_on_collision)) | trunc,
                actions_vehicle_frame=avf, dist=dist)


def observation(target, position, orientation, body_linvel, body_angvel, robot_actions, z):
    """agx_sim2real_obs.  z: [4, N, 3] standard normals (euler, position, linvel, angvel) -> (obs [N, 17], the orientation as it
    is stored back)"""
    z = f32(z)
    q = f32(orientation)
    q = sign0(q[:, 3])[:, None] * q
    e = ssa(euler_xyz(q)) + z[0] * F(0.02)
    obs = np.concatenate([(f32(target) - f32(position)) + z[1] * F(0.03), quat_from_euler_xyz(e),
                          f32(body_linvel) + z[2] * F(0.02), f32(body_angvel) + z[3] * F(0.02), f32(robot_actions)], axis=1)
    return obs.astype(np.float32), q.astype(np.float32)


class TaskRef:
    """The task-side state of one of the two tasks and the order in which step() touches it."""

    def __init__(self, kind, n):
        self.kind, self.n = kind, n
        self.actions = np.zeros((n, 4), np.float32)  # a REFERENCE to the caller's array after the first step, like the tasks
        self.prev_actions = np.zeros((n, 4), np.float32)
        self.prev_dist = np.zeros(n, np.float32)
        self.actions_vehicle_frame = np.zeros((n, 4), np.float32)
        self.prev_actions_vehicle_frame = np.zeros((n, 4), np.float32)
        self.target = np.zeros((n, 3), np.float32)

    def pre_step(self, position, orientation, actions):
        self.prev_actions, self.prev_dist, pavf = pre_step(self.kind, self.target, position, orientation, self.actions, actions)
        if pavf is not None:
            self.prev_actions_vehicle_frame = pavf
        self.actions = actions

    def reward(self, position, orientation, vehicle_orientation, body_linvel, crashes, sim_steps, episode_len, reset_on_collision=True):
        r = reward(self.kind, self.target, position, orientation, vehicle_orientation, body_linvel, crashes, sim_steps, self.actions,
                   self.prev_actions, self.prev_dist, self.prev_actions_vehicle_frame, episode_len, reset_on_collision)
        if r["actions_vehicle_frame"] is not None:
            self.actions_vehicle_frame = r["actions_vehicle_frame"]
        return r

    def observation(self, position, orientation, body_linvel, body_angvel, robot_actions, z):
        return observation(self.target, position, orientation, body_linvel, body_angvel, robot_actions, z)
