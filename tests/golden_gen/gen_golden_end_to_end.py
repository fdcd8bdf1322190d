"""TEST INFRASTRUCTURE -- golden vectors of the end-to-end motor-command set-point task and its tinyprop airframe, produced by running
the REFERENCE's own code (needs the reference tree, ref_shells.REFERENCE_ROOT; uses the helpers under oracle/ by path).

    python tests/golden_gen/gen_golden_end_to_end.py [--cr] [--out DIR]

writes, into tests/golden/ (tests/golden/end_to_end_cr/ with --cr: the same code with correctly rounded elementary functions,
oracle/cr_torch.py):

  end_to_end_reward.npz   n = 768: inputs and outputs of compute_rewards_and_crashes (position_setpoint_task_sim2real_end_to_end.py
                          :232-252 + :267-309) called as an unbound method on a stand-in object; error lengths on both sides of
                          crash_dist, steps that moved closer and farther, actions at the limits, pre-set crashes
  end_to_end_obs.npz      n = 256: process_obs_for_task (:204-229) the same way; attitudes over the whole sphere, four rows each with
                          the asin argument exactly +-1, one ulp inside and one ulp outside (NaN); the four normal tensors re-drawn
                          from the same seed in the same order and stored as STANDARD normals (z * std is checked here to reproduce
                          what torch.normal(zeros, std) returned, bit for bit)
  end_to_end_glue.npz     the real step() (own constructor, reset, step) for 12 steps on a scripted stand-in for the simulator,
                          with the second reset_idx call of every resetting step and its argument recorded
  end_to_end_config.npz   the scalar values of the task config (JSON) and both action-limit vectors
  step_tinyprop_no_control.npz, step_edge_tinyprop_no_control.npz
                          the reference's BaseMultirotor.step on tinyprop + no_control, recorded by oracle/gen_golden.py's gen_step:
                          64 envs x 2 sub-steps, its nominal source and its edge source
  robot_tinyprop.npz      composite mass, centre of mass, 3 x 3 inertia and motor table of resources/robots/tinyprop/tinyprop.urdf and
                          the numbers of TinyPropCfg, in the keys of robot_lmf2.npz

pytorch3d is not installed where this runs: the four functions the task imports from pytorch3d.transforms are restated below from
pytorch3d's published transforms/rotation_conversions.py (quaternion_to_matrix, _axis_angle_rotation, euler_angles_to_matrix,
_angle_from_tan, _index_from_letter, matrix_to_euler_angles, matrix_to_rotation_6d) and pinned by known-answer tests at start-up.
"""
import json
import math
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg  # noqa: E402  FIRST: it switches TorchScript off before torch is imported (cr_torch.py)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_shells  # noqa: E402

OUT = (sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
       else os.path.join(ROOT, "tests", "golden", *(["end_to_end_cr"] if gg.CR else [])))
TASK = "position_setpoint_task_sim2real_end_to_end"
CONFIG_KEYS = ("seed", "sim_name", "env_name", "robot_name", "controller_name", "num_envs", "use_warp", "headless", "device",
               "observation_space_dim", "privileged_observation_space_dim", "action_space_dim", "episode_len_steps",
               "return_state_before_reset", "crash_dist", "args", "reward_parameters")
NOISE_STD = (0.001, torch.pi / 1032, 0.002, 0.001)  # position, orientation, linear velocity, body angular velocity (:207-218)
ASIN_EDGE = 1.0 - 1e-4  # rows with the asin argument beyond this may be left out of the plain-torch comparison: at most 2 % of rows


# ---------------------------------------------------------------------------------------------------------------------------
# pytorch3d/transforms/rotation_conversions.py, restated
def quaternion_to_matrix(quaternions):
    """rotation_conversions.py: quaternion_to_matrix (real part first)"""
    r, i, j, k = torch.unbind(quaternions, -1)
    two_s = 2.0 / (quaternions * quaternions).sum(-1)
    o = torch.stack(
        (
            1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
            two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
            two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j),
        ),
        -1,
    )
    return o.reshape(quaternions.shape[:-1] + (3, 3))


def _axis_angle_rotation(axis, angle):
    """rotation_conversions.py: _axis_angle_rotation"""
    cos, sin = torch.cos(angle), torch.sin(angle)
    one, zero = torch.ones_like(angle), torch.zeros_like(angle)
    if axis == "X":
        R_flat = (one, zero, zero, zero, cos, -sin, zero, sin, cos)
    elif axis == "Y":
        R_flat = (cos, zero, sin, zero, one, zero, -sin, zero, cos)
    elif axis == "Z":
        R_flat = (cos, -sin, zero, sin, cos, zero, zero, zero, one)
    else:
        raise ValueError("letter must be either X, Y or Z.")
    return torch.stack(R_flat, -1).reshape(angle.shape + (3, 3))


def euler_angles_to_matrix(euler_angles, convention):
    """rotation_conversions.py: euler_angles_to_matrix"""
    if euler_angles.dim() == 0 or euler_angles.shape[-1] != 3:
        raise ValueError("Invalid input euler angles.")
    matrices = [_axis_angle_rotation(c, e) for c, e in zip(convention, torch.unbind(euler_angles, -1))]
    return torch.matmul(torch.matmul(matrices[0], matrices[1]), matrices[2])


def _angle_from_tan(axis, other_axis, data, horizontal, tait_bryan):
    """rotation_conversions.py: _angle_from_tan"""
    i1, i2 = {"X": (2, 1), "Y": (0, 2), "Z": (1, 0)}[axis]
    if horizontal:
        i2, i1 = i1, i2
    even = (axis + other_axis) in ["XY", "YZ", "ZX"]
    if horizontal == even:
        return torch.atan2(data[..., i1], data[..., i2])
    if tait_bryan:
        return torch.atan2(-data[..., i2], data[..., i1])
    return torch.atan2(data[..., i2], -data[..., i1])


def _index_from_letter(letter):
    return {"X": 0, "Y": 1, "Z": 2}[letter]


def matrix_to_euler_angles(matrix, convention):
    """rotation_conversions.py: matrix_to_euler_angles, with the sign rule of the Tait-Bryan central angle; no clamp before asin"""
    i0 = _index_from_letter(convention[0])
    i2 = _index_from_letter(convention[2])
    tait_bryan = i0 != i2
    if tait_bryan:
        central_angle = torch.asin(matrix[..., i0, i2] * (-1.0 if i0 - i2 in [-1, 2] else 1.0))
    else:
        central_angle = torch.acos(matrix[..., i0, i0])
    o = (
        _angle_from_tan(convention[0], convention[1], matrix[..., i2], False, tait_bryan),
        central_angle,
        _angle_from_tan(convention[2], convention[1], matrix[..., i0, :], True, tait_bryan),
    )
    return torch.stack(o, -1)


def matrix_to_rotation_6d(matrix):
    """rotation_conversions.py: matrix_to_rotation_6d"""
    batch_dim = matrix.size()[:-2]
    return matrix[..., :2, :].clone().reshape(batch_dim + (6,))


def install_pytorch3d_stand_ins():
    ref_shells.install()
    t = sys.modules["pytorch3d.transforms"]
    t.quaternion_to_matrix, t.matrix_to_euler_angles = quaternion_to_matrix, matrix_to_euler_angles
    t.euler_angles_to_matrix, t.matrix_to_rotation_6d = euler_angles_to_matrix, matrix_to_rotation_6d


def known_answer_tests():
    """Euler -> matrix -> Euler round trips for every Tait-Bryan convention; "ZYX" against the reference's own quaternion ->
    roll / pitch / yaw (utils/math.py get_euler_xyz_tensor), up to wrapping and away from |pitch| = 90 degrees; known matrices."""
    m = ref_shells.ref("utils.math")
    g = torch.Generator().manual_seed(9)
    e = (torch.rand(512, 3, generator=g, dtype=torch.float64) - 0.5) * torch.tensor([2 * math.pi, 0.98 * math.pi, 2 * math.pi], dtype=torch.float64)
    for conv in ("XYZ", "XZY", "YXZ", "YZX", "ZXY", "ZYX"):
        back = matrix_to_euler_angles(euler_angles_to_matrix(e, conv), conv)
        assert float((back - e).abs().max()) < 1e-9, conv
    half = torch.tensor(math.pi / 2, dtype=torch.float64)
    Rz = euler_angles_to_matrix(torch.stack([half, 0 * half, 0 * half]), "ZYX")  # a quarter turn about z: x -> y
    assert torch.allclose(Rz, torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64), atol=1e-15)
    assert torch.equal(quaternion_to_matrix(torch.tensor([1.0, 0.0, 0.0, 0.0])), torch.eye(3))
    assert matrix_to_rotation_6d(Rz).tolist() == Rz[:2].reshape(6).tolist()
    q = torch.randn(2048, 4, generator=g, dtype=torch.float64)
    q = q / q.norm(dim=1, keepdim=True)
    q = q[(2.0 * (q[:, 3] * q[:, 1] - q[:, 2] * q[:, 0])).abs() < 0.999]
    mine = matrix_to_euler_angles(quaternion_to_matrix(q[:, [3, 0, 1, 2]]), "ZYX")[:, [2, 1, 0]]
    theirs = m.get_euler_xyz_tensor(q)
    d = torch.remainder(mine - theirs + math.pi, 2 * math.pi) - math.pi
    assert float(d.abs().max()) < 1e-9, float(d.abs().max())


# ---------------------------------------------------------------------------------------------------------------------------
def import_on_cpu(name):
    """the task config builds its limit tensors with device="cuda:0" at import: drop the device while it is imported"""
    real = torch.ones
    torch.ones = lambda *a, device=None, **k: real(*a, **k)
    try:
        return ref_shells.ref(name)
    finally:
        torch.ones = real


def task_module():
    name = "aerial_gym.task." + TASK
    if name not in sys.modules:  # (task/__init__.py registers every task: ref_shells bypasses it, sub-package by sub-package)
        sp = types.ModuleType(name)
        sp.__path__ = [os.path.join(ref_shells.REFERENCE_ROOT, "aerial_gym", "task", TASK)]
        sys.modules[name] = sp
    return ref_shells.ref("task.%s.%s" % (TASK, TASK))


def task_config():
    return import_on_cpu("config.task_config.%s_config" % TASK).task_config


def unit_quats(n, rng):
    q = torch.randn(n, 4, generator=rng)
    return q / q.norm(dim=1, keepdim=True)


def gen_reward(rng):
    n = 768
    cls = task_module().PositionSetpointTaskSim2RealEndToEnd
    cfg = task_config()
    u = torch.rand(n, generator=rng)
    length = torch.where(u < 0.1, torch.rand(n, generator=rng) * 0.1,
                         torch.where(u > 0.8, cfg.crash_dist + (torch.rand(n, generator=rng) - 0.5) * 0.4, torch.rand(n, generator=rng) * 3.0))
    d = torch.randn(n, 3, generator=rng)
    err = d / d.norm(dim=1, keepdim=True) * length.unsqueeze(1)
    target = (torch.rand(n, 3, generator=rng) - 0.5) * 2.0
    position = target - err
    q = gg.random_state(n, rng)[:, 3:7]
    q[::5] = unit_quats(n, rng)[::5]  # any attitude, either sign of w
    linvel = torch.randn(n, 3, generator=rng) * 0.5
    linvel[::6] *= 0.05
    wbody = torch.randn(n, 3, generator=rng) * 0.5
    wbody[::4] *= 0.05
    crashes = torch.rand(n, generator=rng) < 0.1
    prev_pos_error = (target - position) * (1.0 + torch.randn(n, 1, generator=rng) * 0.03)  # the step moved closer or farther
    prev_pos_error[::11] = (target - position)[::11]  # ... or not at all: closer_by_dist == 0 takes the `>= 0` side
    lo, hi = float(cfg.action_limit_min[0]), float(cfg.action_limit_max[0])
    actions = lo + torch.rand(n, 4, generator=rng) * (hi - lo)
    prev_actions = lo + torch.rand(n, 4, generator=rng) * (hi - lo)
    actions[::7] = cfg.action_limit_max
    actions[3::7] = cfg.action_limit_min
    prev_actions[::14] = cfg.action_limit_min
    fake = types.SimpleNamespace(target_position=target, actions=actions, prev_actions=prev_actions, prev_pos_error=prev_pos_error,
                                 task_config=types.SimpleNamespace(crash_dist=cfg.crash_dist))
    obs_dict = {"robot_position": position, "robot_linvel": linvel, "robot_orientation": q, "robot_body_angvel": wbody, "crashes": crashes.clone()}
    inputs = {k: v.clone() for k, v in (("actions", actions), ("prev_actions", prev_actions), ("prev_pos_error", prev_pos_error))}
    reward, crashes_out = cls.compute_rewards_and_crashes(fake, obs_dict)
    for k, v in inputs.items():
        assert torch.equal(v, getattr(fake, k)), k  # (the function works on clones: the task's tensors stay as they were)
    rec = dict(target=target, position=position, orientation=q, linvel=linvel, body_angvel=wbody, crashes_in=crashes, reward=reward,
               crashes_out=crashes_out, crash_dist=torch.tensor(cfg.crash_dist, dtype=torch.float64), **inputs)
    np.savez(os.path.join(OUT, "end_to_end_reward.npz"), **{k: v.numpy().copy() for k, v in rec.items()})
    dist, prev = (target - position).norm(dim=1), prev_pos_error.norm(dim=1)
    print("end_to_end_reward mean %.4f  inside 0.1 m: %d  beyond crash_dist: %d  crashed: %d -> %d  closer / equal / farther: %d / %d / %d" % (
        float(reward.mean()), int((dist < 0.1).sum()), int((dist > cfg.crash_dist).sum()), int(crashes.sum()), int(crashes_out.sum()),
        int((dist < prev).sum()), int((dist == prev).sum()), int((dist > prev).sum())))


def asin_argument(q_xyzw):
    """the argument process_obs_for_task hands to asin, in its own float32 arithmetic"""
    return -quaternion_to_matrix(q_xyzw[:, [3, 0, 1, 2]])[:, 2, 0]


def asin_edge_rows(rng):
    """quaternions next to a pitch of +-90 degrees whose asin argument is, in float32: exactly +-1, one ulp inside, one ulp outside
    (four rows each, both signs)"""
    one = np.float32(1.0)
    want = {"exact": one, "inside": np.nextafter(one, np.float32(0.0)), "outside": np.nextafter(one, np.float32(2.0))}
    found = {k: [] for k in want}
    s = math.sqrt(0.5)
    for _ in range(400):
        m = 4096
        yaw = (torch.rand(m, generator=rng) - 0.5) * 2 * math.pi
        sign = torch.where(torch.rand(m, generator=rng) < 0.5, -1.0, 1.0)
        # pitch of +-90 degrees composed with a yaw, scaled and perturbed by a few ulps
        q = torch.stack([-s * torch.sin(yaw / 2) * sign, s * torch.cos(yaw / 2) * sign, s * torch.sin(yaw / 2), s * torch.cos(yaw / 2)], dim=1)
        q = (q * (1.0 + (torch.rand(m, 1, generator=rng) - 0.5) * 1e-3) + (torch.rand(m, 4, generator=rng) - 0.5) * 4e-7).float()
        a = asin_argument(q).numpy()
        for name, v in want.items():
            for sg in (1.0, -1.0):
                rows = np.nonzero(a == np.float32(sg) * v)[0]
                have = sum(1 for _, s_ in found[name] if s_ == sg)
                for r in rows[: max(0, 2 - have)]:
                    found[name].append((q[r].clone(), sg))
        if all(len(v) >= 4 for v in found.values()):
            break
    assert all(len(v) >= 4 for v in found.values()), {k: len(v) for k, v in found.items()}
    return torch.stack([q for name in ("exact", "inside", "outside") for q, _ in found[name][:4]])


def gen_obs(rng):
    n = 256
    cls = task_module().PositionSetpointTaskSim2RealEndToEnd
    assert open(task_module().__file__).read().count("torch.normal(") == 4
    state = gg.random_state(n, rng, spread=1.0)
    state[:, 3:7] = unit_quats(n, rng)  # attitudes over the whole sphere
    edge = asin_edge_rows(rng)
    state[0:12, 3:7] = edge
    arg = asin_argument(state[:, 3:7])
    assert (arg[0:4].abs() == 1).all() and (arg[4:8].abs() < 1).all() and (arg[8:12].abs() > 1).all()
    beyond = int((arg.abs() > ASIN_EDGE).sum())
    assert beyond >= 12 and beyond - 12 <= 0.02 * n, beyond  # the cap of the plain-torch comparison: 2 % of rows next to the 12 edge rows
    target = (torch.rand(n, 3, generator=rng) - 0.5) * 2.0
    wbody = torch.randn(n, 3, generator=rng)
    fake = types.SimpleNamespace(
        target_position=target, rewards=torch.zeros(n), terminations=torch.zeros(n, dtype=torch.bool), truncations=torch.zeros(n, dtype=torch.bool),
        obs_dict={"robot_position": state[:, 0:3], "robot_orientation": state[:, 3:7], "robot_linvel": state[:, 7:10], "robot_body_angvel": wbody},
        task_obs={"observations": torch.zeros(n, 15)})
    state_in = state.clone()
    torch.manual_seed(31)
    cls.process_obs_for_task(fake)
    assert torch.equal(state, state_in)
    torch.manual_seed(31)  # the same draws again, as the task made them (:207-218): position, orientation, linvel, angvel
    scaled = [torch.normal(mean=torch.zeros(n, 3), std=s) for s in NOISE_STD]
    torch.manual_seed(31)
    z = [torch.randn(n, 3) for _ in NOISE_STD]
    for zk, sk, std in zip(z, scaled, NOISE_STD):
        assert torch.equal(zk * std, sk), "z * std does not reproduce torch.normal(zeros, std): store the scaled draws instead"
    obs = fake.task_obs["observations"]
    nan_rows = torch.isnan(obs).any(dim=1)
    assert nan_rows[8:12].all() and int(nan_rows.sum()) == int((arg.abs() > 1).sum())
    np.savez(os.path.join(OUT, "end_to_end_obs.npz"), state=state_in.numpy(), target=target.numpy(), body_angvel=wbody.numpy(),
             z=torch.stack(z).numpy(), obs=obs.numpy(), asin_argument=arg.numpy())
    print("end_to_end_obs: ok  |asin argument| > %g: %d of %d  NaN rows: %d  edge arguments:" % (ASIN_EDGE, beyond, n, int(nan_rows.sum())),
          ["%.9g" % v for v in arg[0:12].tolist()])


N_GLUE, T_GLUE, EPISODE_GLUE = 48, 12, 5


class ScriptedSim:
    """EnvManager stand-in: the tensors the task reads, advanced from a pre-drawn script; reset_idx calls are recorded"""

    def __init__(self, g):
        N = N_GLUE
        self.num_envs, self.g = N, g
        z = torch.zeros
        self.d = {"robot_position": z(N, 3), "robot_orientation": z(N, 4), "robot_linvel": z(N, 3), "robot_body_angvel": z(N, 3),
                  "crashes": z(N, dtype=torch.bool), "truncations": z(N, dtype=torch.bool)}
        self.sim_steps = torch.zeros(N, dtype=torch.int32)
        self.sim_steps[: N // 2] = 2  # two phases of episodes: truncations on different steps
        self.log, self.reset_idx_calls, self.t = [], [], -1
        self._draw(torch.arange(N))

    def _draw(self, ids):
        g, d, k = self.g, self.d, len(ids)
        far = (torch.rand(k, generator=g) < 0.08) & (self.t % 3 == 1)  # distance crashes in some steps, none in others
        d["robot_position"][ids] = torch.randn(k, 3, generator=g) * torch.where(far, 2.0, 0.3).unsqueeze(1)
        d["robot_orientation"][ids] = unit_quats(k, g)
        d["robot_linvel"][ids] = torch.randn(k, 3, generator=g) * 0.5
        d["robot_body_angvel"][ids] = torch.randn(k, 3, generator=g) * 0.5

    def get_obs(self):
        return self.d

    def reset(self):
        pass

    def step(self, actions):
        d = self.d
        self.sim_steps += 1
        self.t += 1
        self.actions_seen = actions.clone()
        self._draw(torch.arange(self.num_envs))
        d["crashes"][:] = (torch.rand(self.num_envs, generator=self.g) < 0.04) & (self.t % 3 == 1)
        self.log.append({k: d[k].clone() for k in ("robot_position", "robot_orientation", "robot_linvel", "robot_body_angvel", "crashes")})
        self.log[-1]["sim_steps"] = self.sim_steps.clone()
        self.log[-1]["sim_actions"] = self.actions_seen
        self.reset_idx_calls = []

    def _reset(self, ids):
        self._draw(ids)
        self.sim_steps[ids] = 0

    def post_reward_calculation_step(self):
        d = self.d
        ids = torch.nonzero(d["crashes"] | d["truncations"]).squeeze(-1)
        if len(ids) > 0:
            self._reset(ids)
        mask = torch.zeros(self.num_envs, dtype=torch.uint8)
        mask[ids] = 1
        self.log[-1].update(reset_mask=mask, **{"first_" + k: d[k].clone() for k in ("robot_position", "robot_orientation")})
        return ids

    def reset_idx(self, env_ids):  # the task's own reset_idx calls this a SECOND time for the same envs (:180-182)
        self.reset_idx_calls.append(env_ids.clone())
        self._reset(env_ids)

    def delete_env(self):
        pass


def gen_glue():
    mod = task_module()
    g = torch.Generator().manual_seed(779)
    sim = ScriptedSim(g)

    class Builder:
        def build_env(self, **kw):
            return sim

    mod.SimBuilder = Builder
    ref_cfg = task_config()

    class cfg(ref_cfg):
        num_envs = N_GLUE
        device = "cpu"
        headless = True
        episode_len_steps = EPISODE_GLUE

    cfg.reward_parameters = dict(ref_cfg.reward_parameters)
    task = mod.PositionSetpointTaskSim2RealEndToEnd(cfg)
    torch.manual_seed(100)
    task.reset()
    out = {"episode_len_steps": np.int64(EPISODE_GLUE), "crash_dist": np.float64(cfg.crash_dist)}
    rows = {}

    def keep(name, v):
        rows.setdefault(name, []).append(v.clone().numpy())

    keep_attr0 = {k: getattr(task, k).clone().numpy() for k in ("prev_actions", "prev_pos_error", "prev_position", "action_history")}
    assert not any(v.any() for v in keep_attr0.values())  # zero before the first step
    for t in range(T_GLUE):
        a = (torch.rand(N_GLUE, 4, generator=g) - 0.5) * (3.0 if t % 4 == 3 else 2.0)  # beyond +-1 every fourth step: the clamp
        handed = a.clone()
        if t == 6:
            task.target_position[::9, 0] = 3.0  # a moved set-point: distance crashes
        keep("target", task.target_position)
        keep("action_in", handed)
        keep("pre_position", sim.d["robot_position"])
        torch.manual_seed(1000 + t)
        obs, rewards, terminations, truncations, _ = task.step(handed)
        torch.manual_seed(1000 + t)
        keep("z", torch.stack([torch.randn(N_GLUE, 3) for _ in NOISE_STD]))
        assert torch.equal(handed, a) and task.actions is not handed  # the caller's tensor: neither kept nor changed
        log = sim.log[-1]
        for k, v in log.items():
            keep(k, v)
        second = torch.zeros(N_GLUE, dtype=torch.uint8)
        assert len(sim.reset_idx_calls) == (1 if log["reset_mask"].any() else 0)
        for ids in sim.reset_idx_calls:
            second[ids] = 1
        keep("second_reset_mask", second)  # the argument of the task's own reset_idx call: the same envs again
        for k, v in (("actions", task.actions), ("prev_actions", task.prev_actions), ("prev_pos_error", task.prev_pos_error),
                     ("prev_position", task.prev_position), ("rewards", rewards), ("terminations", terminations), ("truncations", truncations),
                     ("observations", obs["observations"]), ("action_history", task.action_history)):
            keep(k, v)
        for k in ("robot_position", "robot_orientation", "robot_linvel", "robot_body_angvel"):
            keep("post_" + k, sim.d[k])
    for k, v in rows.items():
        out[k] = np.stack(v)
    assert np.array_equal(out["second_reset_mask"], out["reset_mask"]) and not out["action_history"].any()
    resets = out["reset_mask"].any(axis=1)
    assert resets.any() and not resets.all()
    moved = [bool((out["first_robot_position"][t] != out["post_robot_position"][t]).any()) for t in range(T_GLUE)]
    assert moved == resets.tolist()  # the final state is the SECOND reset's
    print("end_to_end_glue resets %d in steps %s  truncations %d  crashes in / out %d / %d" % (
        int(out["reset_mask"].sum()), np.nonzero(resets)[0].tolist(), int(out["truncations"].sum()), int(out["crashes"].sum()),
        int(out["terminations"].sum())))
    np.savez(os.path.join(OUT, "end_to_end_glue.npz"), **out)


def gen_config():
    c = task_config()
    src = open(import_on_cpu("config.task_config.%s_config" % TASK).__file__).read()
    assert "torch.ones(action_space_dim,device=device)" in src and c.device == "cuda:0"  # the limits are made on cuda:0 at import there
    np.savez(os.path.join(OUT, "end_to_end_config.npz"), config=np.array(json.dumps({k: getattr(c, k) for k in CONFIG_KEYS}, sort_keys=True)),
             action_limit_min=c.action_limit_min.numpy(), action_limit_max=c.action_limit_max.numpy())
    print("end_to_end_config:", {k: getattr(c, k) for k in CONFIG_KEYS}, c.action_limit_min.tolist(), c.action_limit_max.tolist())


def tinyprop_links():
    return gg.parse_urdf(os.path.join(ref_shells.REFERENCE_ROOT, "resources", "robots", "tinyprop", "tinyprop.urdf"))


def gen_steps():
    """gen_golden.robot_constants for tinyprop (its collision shape is a box, which that function does not read) + gen_step"""
    cfg = ref_shells.ref("config.robot_config.tinyprop_config").TinyPropCfg
    links = tinyprop_links()
    mass, com, J = gg.composite(links)
    ca = cfg.control_allocator_config
    cq = ca.motor_model_config.thrust_to_torque_ratio
    W = np.zeros((6, ca.num_motors))
    for i in range(ca.num_motors):
        link = links["motor_%d" % i]
        ez = link["R"][:, 2]
        W[0:3, i] = ez
        W[3:6, i] = np.cross(link["xyz"] - com, ez) - cq * ca.motor_directions[i] * ez
    consts = dict(mass=np.float64(mass), com=com, inertia=J, wrench_map=W, alloc=np.array(ca.allocation_matrix, dtype=np.float64),
                  collision_radius=np.float64(0.055))
    gg.OUT = OUT  # (gen_step writes next to the other fixtures of this generator, not into oracle/gen_golden.py's fixed file set)
    gg.gen_step("tinyprop", cfg, "no_control", "no_control", consts, n=64, K=2, seed=7)
    gg.gen_step("tinyprop", cfg, "no_control", "no_control", consts, n=64, K=2, seed=11, source=gg.EdgeSource())


def gen_robot():
    cfg = ref_shells.ref("config.robot_config.tinyprop_config").TinyPropCfg
    links = tinyprop_links()
    mass, com, J = gg.composite(links)
    ca = cfg.control_allocator_config
    mm = ca.motor_model_config
    motors = ["motor_%d" % i for i in range(ca.num_motors)]
    arms = ["arm_motor_%d" % i for i in range(ca.num_motors)]
    out = dict(mass=np.float64(mass), com=com, inertia=J, alloc=np.array(ca.allocation_matrix, np.float64),
               base_mass=np.float64(links["base_link"]["mass"]), base_inertia=links["base_link"]["inertia"],
               motor_mass=np.float64(links[motors[0]]["mass"]), motor_inertia=links[motors[0]]["inertia"],
               motor_pos=np.array([links[p]["xyz"] for p in motors]), motor_rpy=np.array([links[p]["rpy"] for p in motors], np.float64),
               arm_mass=np.float64(links[arms[0]]["mass"]), arm_inertia=links[arms[0]]["inertia"],
               arm_pos=np.array([links[p]["xyz"] for p in arms]), arm_rpy=np.array([links[p]["rpy"] for p in arms], np.float64),
               collision_radius=np.float64(0.055), force_application_level=np.array(ca.force_application_level),
               application_mask=np.array(ca.application_mask), motor_directions=np.array(ca.motor_directions),
               motor_model=np.array([mm.motor_thrust_constant_min, mm.motor_thrust_constant_max, mm.motor_time_constant_increasing_min,
                                     mm.motor_time_constant_increasing_max, mm.motor_time_constant_decreasing_min,
                                     mm.motor_time_constant_decreasing_max, mm.max_thrust, mm.min_thrust, mm.max_thrust_rate,
                                     mm.thrust_to_torque_ratio], np.float64),
               motor_model_flags=np.array(json.dumps(dict(use_rps=mm.use_rps, use_discrete_approximation=mm.use_discrete_approximation,
                                                          integration_scheme=mm.integration_scheme))),
               min_init_state=np.array(cfg.init_config.min_init_state, np.float64), max_init_state=np.array(cfg.init_config.max_init_state, np.float64),
               disturbance=np.array([float(cfg.disturbance.enable_disturbance), cfg.disturbance.prob_apply_disturbance]
                                    + list(cfg.disturbance.max_force_and_torque_disturbance), np.float64),
               sensors=np.array([cfg.sensor_config.enable_camera, cfg.sensor_config.enable_lidar, cfg.sensor_config.enable_imu]),
               damping=np.array([cfg.robot_asset.linear_damping, cfg.robot_asset.angular_damping], np.float64))
    # every joint of this URDF hangs off base_link (parse_urdf places links by their own joint): say so, the fixture relies on it
    import xml.etree.ElementTree as ET

    urdf = ET.parse(os.path.join(ref_shells.REFERENCE_ROOT, "resources", "robots", "tinyprop", "tinyprop.urdf")).getroot()
    assert {j.find("parent").get("link") for j in urdf.findall("joint")} == {"base_link"}
    np.savez(os.path.join(OUT, "robot_tinyprop.npz"), **out)
    print("robot_tinyprop: mass %.9g  com %s\n%s" % (mass, com, J))


def main():
    os.makedirs(OUT, exist_ok=True)
    ref_shells.install()
    ref_shells.install_task_shells()
    install_pytorch3d_stand_ins()
    known_answer_tests()
    rng = torch.Generator().manual_seed(20253)
    gen_reward(rng)
    gen_obs(rng)
    gen_glue()
    gen_config()
    gen_steps()
    if not gg.CR:  # (no elementary function in it: one copy)
        gen_robot()


if __name__ == "__main__":
    main()
