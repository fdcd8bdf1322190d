"""GPU: the dynamics kernels over ALL attitudes and at the controllers' edge inputs.

Every other device test of the dynamics path starts from nominal flight (tilt <= 65 deg, |v| <= 1.4 m/s).  The edge fixtures
tests/golden/step_edge_<robot>_<ctrl>.npz (tests/edge_cases_util.py, oracle/gen_golden.py EdgeSource: the reference's
BaseMultirotor.step recorded on 96 envs x 2 chained sub-steps) hold what nominal flight never reaches: the |sinp| >= 1 clamp of
get_euler_xyz, atan2 with a zero / negative denominator on an inverted vehicle, roll / pitch / yaw either side of 0, pi and 2 pi,
the four branches of matrix_to_quaternion (>= 37 rows each per position / velocity case), f = 0 and f below the horizon, the
fully-actuated |q| < 1e-9 floor, velocities and actions beyond their clamps, motor thrusts at their limits and negative.

Five formulations of the same per-env arithmetic are held to them: the one-lane k_env_step<M, CTRL> (b), the four-lanes-per-env
k_env_step_quad_position / k_env_step_quad_loop<M, CTRL> wherever an env sits in its wave (c), the fused single-launch position
step with its helper wave (d), and the stand-alone agx_update_states (a) -- against the CPU oracle bit for bit, against the
reference evaluated with correctly rounded functions bit for bit, and against the reference's recorded numbers within 1e-5."""
import ctypes as C

import numpy as np
import pytest
import torch
from aerial_gym_simulator_amd import _lib
from conftest import elem_err, golden_params, load_golden, max_abs
from edge_cases_util import EDGE_CASES, TOL, angle_err, arrangement

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EXACT = 0.0
QUAD_KERNEL_CASES = ["edge_" + c for c in ("quad_position", "quad_velocity", "quad_attitude", "quad_rates", "quad_acceleration",
                                           "quad_velocity_steering", "octarotor_fully_actuated", "octarotor_position",
                                           "octarotor_velocity")]


def _split(d):
    return dict(euler=d[:, 0:3], qveh=d[:, 3:7], vveh=d[:, 7:10], vbody=d[:, 10:13], wbody=d[:, 13:16])


def _update_states(pd, state):
    from gpu_harness import DynHarness

    H = DynHarness(pd, state.shape[0])
    H.set(state=state)
    H.update_states()
    return _split(H.get("derived"))


# ---------------------------------------------------------------------------------------------------------------- (a)
def test_update_states_over_the_sphere(orc, parity):
    """agx_update_states on the 256 quaternions of math_utils.npz (uniform on the sphere; its `v` as both velocities): the oracle's
    update_states bit for bit, the reference's helpers (get_euler_xyz + ssa, vehicle_frame_quat_from_quat, quat_rotate_inverse)
    within 1e-5, the same helpers evaluated with correctly rounded functions bit for bit."""
    pd = golden_params(load_golden("step_edge_quad_position"))
    for cr in (False, True):
        g = load_golden("math_utils", cr=cr)
        n = g["q"].shape[0]
        state = np.zeros((n, 13), np.float32)
        state[:, 3:7], state[:, 7:10], state[:, 10:13] = g["q"], g["v"], g["v"]
        got = _update_states(pd, state)
        tilt = 1.0 - 2.0 * (g["q"][:, 0] ** 2 + g["q"][:, 1] ** 2)  # body z . world z
        assert (tilt < 0).sum() > n // 3  # inverted attitudes: what nominal flight never shows
        if cr:
            tag = "update_states_vs_reference_with_correctly_rounded_functions[math_utils]"
            for name, x, ref in (("euler", got["euler"], g["ssa_euler"]), ("qveh", got["qveh"], g["vehicle_quat"]),
                                 ("vbody", got["vbody"], g["quat_rotate_inverse"]), ("wbody", got["wbody"], g["quat_rotate_inverse"])):
                parity.check(f"{tag}/{name}", max_abs(x, ref), EXACT, "abs (bit-exact)")
            continue
        o = dict(zip(("euler", "qveh", "vveh", "vbody", "wbody"), orc.update_states(state)))
        parity.check("update_states_euler_vs_oracle[math_utils]", angle_err(got["euler"], o["euler"]), EXACT, "rad (bit-exact)")
        for name in ("qveh", "vveh", "vbody", "wbody"):
            parity.check(f"update_states_{name}_vs_oracle[math_utils]", max_abs(got[name], o[name]), EXACT, "abs (bit-exact)")
        parity.check("update_states_euler_vs_reference[math_utils]", angle_err(got["euler"], g["ssa_euler"]), TOL, "rad")
        parity.check("update_states_qveh_vs_reference[math_utils]", elem_err(got["qveh"], g["vehicle_quat"]), TOL, "|err| / max(1, |x|)")
        for name in ("vbody", "wbody"):
            parity.check(f"update_states_{name}_vs_reference[math_utils]", elem_err(got[name], g["quat_rotate_inverse"]), TOL,
                         "|err| / max(1, |x|)")


@pytest.mark.parametrize("case", ["edge_quad_position", "edge_octarotor_velocity"])
def test_update_states_on_the_edge_table(orc, parity, case):
    """agx_update_states on the edge table's states (both recorded sub-steps: the special attitudes, then what one sub-step makes
    of them): oracle bit for bit, the reference's recorded derived tensors within 1e-5, the correctly rounded reference bit for bit"""
    for cr in (False, True):
        g = load_golden("step_" + case, cr=cr)
        pd = golden_params(g)
        for k in range(g["state"].shape[0]):
            state = g["state"][k]
            got = _update_states(pd, state)
            if cr:
                for name in ("euler", "qveh", "vveh", "vbody", "wbody"):
                    parity.check(f"update_states_vs_reference_with_correctly_rounded_functions[{case}]/{name}", max_abs(got[name], g[name][k]),
                                 EXACT, "abs (bit-exact)", k)
                continue
            o = dict(zip(("euler", "qveh", "vveh", "vbody", "wbody"), orc.update_states(state)))
            parity.check(f"update_states_euler_vs_oracle[{case}]", angle_err(got["euler"], o["euler"]), EXACT, "rad (bit-exact)", k)
            parity.check(f"update_states_euler_vs_reference[{case}]", angle_err(got["euler"], g["euler"][k]), TOL, "rad", k)
            for name in ("qveh", "vveh", "vbody", "wbody"):
                parity.check(f"update_states_{name}_vs_oracle[{case}]", max_abs(got[name], o[name]), EXACT, "abs (bit-exact)", k)
                parity.check(f"update_states_{name}_vs_reference[{case}]", elem_err(got[name], g[name][k]), TOL, "|err| / max(1, |x|)", k)


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("case", EDGE_CASES)
def test_single_substep_one_lane_kernels_on_the_edge_table(orc, parity, case):
    """the comparison of test_gpu_dynamics.test_single_substep_vs_oracle_and_golden on the edge fixtures, one lane per env
    (k_env_step<M, CTRL>): the oracle and the correctly rounded reference bit for bit; the reference's recorded state, thrust (over
    the full-scale thrust), derived tensors and wrench within 1e-5, at most 1 % of an array where the reference is undefined"""
    from test_gpu_dynamics import single_substep_vs_oracle_and_golden

    _lib.set_option("env_step_quad", 0)
    single_substep_vs_oracle_and_golden(orc, parity, case, edge=True)


# ---------------------------------------------------------------------------------------------------------------- (c)
def _run_arranged(g, pd, k, idx, quad):
    """k sub-steps from each recorded sub-step of fixture `g`, the batch holding the table's envs `idx` in that order ->
    (kernel name, [per recorded sub-step: {buffer: rows in the batch's order}])"""
    from gpu_harness import DynHarness

    _lib.set_option("env_step_quad", int(quad))
    n = len(idx)
    H = DynHarness(pd, n)
    H.set(kT=g["kT"][idx], tau_inc=g["tau_inc"][idx], tau_dec=g["tau_dec"][idx])
    H.set_gains(g["Kp"][idx], g["Kv"][idx], g["KR"][idx], g["Kw"][idx])
    buf = C.create_string_buffer(128)
    H.lib.agx_env_step_kernel(H.P, H.B, n, k, None, buf, 128)
    out = []
    for s in range(g["state"].shape[0]):
        H.set(state=g["state"][s][idx], thrust=g["thrust_in"][s][idx])
        if g["disturb"].any():  # the octarotor's recorded disturbance draws, the same in each of the k sub-steps
            H.set_disturb(np.repeat(g["disturb"][s][idx][None], k, axis=0), g["disturb_max"])
        H.substeps(g["action"][s][idx], k)
        out.append({x: H.get(x).copy() for x in ("state", "thrust", "derived", "wrench")})
    return buf.value.decode(), out


@pytest.mark.parametrize("case", QUAD_KERNEL_CASES)
@pytest.mark.parametrize("k", [1, 4])
def test_four_lane_kernels_equal_one_lane_kernels_wherever_an_env_sits(case, k):
    """k sub-steps from the edge table through the four-lanes-per-env kernel and through the one-lane kernel, the env order
    rotated by 0, 1, 2, 3 and 17 (every edge row in every lane group of its wave, next to neighbours that take other branches)
    and the batch cut to 83 envs (no multiple of 16 or 64: the last wave is partial and ends inside a group of four envs):
    every env's state / thrust / derived tensors / wrench are the same bits in all of them."""
    g = load_golden("step_" + case)
    pd = golden_params(g)
    n = g["state"].shape[1]
    base_name, base = _run_arranged(g, pd, k, arrangement(n), quad=0)
    octa = "octarotor" in case
    for rotate, cut in ((0, None), (1, None), (2, None), (3, None), (17, None), (0, 83), (2, 83)):
        idx = arrangement(n, rotate, cut)
        for quad in (0, 1):
            name, got = _run_arranged(g, pd, k, idx, quad)
            if quad:
                assert name.startswith("k_env_step_quad_position" if (case == "edge_quad_position" and k == 1) else "k_env_step_quad_loop<"), name
            else:
                assert name.startswith("k_env_step<8," if octa else "k_env_step<4,"), name
            for s, (a, b) in enumerate(zip(base, got)):
                for buf in a:
                    same = (a[buf][idx].view(np.uint32) == b[buf].view(np.uint32)).all(axis=1)
                    assert same.all(), (case, k, "rotate", rotate, "cut", cut, "quad", quad, "sub-step", s, buf,
                                        "table rows", idx[~same][:8].tolist(), "batch positions", np.nonzero(~same)[0][:8].tolist())


# ---------------------------------------------------------------------------------------------------------------- (d)
@pytest.fixture
def _position_task_config():
    """the task config class this file changes"""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config.task_config import position_setpoint_task_config as cfg

    old = (cfg.device, cfg.controller_name, cfg.episode_len_steps, cfg.args)
    yield cfg
    cfg.device, cfg.controller_name, cfg.episode_len_steps, cfg.args = old
    _lib.set_option("single_launch_step", 1)


def _npy(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x.astype(np.int64)


def edge_position_scenario(n, L):
    """(state, motor thrusts, sim_steps) of test_fused_position_step_from_edge_states: the edge table tiled over n envs; in each
    of the first five waves one env just outside the 8 m crash radius (at rest) and one just inside, flying outward; every
    fifth env 1 .. 5 steps from its truncation"""
    e = load_golden("step_edge_quad_position")
    rows = np.arange(n) % e["state"].shape[1]
    state, thrust = e["state"][0][rows].copy(), e["thrust_in"][0][rows].copy()
    outside, inside = np.arange(3, n, 16)[:5], np.arange(7, n, 16)[:5]
    state[outside, 0:3] = np.array([0.0, 8.01, 0.0], np.float32)
    state[outside, 7:10] = 0.0
    state[inside, 0:3] = np.array([7.985, 0.0, 0.0], np.float32)
    state[inside, 7:10] = np.array([1.0, 0.0, 0.0], np.float32)  # inside after the first step, across the radius in the second
    steps = np.zeros(n, np.int32)
    trunc = np.arange(1, n, 5)
    steps[trunc] = L - 1 - (trunc // 5) % 5  # these truncate in steps 2 .. 6, in the waves of the crashing envs among others
    return state, thrust, steps


@pytest.mark.parametrize("n", [83, 333])
def test_fused_position_step_from_edge_states(orc, _position_task_config, n):
    """position_setpoint_task (Lee position control, device RNG) with every env's state and motor thrusts overwritten by rows of
    the edge table through the public tensors, a few envs just inside (flying outward) and just outside the 8 m crash radius,
    episode counters staggered so that truncations, crashes and envs without a reset share a wave: 12 steps of the single-launch
    task (k_position_step_fused, helper wave) and of its two-launch twin, bit for bit equal to each other and to the oracle's
    env loop at every step -- state, thrust, reward, observation, crash / truncation flags, reset mask."""
    from aerial_gym_simulator_amd.registry.task_registry import task_registry
    from oracle_env import OraclePositionEnv
    from test_gpu_single_launch_step import _assert_same

    cfg = _position_task_config
    L, T, seed = 30, 12, 0x5EED0123456789
    cfg.device, cfg.controller_name, cfg.episode_len_steps = DEV, "lee_position_control", L
    tasks = []
    for single in (False, True):
        cfg.args = {"strict_rng": False, "rng_seed": seed, "single_launch_step": single}
        tasks.append(task_registry.make_task("position_setpoint_task", seed=5, num_envs=n, headless=True))
    plain, fused = tasks
    assert fused._proof_watch is not None and plain._proof_watch is None
    state, thrust, steps = edge_position_scenario(n, L)
    for task in tasks:
        task.reset()
        g = task.sim_env.global_tensor_dict
        mm = task.sim_env.robot_manager.robot.control_allocator.motor_model
        g["robot_state_tensor"][:] = torch.from_numpy(state).to(DEV)
        mm.current_motor_thrust[:] = torch.from_numpy(thrust).to(DEV)
        task.sim_env.sim_steps.copy_(torch.from_numpy(steps).to(DEV))
        task.sim_env.robot_manager.robot.update_states()  # the derived tensors of the new state, as the reset path leaves them
    torch.cuda.synchronize()
    _assert_same(plain, fused, -1)

    env = fused.sim_env
    g = env.global_tensor_dict
    robot = env.robot_manager.robot
    mm = robot.control_allocator.motor_model
    assert np.array_equal(_npy(g["robot_state_tensor"]), state) and np.array_equal(_npy(mm.current_motor_thrust), thrust)
    pd = dict(robot.params_dict)
    M = pd["num_motors"]
    ctrl = robot.controller
    gains = [np.tile(((np.array(ctrl.gains_max, np.float32) + np.array(ctrl.gains_min, np.float32)) / np.float32(2))[3 * k:3 * k + 3], (n, 1))
             for k in range(4)]
    ranges = dict(mm.ranges)
    ranges.setdefault("thrust", (float(pd["min_thrust"]), float(pd["max_thrust"])))
    ec = env.cfg.env
    bcfg = [np.array(x, np.float32) for x in (ec.lower_bound_min, ec.lower_bound_max, ec.upper_bound_min, ec.upper_bound_max)]

    class Env(OraclePositionEnv):
        """(the env bounds of a resetting env are re-drawn in front of its new state)"""
        new_bounds = None

        def reset_masked(self, mask, *draws):
            m = np.asarray(mask).astype(bool)
            self.bmin[m], self.bmax[m] = self.new_bounds[0][m], self.new_bounds[1][m]
            super().reset_masked(mask, *draws)

    o = Env(pd, n, L, gains, robot.min_init_state, robot.max_init_state, ranges)
    o.state[:], o.thrust[:], o.kT[:] = state, thrust, _npy(mm.motor_thrust_constant)
    o.tau_inc[:], o.tau_dec[:] = _npy(mm.motor_time_constants_increasing), _npy(mm.motor_time_constants_decreasing)
    o.bmin[:], o.bmax[:] = _npy(g["env_bounds_min"]), _npy(g["env_bounds_max"])
    o.sim_steps[:] = steps
    o.euler, o.qveh, o.vveh, o.vbody, o.wbody = orc.update_states(o.state)
    episodes = _npy(g["episode_count"]).astype(np.int32)
    agen = torch.Generator(device=DEV).manual_seed(11)
    seen = dict(crash=0, crash_after_first_step=0, trunc=0, mixed_wave=0)
    for t in range(T):
        a = (torch.rand(n, 4, device=DEV, generator=agen) * 2 - 1) * (3.0 if t % 4 == 3 else 1.0)
        ub = orc.rng_fill(seed, episodes, orc.RNG_BOUNDS, 6)
        o.new_bounds = ((bcfg[1] - bcfg[0]) * ub[:, :3] + bcfg[0], (bcfg[3] - bcfg[2]) * ub[:, 3:] + bcfg[2])
        mot = orc.rng_fill(seed, episodes, orc.RNG_MOTOR, 4 * M).reshape(n, M, 4)
        draws = (orc.rng_fill(seed, episodes, orc.RNG_STATE, 13), np.ascontiguousarray(mot[..., 0]), np.ascontiguousarray(mot[..., 1]),
                 np.ascontiguousarray(mot[..., 2]), np.ascontiguousarray(mot[..., 3]))
        results = [task.step(a) for task in tasks]
        torch.cuda.synchronize()
        _assert_same(plain, fused, t)
        o_obs, o_rew, o_crash, o_trunc, o_mask, _ = o.step(_npy(a), draws)
        episodes = episodes + o_mask.astype(np.int32)
        for task, (obs, rew, term, trunc_, _info) in zip(tasks, results):
            tg = task.sim_env.global_tensor_dict
            tm = task.sim_env.robot_manager.robot.control_allocator.motor_model
            for name, got, ref in (("state", tg["robot_state_tensor"], o.state), ("thrust", tm.current_motor_thrust, o.thrust),
                                   ("reward", rew, o_rew), ("obs", obs["observations"], o_obs), ("kT", tm.motor_thrust_constant, o.kT),
                                   ("crashes", term, o_crash.astype(bool)), ("truncations", trunc_, o_trunc.astype(bool)),
                                   ("reset_mask", tg["reset_mask"], o_mask), ("episode_count", tg["episode_count"], episodes),
                                   ("sim_steps", tg["sim_steps"], o.sim_steps)):
                same = _bits(_npy(got)) == _bits(ref)
                assert same.all(), (t, "single launch" if task is fused else "two launches", name, "envs", np.unique(np.argwhere(~same)[:, 0])[:8].tolist())
        pad = (-n) % 16
        wave = lambda x: np.pad(x.astype(bool), (0, pad)).reshape(-1, 16)  # noqa: E731
        cr, tr = wave(o_crash), wave(o_trunc)
        seen["crash"] += int(o_crash.sum())
        seen["crash_after_first_step"] += int(o_crash.sum()) if t > 0 else 0
        seen["trunc"] += int(o_trunc.sum())
        seen["mixed_wave"] += int((cr.any(1) & tr.any(1) & ~(cr | tr).all(1)).sum())
    assert seen["crash"] >= 8 and seen["crash_after_first_step"] >= 3 and seen["trunc"] >= n // 6 and seen["mixed_wave"] >= 1, seen
    stats = fused.single_launch_stats()
    assert stats["violations"] == 0
    assert stats["modes"]["any"] >= 1 and stats["modes"]["none"] >= 1, stats
    m = plain.single_launch_stats()["modes"]
    assert m["any"] == m["none"] == 0
