"""GPU: the position step under every shape of arguments its load block branches on, three ways.

The step wave and the helper wave of the position-step kernels fetch their kernel arguments as one batch and issue their input
loads as one batch (csrc/agx_dyn_state.h: arg_pin; agx_dyn_position_step.h: position_step_quad, position_step_helper).  What the
batch holds depends on which optional buffers exist: per-env controller gains or the uniform ones, per-motor time constants or
the uniform ones, the thrust constant with use_rps, the body-force and wrench outputs, and whether a crash resets an env.  For
each shape, a single-launch task (ANY / NONE launches), its two-launch twin and the CPU oracle's env loop run 60 steps on the
same actions; after EVERY step every buffer of the two tasks is compared bit for bit, and the single-launch task against the
oracle.  Truncations and crashes occur in every run (asserted), the latter next to the former in the same launches.

Shapes also covered elsewhere, two ways (single launch against two launches) and at greater length:
  default (uniform gains and time constants, use_rps, no outputs, crashes reset)   test_gpu_single_launch_step.py,
                                                                                  test_gpu_fused_step_helper_wave.py
  per-env gains + per-motor time constants, re-drawn at every reset               test_gpu_fused_step_helper_wave.py::
                                                                                  test_randomised_gains_and_motor_constants
and against the oracle, default shape: test_gpu_full_size_parity.py::test_config1_every_env_of_8192_for_50_steps.  They are part
of the matrix below all the same: here all three meet on every step."""
import numpy as np
import pytest
import torch

from aerial_gym_simulator_amd import _lib
from task_test_util import npy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS, L = 60, 14
SEED = 0x5EED0123456789
ANY = _lib.STEP_MODES.index("any")
TAU_NAMES = ("motor_time_constant_increasing_min", "motor_time_constant_increasing_max", "motor_time_constant_decreasing_min",
             "motor_time_constant_decreasing_max")

#            gains   tau     use_rps  outputs  reset_on_collision
SHAPES = {
    "default": (False, False, True, False, True),
    "per_env_gains_tau_outputs": (True, True, True, True, True),
    "no_rps_tau_crashes_stay": (False, True, False, False, False),
    "no_rps_gains_outputs_crashes_stay": (True, False, False, True, False),
    "gains_only": (True, False, True, False, True),
    "tau_outputs_crashes_stay": (False, True, True, True, False),
}


def _cfgs():
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config.controller_config import lee_controller_config as ctrl
    from aerial_gym_simulator_amd.config.robot_config import BaseQuadCfg
    from aerial_gym_simulator_amd.config.task_config import position_setpoint_task_config as cfg

    return cfg, ctrl, BaseQuadCfg.control_allocator_config.motor_model_config


@pytest.fixture(autouse=True)
def _restore():
    """the config classes this file changes"""
    cfg, ctrl, mm = _cfgs()
    old = (cfg.device, cfg.controller_name, cfg.episode_len_steps, cfg.args, ctrl.randomize_params, mm.use_rps,
           [getattr(mm, k) for k in TAU_NAMES])
    yield
    for env_cfg, roc in reversed(_ROC_TOUCHED):  # (the first entry of a class holds the value from before the test)
        env_cfg.reset_on_collision = roc
    del _ROC_TOUCHED[:]
    cfg.device, cfg.controller_name, cfg.episode_len_steps, cfg.args, ctrl.randomize_params, mm.use_rps = old[:6]
    for k, v in zip(TAU_NAMES, old[6]):
        setattr(mm, k, v)
    _lib.set_option("single_launch_step", 1)


_ROC_TOUCHED = []  # (env config class, its reset_on_collision before a test changed it)


class _Task:
    """one task of a shape; the optional outputs and the crash switch are set on the structs its step plan points at"""

    def __init__(self, n, single, shape):
        from aerial_gym_simulator_amd.registry.task_registry import task_registry

        gains, tau, rps, outputs, roc = shape
        cfg, ctrl, mm = _cfgs()
        cfg.device, cfg.controller_name, cfg.episode_len_steps = DEV, "lee_position_control", L
        cfg.args = {"strict_rng": False, "rng_seed": SEED, "single_launch_step": single}
        ctrl.randomize_params = bool(gains)
        mm.use_rps = bool(rps)
        if tau:
            mm.motor_time_constant_increasing_min, mm.motor_time_constant_increasing_max = 0.01, 0.03
            mm.motor_time_constant_decreasing_min, mm.motor_time_constant_decreasing_max = 0.02, 0.05
        self.task = task = task_registry.make_task("position_setpoint_task", seed=5, num_envs=n, headless=True)
        env = self.env = task.sim_env
        B = env._buffers
        assert bool(B.gains) == bool(gains) and bool(B.motor_tau_inc) == bool(tau) and bool(B.motor_tau_dec) == bool(tau)
        assert bool(env._params.use_rps) == bool(rps)
        assert task._plan is not None and (task._proof_watch is not None) == bool(single)
        self.body_force = self.wrench = None
        if outputs:
            self.body_force, self.wrench = torch.zeros(3, n, device=DEV), torch.zeros(6, n, device=DEV)
            B.body_force, B.wrench_cmd = _lib.dptr(self.body_force), _lib.dptr(self.wrench)
        _ROC_TOUCHED.append((env.cfg.env, env.cfg.env.reset_on_collision))
        env.cfg.env.reset_on_collision = bool(roc)
        task._plan_task.reset_on_collision = int(roc)

    def tensors(self):
        task, env = self.task, self.env
        g = env.global_tensor_dict
        mm = env.robot_manager.robot.control_allocator.motor_model
        out = {"obs": task.task_obs["observations"], "reward": task.rewards, "crashes": g["crashes"], "truncations": g["truncations"],
               "state": g["robot_state_soa"], "derived": g["robot_derived_soa"], "thrust": mm.thrust_soa, "tau_inc": mm.tau_inc_soa,
               "tau_dec": mm.tau_dec_soa, "kT": mm.kT_soa, "gains": g["controller_gains_soa"], "actions": g["robot_actions_soa"],
               "prev_actions": g["robot_prev_actions_soa"], "sim_steps": g["sim_steps"], "episode_count": g["episode_count"],
               "bounds_min": env.bounds_soa[0], "bounds_max": env.bounds_soa[1], "reset_mask": g["reset_mask"],
               "reset_flag": g["reset_flag"]}
        if self.body_force is not None:
            out["body_force"], out["wrench_cmd"] = self.body_force, self.wrench
        return out


def _assert_same(a, b, t):
    ta, tb = a.tensors(), b.tensors()
    for k in ta:
        assert torch.equal(ta[k], tb[k]), (t, k)


class _Oracle:
    """EnvManager.step + PositionSetpointTask.step from the CPU oracle's functions (tests/oracle_env.py), with what the shapes
    add: gains re-drawn at a reset, crashes that do not reset"""

    def __init__(self, orc, T, shape):
        from oracle_env import OraclePositionEnv

        self.orc, self.shape = orc, shape
        gains, tau, rps, outputs, roc = shape
        task, env = T.task, T.env
        g = env.global_tensor_dict
        robot = env.robot_manager.robot
        mm, ctrl = robot.control_allocator.motor_model, robot.controller
        pd = dict(robot.params_dict)
        assert bool(pd["use_rps"]) == bool(rps)
        n = self.n = env.num_envs
        self.M = pd["num_motors"]
        self.gmin, self.gmax = np.array(ctrl.gains_min, np.float32), np.array(ctrl.gains_max, np.float32)
        if gains:
            k = npy(g["controller_gains_soa"]).T  # [N, 12]
        else:
            k = np.tile(((self.gmax + self.gmin) / np.float32(2)), (n, 1))
        ranges = dict(mm.ranges)
        ranges.setdefault("thrust", (float(pd["min_thrust"]), float(pd["max_thrust"])))
        o = self.o = OraclePositionEnv(pd, n, L, [k[:, 3 * j:3 * j + 3] for j in range(4)], robot.min_init_state, robot.max_init_state, ranges)
        o.state[:], o.thrust[:], o.kT[:] = npy(g["robot_state_tensor"]), npy(mm.current_motor_thrust), npy(mm.motor_thrust_constant)
        o.tau_inc[:], o.tau_dec[:] = npy(mm.motor_time_constants_increasing), npy(mm.motor_time_constants_decreasing)
        o.bmin[:], o.bmax[:] = npy(g["env_bounds_min"]), npy(g["env_bounds_max"])
        o.sim_steps[:] = npy(g["sim_steps"])
        o.target[:] = npy(task.target_position)
        o.euler, o.qveh, o.vveh, o.vbody, o.wbody = orc.update_states(o.state)
        self.episodes = npy(g["episode_count"]).astype(np.int32)
        e = env.cfg.env
        self.bcfg = [np.array(x, np.float32) for x in (e.lower_bound_min, e.lower_bound_max, e.upper_bound_min, e.upper_bound_max)]

    def step(self, action):
        orc, o, n, M = self.orc, self.o, self.n, self.M
        gains, tau, rps, outputs, roc = self.shape
        crashes = np.zeros(n, np.uint8)
        s = orc.substep(o.P, o.state, action, o.thrust, o.kT, o.tau_inc, o.tau_dec, o.Kp, o.Kv, o.KR, o.Kw)
        o.euler, o.qveh, o.vveh, o.vbody, o.wbody = s.euler, s.qveh, s.vveh, s.vbody, s.wbody
        o.sim_steps += 1
        reward = orc.reward_position(o.state, o.qveh, o.wbody, o.target, crashes)
        trunc = (o.sim_steps > L).astype(np.uint8)
        mask = (((crashes > 0) & bool(roc)) | (trunc > 0)).astype(np.uint8)
        if mask.any():
            m = mask.astype(bool)
            ep, bcfg = self.episodes, self.bcfg
            ub = orc.rng_fill(SEED, ep, orc.RNG_BOUNDS, 6)
            o.bmin[m] = ((bcfg[1] - bcfg[0]) * ub[:, :3] + bcfg[0])[m]
            o.bmax[m] = ((bcfg[3] - bcfg[2]) * ub[:, 3:] + bcfg[2])[m]
            if gains:
                ug = orc.rng_fill(SEED, ep, orc.RNG_GAINS, 12)
                k = ((self.gmax - self.gmin) * ug + self.gmin).astype(np.float32)
                for j, K in enumerate((o.Kp, o.Kv, o.KR, o.Kw)):
                    K[m] = k[:, 3 * j:3 * j + 3][m]
            mot = orc.rng_fill(SEED, ep, orc.RNG_MOTOR, 4 * M).reshape(n, M, 4)
            o.reset_masked(mask, orc.rng_fill(SEED, ep, orc.RNG_STATE, 13), *(np.ascontiguousarray(mot[..., c]) for c in range(4)))
            self.episodes = ep + mask.astype(np.int32)
        obs = orc.obs_position(o.state, o.vbody, o.wbody, o.target)
        return obs, reward, crashes, trunc, mask

    def place(self, idx, offset, linvel=None):
        self.o.state[idx, 0:3] = self.o.target[idx] + np.asarray(offset, np.float32)
        if linvel is not None:
            self.o.state[idx, 7:10] = np.asarray(linvel, np.float32)


def _assert_oracle(T, O, out, t):
    gains, tau, rps, outputs, roc = O.shape
    task, env, o = T.task, T.env, O.o
    g = env.global_tensor_dict
    mm = env.robot_manager.robot.control_allocator.motor_model
    o_obs, o_rew, o_crash, o_trunc, o_mask = out
    pairs = [("state", g["robot_state_tensor"], o.state), ("thrust", mm.current_motor_thrust, o.thrust), ("reward", task.rewards, o_rew),
             ("obs", task.task_obs["observations"], o_obs), ("kT", mm.motor_thrust_constant, o.kT),
             ("episode_count", g["episode_count"], O.episodes), ("sim_steps", g["sim_steps"], o.sim_steps),
             ("crashes", g["crashes"], o_crash), ("truncations", g["truncations"], o_trunc), ("reset_mask", g["reset_mask"], o_mask),
             ("bounds_min", g["env_bounds_min"], o.bmin), ("bounds_max", g["env_bounds_max"], o.bmax)]
    if tau:
        pairs += [("tau_inc", mm.motor_time_constants_increasing, o.tau_inc), ("tau_dec", mm.motor_time_constants_decreasing, o.tau_dec)]
    if gains:
        pairs += [("gains", g["controller_gains_soa"].T, np.concatenate([o.Kp, o.Kv, o.KR, o.Kw], axis=1))]
    for name, got, ref in pairs:
        got = npy(got).reshape(ref.shape)
        ref = ref.astype(got.dtype) if ref.dtype != got.dtype else ref
        if not np.array_equal(got, ref):
            bad = np.argwhere(got != ref)
            raise AssertionError(f"step {t}: {name} differs from the oracle in {len(bad)} of {got.size} entries, first {bad[0]}: "
                                 f"{got[tuple(bad[0])]!r} vs {ref[tuple(bad[0])]!r}")


@pytest.mark.parametrize("n", [333, 8192])
@pytest.mark.parametrize("name", list(SHAPES))
def test_three_ways_agree_on_every_buffer_after_every_step(orc, name, n):
    shape = SHAPES[name]
    roc = shape[4]
    plain, fused = _Task(n, False, shape), _Task(n, True, shape)
    for T in (plain, fused):
        T.task.reset()
        T.env.sim_steps.copy_(torch.randint(0, L, (n,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(9),
                                            dtype=torch.int32))
    torch.cuda.synchronize()
    _assert_same(plain, fused, -1)
    O = _Oracle(orc, fused, shape)
    gen = torch.Generator(device=DEV).manual_seed(7)
    far = torch.arange(3, n, 16, device=DEV)   # one env in every wave: beyond the crash radius when the step starts
    near = torch.arange(9, n, 16, device=DEV)  # another one: just inside it, flying outward -- crosses it within an ANY launch
    seen = {"truncations": 0, "crashes": 0, "resets": 0, "any_launches": 0, "any_with_crash": 0}
    for t in range(STEPS):
        if t % 14 == 5:
            for T in (plain, fused):
                g = T.env.global_tensor_dict
                g["robot_position"][near] = T.task.target_position[near] + torch.tensor([7.9, 0.0, 0.0], device=DEV)
                g["robot_linvel"][near] = torch.tensor([4.0, 0.0, 0.0], device=DEV)
            O.place(npy(near), [7.9, 0.0, 0.0], [4.0, 0.0, 0.0])
        elif t % 14 == 12:
            for T in (plain, fused):
                g = T.env.global_tensor_dict
                g["robot_position"][far] = T.task.target_position[far] + torch.tensor([0.0, 9.0, 0.0], device=DEV)
            O.place(npy(far), [0.0, 9.0, 0.0])
        a = (torch.rand(n, 4, device=DEV, generator=gen) * 2 - 1) * 3.0
        for T in (plain, fused):
            T.task.step(a)
        torch.cuda.synchronize()
        out = O.step(npy(a))
        _assert_same(plain, fused, t)
        _assert_oracle(fused, O, out, t)
        g = fused.env.global_tensor_dict
        crashed, truncated = int(g["crashes"].sum()), int(g["truncations"].sum())
        seen["truncations"] += truncated
        seen["crashes"] += crashed
        seen["resets"] += int(out[4].sum())
        if int(fused.task._plan.last_mode) == ANY:
            seen["any_launches"] += 1
            seen["any_with_crash"] += int(crashed > 0)
    print(f"\n{name} n={n}: {seen}")
    # 60 steps of episodes of 14, desynchronised: about n / 15 envs truncate in every step
    # (an env truncates every 15 steps unless a crash reset it in between: two of sixteen are made to crash)
    assert seen["truncations"] >= 2 * n, seen
    assert seen["crashes"] >= 1 and seen["any_with_crash"] >= 1, seen
    assert seen["any_launches"] >= STEPS // 2, seen
    if not roc:  # a crashed env stays where it is until it truncates: more crash flags than resets they caused
        assert seen["resets"] == seen["truncations"], seen
    assert fused.task.single_launch_stats()["violations"] == 0
    m = plain.task.single_launch_stats()["modes"]
    assert m["any"] == m["none"] == 0
