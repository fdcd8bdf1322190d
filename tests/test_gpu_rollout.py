"""GPU: EnvManager.rollout -- T env steps in one launch (agx_env_rollout, k_env_step_rollout) -- against the eager loop
`for t in range(T): env.step(actions_t)`, which the rest of the suite pins to the CPU restatement of the reference.

Each case: build one env, reset(), snapshot(), run T eager steps (cloning the recorded keys and the crash flags after each), restore()
the snapshot, run rollout() with the same actions, and compare BITS: every tensor of the dict and the motor thrusts, every recorded
step, first_crash_step, the host's counters and python's `random` state; then three more eager steps from both end states.
(snapshot() refuses none of the configurations below, so no case needs the two-envs-of-one-seed fallback.)"""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL_KEYS = ("robot_position", "robot_orientation", "robot_linvel", "robot_angvel", "robot_body_angvel",
            "robot_euler_angles", "robot_vehicle_orientation", "motor_thrusts", "crashes", "robot_body_linvel", "robot_vehicle_linvel")
REST_KEYS = ("robot_vehicle_linvel", "robot_body_linvel", "crashes")  # what ALL_KEYS drops to fit 32 channels, in a record of its own


def build(robot, controller, n, env_name="empty_env", sim="base_sim", args=None, seed=7):
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.sim.sim_builder import SimBuilder

    a = {"rng_seed": seed}
    a.update(args or {})
    return SimBuilder().build_env(sim_name=sim, env_name=env_name, robot_name=robot, controller_name=controller, device=DEV, args=a,
                                  num_envs=n, headless=True, use_warp=False)


def keys_for(env, keys=ALL_KEYS):
    """the keys that fit the channel table of this robot (an eight-motor robot drops the last ones)"""
    M = int(env.robot_manager.robot.cfg.control_allocator_config.num_motors)
    keys = list(keys)
    width = lambda k: M if k == "motor_thrusts" else {"robot_orientation": 4, "robot_vehicle_orientation": 4, "crashes": 1}.get(k, 3)  # noqa: E731
    while sum(width(k) for k in keys) > 32:
        keys.pop()
    return tuple(keys)


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def tensors(env):
    g = env.global_tensor_dict
    out = {k: dict.get(g, k) for k in g if isinstance(dict.get(g, k), torch.Tensor)}
    mm = env.robot_manager.robot.control_allocator.motor_model
    out["motor_thrusts"] = mm.current_motor_thrust
    return out


def clone(env):
    return {k: v.clone() for k, v in tensors(env).items()}


def host(env):
    B = env._buffers
    return dict(step_counter=env.step_counter, parity=env._parity, produced=tuple(sorted(env._produced)), b_step=int(B.step_counter),
                disturb_prob=float(B.disturb_prob), disturb=B.disturb, random=random.getstate())


def look(env, key):
    if key == "motor_thrusts":
        return env.robot_manager.robot.control_allocator.motor_model.current_motor_thrust.clone()
    v = env.global_tensor_dict[key]
    return v.to(torch.float32).unsqueeze(1) if key == "crashes" else v.clone()


def make_actions(env, T, scale, held, seed=3, offset=0.0):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    shape = (env.num_envs, env.num_robot_actions) if held else (T, env.num_envs, env.num_robot_actions)
    return (torch.rand(shape, device=DEV, generator=gen) * 2 - 1) * scale + offset


def run_both(env, actions, T, record, before_compare=None, script=None):
    """the comparison of the module docstring; returns (eager per-step values, the record)"""
    held = actions.dim() == 2
    if script is not None:  # num_physics_steps patched on the env, the same script on both paths and for the three steps behind
        def patch():
            it = iter(list(script) + [1, 2, 1])
            env.num_physics_steps = lambda: next(it)
    else:
        def patch():
            pass
    tail = make_actions(env, 3, 0.5, False, seed=11, offset=float(actions.mean()))
    env.reset()
    snap = env.snapshot()
    patch()
    calls0 = env._calls
    eager = {k: [] for k in record}
    flags = []
    for t in range(T):
        env.step(actions if held else actions[t])
        for k in record:
            eager[k].append(look(env, k))
        flags.append(env.global_tensor_dict["crashes"].clone())
    end_eager, host_eager, calls_eager = clone(env), host(env), env._calls - calls0
    for t in range(3):
        env.step(tail[t])
    tail_eager, tail_host = clone(env), host(env)
    flags = torch.stack(flags)  # [T, N]
    if before_compare is not None:
        before_compare(flags)
    assert bool(torch.isfinite(end_eager["robot_state_tensor"]).all()), "the eager run left the numbers"

    env.restore(snap)
    patch()
    calls1 = env._calls
    rec = env.rollout(actions, steps=T if held else None, record=record)
    assert env._calls - calls1 == calls_eager == T
    end_roll, host_roll = clone(env), host(env)
    assert host_roll == host_eager, {k: (host_roll[k], host_eager[k]) for k in host_roll if host_roll[k] != host_eager[k] and k != "random"}
    assert set(end_roll) == set(end_eager)
    for k in end_eager:
        assert same(end_roll[k], end_eager[k]), k
    for k in record:
        assert rec[k].shape == (T, env.num_envs, eager[k][0].shape[1]) and rec[k].dtype == torch.float32
        for t in range(T):
            assert same(rec[k][t], eager[k][t]), (k, t)
    step_of = torch.arange(T, device=DEV, dtype=torch.int32).unsqueeze(1).expand(T, env.num_envs)
    first = torch.where(flags, step_of, torch.full_like(step_of, T)).min(dim=0).values
    first = torch.where(first == T, torch.full_like(first, -1), first)
    assert rec.first_crash_step.dtype == torch.int32 and torch.equal(rec.first_crash_step, first)
    for t in range(3):  # no state was missed: the steps behind the rollout are the steps behind the loop
        env.step(tail[t])
    tail_roll = clone(env)
    for k in tail_eager:
        assert same(tail_roll[k], tail_eager[k]), ("three steps later", k)
    assert host(env) == tail_host
    if script is not None:
        del env.num_physics_steps
    return eager, rec


# ---- batch sizes x step counts: base_quadrotor, lee_position_control (the eager loop runs the lane-quad kernels there) ----
@pytest.mark.parametrize("n,T,held", [(5, 1, False), (5, 2, True), (70, 37, False), (70, 37, True), (300, 2, False), (300, 37, False)])
def test_position_control_matches_the_eager_loop(n, T, held):
    env = build("base_quadrotor", "lee_position_control", n)
    actions = make_actions(env, T, 1.0, held)
    if not held and T > 1:
        assert not torch.equal(actions[0], actions[1])  # a schedule whose rows differ
    run_both(env, actions, T, keys_for(env))


def test_one_step_equals_one_step_and_the_rest_keys_record():
    """T = 1 on 70 envs, with the keys the other cases' 32-channel records leave out"""
    env = build("base_quadrotor", "lee_position_control", 70)
    run_both(env, make_actions(env, 1, 1.0, False), 1, REST_KEYS)
    run_both(env, make_actions(env, 4, 1.0, True), 4, ())  # nothing recorded: first_crash_step alone


def test_256_thread_instances_above_65536_envs():
    env = build("base_quadrotor", "lee_position_control", 65600)
    run_both(env, make_actions(env, 2, 1.0, False), 2, ("robot_position", "robot_euler_angles", "motor_thrusts"))


# ---- robots and laws ----
@pytest.mark.parametrize("robot,controller,scale,offset", [
    ("base_quadrotor", "lee_velocity_control", 1.0, 0.0),
    ("base_quadrotor", "lee_attitude_control", 0.3, 0.0),
    ("base_quadrotor", "lee_acceleration_control", 1.0, 0.0),
    ("base_quadrotor", "lee_rates_control", 0.3, 0.0),
    ("base_quadrotor", "no_control", 0.5, 1.0),
    ("base_quad_root_link_control", "lee_position_control", 1.0, 0.0),
])
def test_laws_match_the_eager_loop(robot, controller, scale, offset):
    env = build(robot, controller, 70)
    run_both(env, make_actions(env, 37, scale, False, offset=offset), 37, keys_for(env))


def test_octarotor_fully_actuated_with_the_device_generator_disturbance(orc):
    env = build("base_octarotor", "fully_actuated_control", 70)
    dcfg = env.robot_manager.robot.cfg.disturbance
    assert dcfg.enable_disturbance and not env.strict_rng and env.num_robot_actions == 7
    T = 37

    def some_env_is_disturbed(flags):
        # the draws the T eager steps made (device stream RNG_DISTURB + sub-step, one sub-step per step in empty_env), restated on the CPU
        start, hit = env.step_counter - (T + 3), 0
        for t in range(T):
            u = orc.rng_fill(env.rng_seed, np.full(env.num_envs, start + t, np.int32), (1 << 20) + 0, 7)
            hit += int(((u[:, 0] < np.float32(dcfg.prob_apply_disturbance)) & (u[:, 1:] != np.float32(0.5)).any(axis=1)).sum())
        print(f"octarotor: {hit} non-zero disturbance draws in {T} steps of {env.num_envs} envs")
        assert hit > 0, "no env draws a disturbance in this run: the case shows nothing"

    run_both(env, make_actions(env, T, 1.0, False), T, keys_for(env), before_compare=some_env_is_disturbed)
    assert np.float32(env._buffers.disturb_prob) == np.float32(dcfg.prob_apply_disturbance)


# ---- obstacles: the crash flag of every step, 10 sub-steps per step ----
OBSTACLE_SEED = 7


def test_obstacles_crash_flags_and_first_crash_step():
    env = build("base_quadrotor", "lee_velocity_control", 70, env_name="env_with_obstacles", seed=OBSTACLE_SEED)
    assert env.cfg.env.num_physics_steps_per_env_step_mean == 10 and env.scene.num_assets > 0
    T = 12

    def some_crash_some_never(flags):
        crashed = flags.any(dim=0)
        print(f"obstacles: {int(crashed.sum())} of {flags.shape[1]} envs crash within {T} steps")
        assert bool(crashed.any()) and not bool(crashed.all())

    eager, rec = run_both(env, make_actions(env, T, 4.0, False), T, ("robot_position", "robot_linvel", "crashes", "motor_thrusts"),
                          before_compare=some_crash_some_never)
    assert bool((rec.first_crash_step >= 0).any()) and bool((rec.first_crash_step < 0).any())


# ---- sub-step counts: a zero count, the per-step array ----
@pytest.mark.parametrize("env_name,controller", [("empty_env", "lee_position_control"), ("env_with_obstacles", "lee_velocity_control")])
def test_scripted_substep_counts(env_name, controller):
    env = build("base_quadrotor", controller, 70, env_name=env_name, seed=OBSTACLE_SEED)
    script = [1, 0, 2, 1, 3]
    eager, rec = run_both(env, make_actions(env, 5, 2.0, False), 5, keys_for(env), script=script)
    assert rec.substeps is not None and rec.substeps.tolist() == script
    # the step of zero sub-steps changed nothing but the counters: its record repeats the step before, its crash flag is clear
    assert same(rec["robot_position"][1], rec["robot_position"][0]) and same(rec["robot_euler_angles"][1], rec["robot_euler_angles"][0])
    assert not bool(rec["crashes"][1].any())


def test_python_random_stream_is_consumed_like_the_loop():
    """a sub-step count with a spread: the T counts are drawn up front through num_physics_steps, in order"""
    env = build("base_quadrotor", "lee_position_control", 70)
    env.cfg.env.num_physics_steps_per_env_step_mean, env.cfg.env.num_physics_steps_per_env_step_std = 2, 1.5
    try:
        random.seed(5)
        eager, rec = run_both(env, make_actions(env, 9, 1.0, False), 9, ("robot_position",))
        assert rec.substeps is not None and len(set(rec.substeps.tolist())) > 1
    finally:
        env.cfg.env.num_physics_steps_per_env_step_mean, env.cfg.env.num_physics_steps_per_env_step_std = 1, 0


# ---- record reuse ----
def test_out_reuses_the_record_and_a_mismatched_one_raises():
    env = build("base_quadrotor", "lee_position_control", 70)
    env.reset()
    a = make_actions(env, 6, 1.0, False)
    rec = env.rollout(a, record=("robot_position", "crashes"))
    first = rec["robot_position"].clone()
    ptrs = (rec.data.data_ptr(), rec.first_crash_step.data_ptr(), rec["robot_position"].data_ptr())
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    rec2 = env.rollout(a, record=("robot_position", "crashes"), out=rec)
    torch.cuda.synchronize()
    assert rec2 is rec and ptrs == (rec.data.data_ptr(), rec.first_crash_step.data_ptr(), rec["robot_position"].data_ptr())
    assert torch.cuda.memory_allocated() == allocated
    assert not torch.equal(rec["robot_position"], first)  # the second six steps, over the first
    before = clone(env)
    for actions, keys in ((a, ("robot_position",)), (a, ("crashes", "robot_position")), (a[:5], ("robot_position", "crashes"))):
        with pytest.raises(ValueError, match=r"rollout\(out=\)"):
            env.rollout(actions, record=keys, out=rec)
    for k, v in before.items():
        assert same(tensors(env)[k], v), k


# ---- refusals: each raises its message before anything is written ----
class _ZeroWrenchController:
    """a user controller class (no KIND attribute): the framework treats it as external code"""

    def __init__(self, config, num_envs, device, mode="robot"):
        self.cfg, self.num_envs, self.device = config, num_envs, device

    def init_tensors(self, g):
        pass

    def reset_idx(self, env_ids):
        pass

    def randomize_params(self, env_ids):
        pass

    def __call__(self, action):
        return torch.zeros(self.num_envs, 6, device=action.device)


def _user_controller_env():
    from aerial_gym_simulator_amd.config.controller_config import lee_controller_config
    from aerial_gym_simulator_amd.registry.controller_registry import controller_registry

    controller_registry.register_controller("rollout_test_user_control", _ZeroWrenchController, lee_controller_config)
    return build("base_quadrotor", "rollout_test_user_control", 8)


def _user_robot_env():
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.registry.robot_registry import robot_registry
    from aerial_gym_simulator_amd.robots.base_multirotor import BaseMultirotor

    class ToyRobot(BaseMultirotor):
        def step(self, action_tensor):
            super().step(action_tensor)

    robot_registry.register("rollout_test_toy_robot", ToyRobot, robot_registry.get_robot_config("base_quadrotor"))
    return build("rollout_test_toy_robot", "lee_position_control", 8)


def _task_env():
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config.task_config import position_setpoint_task_config as cfg
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    cfg.device, cfg.controller_name = DEV, "lee_position_control"
    task = task_registry.make_task("position_setpoint_task", seed=1, num_envs=8, headless=True)
    task.reset()
    env = task.sim_env
    env._keep_task = task
    return env


def _env_actions_env():
    env = build("base_quadrotor", "lee_position_control", 8)
    # what the first step(actions, env_actions=...) leaves in the dict: the obstacle twist buffer
    env.global_tensor_dict["env_actions"] = torch.zeros(8, 1, 6, device=DEV)
    return env


def _step_graph_env():
    env = build("base_quadrotor", "lee_position_control", 8)
    env.step_graph_mode = True  # what a task with args={'step_graph': True} sets on its env
    return env


def _exchange_rows_env():
    env = build("base_quadrotor", "lee_position_control", 8)
    env.bind_step_rows(torch.zeros(2, 8, 16, device=DEV), torch.zeros(8, device=DEV))
    return env


@pytest.mark.parametrize("make,message", [
    (_task_env, "task-owned env"),
    (_user_controller_env, "user-registered controller or robot class"),
    (_user_robot_env, "user-registered controller or robot class"),
    (_env_actions_env, r"env_actions \(moving obstacles\)"),
    (lambda: build("base_octarotor", "fully_actuated_control", 8, args={"strict_rng": True}), "strict_rng and the disturbance enabled"),
    (lambda: build("base_quadrotor_with_imu", "lee_position_control", 8), "with an IMU"),
    (lambda: build("base_quadrotor", "lee_position_control", 8, args={"lean_step": True}), "lean_step"),
    (_step_graph_env, "hipGraph replay"),
    (_exchange_rows_env, "exchange rows"),
    (lambda: build("base_rov", "fully_actuated_control", 8, sim="base_sim_no_gravity"), "rollout of an ROV"),
    (lambda: build("base_random", "lee_position_control", 8), "centre of mass is off the base link"),
], ids=["task", "user_controller", "user_robot", "env_actions", "strict_rng_disturbance", "imu", "lean_step", "step_graph", "exchange_rows",
        "rov", "com_offset"])
def test_refusals_name_the_reason_and_write_nothing(make, message):
    env = make()
    if getattr(env, "_keep_task", None) is None:
        env.reset()
    before, state = clone(env), random.getstate()
    h = host(env)
    a = torch.zeros(env.num_envs, env.num_robot_actions, device=DEV)
    with pytest.raises(RuntimeError, match=message):
        env.rollout(a, steps=3, record=("robot_position",))
    torch.cuda.synchronize()
    for k, v in before.items():
        assert same(tensors(env)[k], v), k
    assert random.getstate() == state and host(env) == h


# ---- the step-response example on top of it ----
def test_sys_id_example_reads_time_constants_from_the_record():
    """examples/sys_id.py, called in process: one rollout per action axis, the time constant one reduction over the record"""
    import importlib.util
    import os

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "sys_id.py")
    spec = importlib.util.spec_from_file_location("agx_example_sys_id", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.identify("velocity", 4)
    assert out["steps"] == 500 and out["controller"] == "lmf2_velocity_control" and [r["axis"] for r in out["axes"]] == ["X", "Y", "Z", "Yaw Rate"]
    for r in out["axes"]:  # every axis answers its unit step within the 2.5 s that follow it, and nobody crashes in an empty env
        assert r["envs_reached"] == 4 and 0.0 < r["time_constant_median"] < 2.5 and r["crashed_envs"] == 0, r
