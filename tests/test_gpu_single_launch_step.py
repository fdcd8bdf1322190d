"""GPU: single-launch position steps (include/aerial_gym_hip.h AgxPositionStepPlan.proof_*, csrc/agx_dyn_position_step.h
k_position_step_fused) against the two launches they replace.

A task with args={"single_launch_step": False} always issues the two launches; its twin, same seed, issues a step as ONE launch
whenever the host record proves the batch-wide reset OR (ANY: some env certainly truncates in it; NONE: no env can reset).  Both
are stepped with the same actions and compared bit for bit at every step: observation, reward, flags, state, derived tensors,
motor thrust, sim_steps, episode count, env bounds, reset mask.  The device's violation word (a NONE launch that saw a reset, an
ANY launch without one) stays 0."""
import pytest
import torch

from aerial_gym_simulator_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _restore():
    """the library option and the task config class this file changes (the tasks read episode_len_steps from it every step)"""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config.task_config import position_setpoint_task_config as cfg

    old = (cfg.device, cfg.controller_name, cfg.episode_len_steps, cfg.args)
    yield
    cfg.device, cfg.controller_name, cfg.episode_len_steps, cfg.args = old
    _lib.set_option("single_launch_step", 1)


def _make(n, L, single, seed=5):
    from aerial_gym_simulator_amd.config.task_config import position_setpoint_task_config as cfg
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    cfg.device, cfg.controller_name, cfg.episode_len_steps = DEV, "lee_position_control", L
    cfg.args = {"rng_seed": 1234, "single_launch_step": single}
    return task_registry.make_task("position_setpoint_task", seed=seed, num_envs=n, headless=True)


def _tensors(task):
    env = task.sim_env
    g = env.global_tensor_dict
    return {"obs": task.task_obs["observations"], "reward": task.rewards, "crashes": g["crashes"], "truncations": g["truncations"],
            "state": g["robot_state_soa"], "derived": g["robot_derived_soa"],
            "thrust": env.robot_manager.robot.control_allocator.motor_model.thrust_soa, "sim_steps": g["sim_steps"],
            "episode_count": g["episode_count"], "bounds_min": env.bounds_soa[0], "bounds_max": env.bounds_soa[1],
            "reset_mask": g["reset_mask"]}


def _assert_same(a, b, t):
    ta, tb = _tensors(a), _tensors(b)
    for k in ta:
        assert torch.equal(ta[k], tb[k]), (t, k)


def _modes(task):
    return dict(zip(_lib.STEP_MODES, (int(x) for x in task._plan.mode_count)))


def _stagger(n):
    i = torch.arange(n, device=DEV)
    return ((i % 7) * 3 + (i >= n // 2).to(torch.int64) * 11).to(torch.int32)


@pytest.mark.parametrize("n", [8192, 333])
def test_single_launch_steps_equal_the_two_launch_steps(n):
    L = 37
    plain, fused = _make(n, L, False), _make(n, L, True)
    assert fused._proof_watch is not None and plain._proof_watch is None
    g = torch.Generator(device=DEV).manual_seed(2)

    def both(t, sync=True):
        a = torch.rand(n, 4, device=DEV, generator=g) * 2 - 1
        plain.step(a)
        fused.step(a)
        if sync:
            torch.cuda.synchronize()
            _assert_same(plain, fused, t)

    def run(steps, t0):
        before = _modes(fused)
        for t in range(t0, t0 + steps):
            both(t)
        after = _modes(fused)
        return {k: after[k] - before[k] for k in after}

    for task in (plain, fused):
        task.reset()
    _assert_same(plain, fused, -1)
    # synchronised episodes: L steps without a reset, then every env truncates together
    sync = run(2 * L, 0)
    assert sync["none"] >= L, sync
    # staggered episodes (written through the public tensor: the records before are void)
    for task in (plain, fused):
        task.sim_env.sim_steps.copy_(_stagger(n) % L)
    run(150, 2 * L)
    # desynchronised the way bench.py does it: sim_steps <- U{0 .. L - 1}, about n / L truncations in every step
    for task in (plain, fused):
        task.sim_env.sim_steps.copy_(torch.randint(0, L, (n,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(9),
                                                   dtype=torch.int32))
    desync = run(400, 2 * L + 150)
    assert desync["any"] >= 0.9 * 400, desync
    assert _modes(plain)["any"] == _modes(plain)["none"] == 0
    assert fused.single_launch_stats()["violations"] == 0


@pytest.mark.parametrize("n", [8192, 333])
def test_identity_survives_host_interference(n):
    """The host changes what the proof rests on behind the kernels' back; the records from before are void and every step stays
    bit-identical -- and when it stops, single launches resume."""
    L = 23
    plain, fused = _make(n, L, False), _make(n, L, True)
    for task in (plain, fused):
        task.reset()
        task.sim_env.sim_steps.copy_(_stagger(n) % L)
    g = torch.Generator(device=DEV).manual_seed(3)
    for t in range(160):
        a = torch.rand(n, 4, device=DEV, generator=g) * 2 - 1
        for task in (plain, fused):
            if t % 10 == 1:  # robots teleported to 7.995 m from their target: one step from the crash radius
                task.obs_dict["robot_position"][: n // 3] = task.target_position[: n // 3] + torch.tensor([7.995, 0.0, 0.0], device=DEV)
            elif t % 10 == 3:  # targets moved 9 m away: an immediate crash
                task.target_position[n // 2: n // 2 + 5, 0] += 9.0
            elif t % 10 == 5:  # step counters rewound / pushed to the brink of truncation
                task.sim_env.sim_steps[7::13] = L
                task.sim_env.sim_steps[3::11] = 0
            elif t % 10 == 7:
                task.reset_idx(torch.arange(0, n, 3, device=DEV))
            elif t % 10 == 9:
                task.sim_env.robot_manager.robot.control_allocator.motor_model.thrust_soa.mul_(0.5)
            elif t == 80:
                task.task_config.episode_len_steps = L + 4
        plain.step(a)
        fused.step(a)
        torch.cuda.synchronize()
        _assert_same(plain, fused, t)
    assert fused.single_launch_stats()["violations"] == 0
    before = _modes(fused)
    for t in range(160, 260):
        a = torch.rand(n, 4, device=DEV, generator=g) * 2 - 1
        plain.step(a)
        fused.step(a)
        torch.cuda.synchronize()
        _assert_same(plain, fused, t)
    after = _modes(fused)
    assert (after["any"] + after["none"]) - (before["any"] + before["none"]) >= 80, (before, after)
    assert fused.single_launch_stats()["violations"] == 0


def test_option_switch_keeps_two_launches():
    n, L = 1024, 29
    a_task, b_task = _make(n, L, False), _make(n, L, True)
    for task in (a_task, b_task):
        task.reset()
    _lib.set_option("single_launch_step", 0)
    act = torch.rand(n, 4, device=DEV) * 2 - 1
    for t in range(20):
        a_task.step(act)
        b_task.step(act)
        torch.cuda.synchronize()
        _assert_same(a_task, b_task, t)
    assert _modes(b_task)["two"] == 20 and b_task.single_launch_stats()["reasons"]["off"] == 20
    _lib.set_option("single_launch_step", 1)
    for t in range(20, 60):
        a_task.step(act)
        b_task.step(act)
        torch.cuda.synchronize()
        _assert_same(a_task, b_task, t)
    assert _modes(b_task)["none"] + _modes(b_task)["any"] >= 20


def test_free_running_2000_steps_end_identical():
    """bench.py's setting: 8192 envs, L = 500, episodes desynchronised through the public tensor, 2000 steps without any
    synchronisation (the host runs ahead of the device, at most max_lag steps ahead of the newest record): the end state equals
    the two-launch run's bit for bit, and >= 95 % of the steps ran as one launch."""
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("agx_bench", os.path.join(os.path.dirname(os.path.dirname(__file__)), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n, L = 8192, 500
    plain, fused = _make(n, L, False), _make(n, L, True)
    g = torch.Generator(device=DEV).manual_seed(1234)
    actions = [torch.rand(n, 4, device=DEV, generator=g) * 2 - 1 for _ in range(16)]
    for task in (plain, fused):
        task.reset()
        bench.desynchronise_episodes(task)
        for i in range(2000):
            task.step(actions[i % 16])
        torch.cuda.synchronize()
    _assert_same(plain, fused, 2000)
    m = _modes(fused)
    assert m["any"] + m["none"] >= 0.95 * 2000, (m, fused.single_launch_stats())
    assert fused.single_launch_stats()["violations"] == 0
