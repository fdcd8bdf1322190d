"""GPU: the host state of an env step (env_manager.py module docstring) on call sequences the public API allows besides
task.step(): the step driven three ways, explicit resets between steps, another current stream, and the exact library calls
of a steady-state task.step() of every task."""
import contextlib

import pytest
import torch

from aerial_gym_simulator_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@contextlib.contextmanager
def _task(name, n, **cfg_values):
    """make_task writes its arguments into the (shared) config class: everything is put back"""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    cfg = task_registry.get_task_config(name)
    keys = ("seed", "num_envs", "headless", "device", "use_warp", "args", "episode_len_steps", "controller_name", "return_state_before_reset")
    old = {k: getattr(cfg, k) for k in keys}
    try:
        cfg.device = DEV
        for k, v in cfg_values.items():
            setattr(cfg, k, v)
        yield task_registry.make_task(name, seed=5, num_envs=n, headless=True)
    finally:
        for k, v in old.items():
            setattr(cfg, k, v)


def _position(n, **cfg_values):
    cfg_values.setdefault("args", {"rng_seed": 1234})
    return _task("position_setpoint_task", n, controller_name="lee_position_control", **cfg_values)


def _log_checks(monkeypatch):
    """every library call goes through _lib.check(code, what): the list of `what`, in call order"""
    log, real = [], _lib.check

    def check(code, what=""):
        log.append(what)
        return real(code, what)

    monkeypatch.setattr(_lib, "check", check)
    return log


def _episodes(task):
    return int(task.sim_env.global_tensor_dict["episode_count"].sum())


def test_three_ways_to_drive_the_position_task_agree():
    """the one-call step, the general path (an action tensor the one-call step does not take) and the EnvManager API called by
    hand as the general path calls it: same seed, same actions -> every buffer bit-identical after every step, also while one
    twin changes between the forms.  83 envs: a partial quad wave; episodes of 9 steps: every env truncates in every 10th step."""
    from test_gpu_single_launch_step import _tensors

    n = 83
    with _position(n, episode_len_steps=9) as a_task, _position(n, episode_len_steps=9) as b_task, \
            _position(n, episode_len_steps=9) as c_task:
        twins = (a_task, b_task, c_task)
        assert a_task._plan is not None and a_task._proof_watch is not None  # single_launch_step at its default: on
        wide = torch.zeros(n, 8, device=DEV)

        def fast(task, a):
            count = sum(task._plan.mode_count)
            task.step(a)
            assert sum(task._plan.mode_count) == count + 1

        def general(task, a):
            wide[:, ::2] = a
            v = wide[:, ::2]
            assert not v.is_contiguous() and torch.equal(v, a)
            count = sum(task._plan.mode_count)
            task.step(v)
            assert sum(task._plan.mode_count) == count

        def by_hand(task, a):
            env = task.sim_env
            task.actions = a
            env.step(actions=a)
            task.compute_rewards_and_crashes(task.obs_dict)
            env.post_reward_calculation_step()
            task.get_return_tuple()

        def same(t):
            torch.cuda.synchronize()
            ref = _tensors(a_task)
            for other in (b_task, c_task):
                for k, v in _tensors(other).items():
                    assert torch.equal(ref[k], v), (t, k)

        for task in twins:
            task.reset()
        same(-1)
        before = _episodes(a_task)
        gen = torch.Generator(device=DEV).manual_seed(2)
        for t in range(50):
            a = torch.rand(n, 4, device=DEV, generator=gen) * 2 - 1
            (general if 40 <= t < 45 else fast)(a_task, a)  # steps 40 .. 44 in b's form, then back
            general(b_task, a)
            by_hand(c_task, a)
            same(t)
        assert _episodes(a_task) >= before + 4 * n
        assert a_task.single_launch_stats()["violations"] == 0


def test_observation_after_an_explicit_reset_is_of_the_reset_state():
    """return_state_before_reset: the reset launch of task.step() writes an observation nobody asks for any more; an explicit
    reset_idx() behind it must not let get_return_tuple() take that one for current.  The observation is subtractions and copies
    of dict tensors: bit for bit."""
    n = 83
    with _position(n, return_state_before_reset=True) as task:
        task.reset()
        gen = torch.Generator(device=DEV).manual_seed(3)
        for _ in range(3):
            task.step(torch.rand(n, 4, device=DEV, generator=gen) * 2 - 1)
        before = _episodes(task)
        task.reset_idx(torch.arange(0, n, 3, device=DEV))
        obs = task.get_return_tuple()[0]["observations"]
        torch.cuda.synchronize()
        assert _episodes(task) == before + len(range(0, n, 3))
        g = task.obs_dict
        expected = torch.cat((task.target_position - g["robot_position"], g["robot_orientation"], g["robot_body_linvel"],
                              g["robot_body_angvel"]), dim=1)
        assert torch.equal(obs, expected)


def test_sensor_poses_and_targets_after_an_explicit_reset_are_computed_again(monkeypatch):
    """The fused robot-side launch of a per-step reset computes the sensor poses and the targets of the reset envs on the side.
    Called by hand without the render that consumes them, and followed by an explicit reset, that must not make the next render
    cast from the poses of before the reset, nor the next target reset skip."""
    from aerial_gym_simulator_amd.env_manager.env_manager import ResetSet

    n = 40
    with _task("navigation_task", n, episode_len_steps=7, args={"rng_seed": 99}) as task:
        task.reset()
        env, sensor = task.sim_env, task.sim_env.robot_manager.warp_sensor
        before = _episodes(task)
        gen = torch.Generator(device=DEV).manual_seed(2)
        for _ in range(10):
            task.step(torch.rand(n, 4, device=DEV, generator=gen) * 2 - 1)
        assert task._fused_side not in (None, False)
        env.reset_terminated_and_truncated_envs()
        env.reset_idx(torch.arange(n, device=DEV))
        env.render()
        torch.cuda.synchronize()
        assert _episodes(task) >= before + 2 * n  # the truncation of step 8 and the explicit reset
        rendered_from = (sensor.sensor_position.clone(), sensor.sensor_orientation.clone())
        log = _log_checks(monkeypatch)
        sensor.compose_pose()
        torch.cuda.synchronize()
        assert log == ["agx_sensor_pose"]
        assert torch.equal(rendered_from[0], sensor.sensor_position) and torch.equal(rendered_from[1], sensor.sensor_orientation)
        del log[:]
        task._reset_targets(ResetSet(env.global_tensor_dict["reset_mask"]))
        assert log == ["agx_nav_target_reset"]


@pytest.mark.parametrize("form", ["one_call", "general"])
def test_launches_follow_the_current_stream(form):
    """a step on the default stream, then calls under another current stream: the handle is looked up again"""
    n = 83
    with _position(n) as task:
        task.reset()
        a = torch.zeros(n, 8, device=DEV)[:, ::2] if form == "general" else torch.zeros(n, 4, device=DEV)
        task.step(a)
        env, s = task.sim_env, torch.cuda.Stream(DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(s):
            assert env._stream().value == s.cuda_stream
            task.get_return_tuple()
            assert env._stream().value == s.cuda_stream
        torch.cuda.synchronize()


# the library calls of one steady-state task.step(), recorded on the code before the per-step record replaced the five one-shot
# flags: a "skip once" that stopped skipping (or started to) shows here, where the outputs would still be bit-identical
STEP_CALLS = {
    "navigation_task": ["agx_action_transform", "agx_env_step", "agx_scene_reset_refresh", "agx_nav_robot_side", "agx_raycast_camera",
                        "agx_obs_navigation"],
    "lidar_navigation_task": ["agx_action_transform", "agx_env_step", "agx_reward_lidar_navigation", "agx_nav_bookkeeping",
                              "agx_scene_reset_refresh", "agx_nav_robot_side", "agx_raycast_lidar", "agx_lidar_image_obs",
                              "agx_obs_lidar_navigation"],
    "position_setpoint_task_sim2real": ["agx_sim2real_pre_step", "agx_env_step", "agx_sim2real_reward", "agx_reset_masked",
                                        "agx_sim2real_obs"],
    "position_setpoint_task": ["agx_env_step", "agx_post_step_position"],
}


@pytest.mark.parametrize("name,n", [("navigation_task", 40), ("lidar_navigation_task", 40), ("position_setpoint_task_sim2real", 83),
                                    ("position_setpoint_task", 83)])
def test_library_calls_of_a_step(name, n, monkeypatch):
    with (_position(n) if name == "position_setpoint_task" else _task(name, n)) as task:
        task.reset()
        general = name == "position_setpoint_task"  # an action tensor the one-call step does not take
        actions = [(torch.zeros(n, 8, device=DEV)[:, ::2] if general else torch.zeros(n, 4, device=DEV)) for _ in range(5)]
        for a in actions[:4]:
            task.step(a)
        log = _log_checks(monkeypatch)
        task.step(actions[4])
        torch.cuda.synchronize()
        print(name, log)
        assert log == STEP_CALLS[name]


def test_one_call_position_step_is_one_library_call(monkeypatch):
    n = 83
    with _position(n) as task:
        task.reset()
        log = _log_checks(monkeypatch)
        for _ in range(5):
            count = sum(task._plan.mode_count)
            task.step(torch.zeros(n, 4, device=DEV))
            assert sum(task._plan.mode_count) == count + 1
        torch.cuda.synchronize()
        assert log == []  # agx_position_task_step's return code is looked at in place; _lib.check only names a failure
