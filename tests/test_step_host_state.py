"""Host state of an env step (env_manager.py module docstring) on an EnvManager without a device: the record of what a step's
launches have already produced, and the parity, which is read from the buffers and nowhere else."""
import pytest


def _env(n=8):
    from aerial_gym_simulator_amd.config.task_config import position_setpoint_task_config as cfg
    from aerial_gym_simulator_amd.task.position_setpoint_task import PositionSetpointTask

    old = (cfg.controller_name, cfg.num_envs, cfg.device, cfg.seed)  # (the task writes its arguments into the shared config class)
    try:
        cfg.controller_name = "lee_position_control"
        return PositionSetpointTask(cfg, num_envs=n, device="cpu", seed=3).sim_env
    finally:
        cfg.controller_name, cfg.num_envs, cfg.device, cfg.seed = old


def test_record_mark_has_take():
    env = _env()
    names = (env.REWARD, env.RESET_SET, env.OBSERVATION, env.SENSOR_POSES, env.TARGETS)
    assert len(set(names)) == 5
    for what in names:
        assert not env.has_produced(what) and not env.take_produced(what)
    env.mark_produced(env.OBSERVATION)
    env.mark_produced(env.RESET_SET)
    for what in names:
        assert env.has_produced(what) == (what in (env.OBSERVATION, env.RESET_SET))
    assert env.has_produced(env.RESET_SET) and env.has_produced(env.RESET_SET)  # looking does not clear
    assert env.take_produced(env.OBSERVATION) and not env.take_produced(env.OBSERVATION)  # taking does, once
    assert env.has_produced(env.RESET_SET) and not env.has_produced(env.OBSERVATION)
    env.mark_produced(env.RESET_SET)  # marking twice is marking once
    assert env.take_produced(env.RESET_SET) and not env.has_produced(env.RESET_SET)


def test_begin_of_call_clears_the_record_and_counts_the_call():
    env = _env()
    for what in (env.REWARD, env.RESET_SET, env.OBSERVATION, env.SENSOR_POSES, env.TARGETS):
        env.mark_produced(what)
    calls = env._calls
    env._begin_call()
    assert not any(env.has_produced(w) for w in (env.REWARD, env.RESET_SET, env.OBSERVATION, env.SENSOR_POSES, env.TARGETS))
    assert env._calls == calls + 1
    env.mark_produced(env.REWARD)
    env._begin_call(counted=False)  # the position task's own one-call step: cleared all the same, not counted
    assert not env.has_produced(env.REWARD) and env._calls == calls + 1


def test_parity_without_buffers_is_zero_and_read_only():
    env = _env()
    assert env._buffers is None and env._parity == 0
    with pytest.raises(AttributeError):
        env._parity = 1
    assert env._parity == 0
