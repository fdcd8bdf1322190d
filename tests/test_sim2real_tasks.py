"""CPU: the two lmf2 sim2real set-point tasks -- registry, configs, the `aerial_gym` alias, the opt-in env argument, and the numpy
restatement the GPU tests compare against (tests/sim2real_ref.py) pinned to the reference's own code through
tests/golden/sim2real_*.npz, tests/golden/sim2real_cr/ (tests/golden_gen/gen_golden_sim2real.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import sim2real_ref as R
import torch
from conftest import ROOT
from task_test_util import config_restored, load_golden
from task_test_util import same_bits as same

CR = "sim2real_cr"  # the fixtures made by the reference's code with correctly rounded elementary functions
CONFIG_KEYS = ("seed", "num_envs", "headless", "device", "use_warp", "args", "episode_len_steps")
KINDS = (("velocity", R.VELOCITY), ("acceleration", R.ACCELERATION))
NAMES = {"velocity": "position_setpoint_task_sim2real", "acceleration": "position_setpoint_task_acceleration_sim2real"}


def test_registry_holds_both_tasks_and_configs_equal_the_reference():
    import aerial_gym_simulator_amd as ag

    g = load_golden("sim2real_config")
    for kind, _ in KINDS:
        assert NAMES[kind] in ag.task_registry.get_task_names()
        cfg = ag.task_registry.get_task_config(NAMES[kind])
        for key, value in json.loads(str(g[kind])).items():
            assert getattr(cfg, key) == value, (kind, key)
        assert cfg.reward_parameters == {} and cfg.args == {"ray_cast_sensors": "off"}
    from aerial_gym_simulator_amd.task.position_setpoint_task_sim2real import (PositionSetpointTaskAccelerationSim2Real,
                                                                              PositionSetpointTaskSim2Real)

    assert ag.task_registry.get_task_class(NAMES["velocity"]) is PositionSetpointTaskSim2Real
    assert ag.task_registry.get_task_class(NAMES["acceleration"]) is PositionSetpointTaskAccelerationSim2Real


def test_alias_config_modules_export_task_config():
    from aerial_gym.config.task_config.position_setpoint_task_acceleration_sim2real_config import task_config as acc
    from aerial_gym.config.task_config.position_setpoint_task_sim2real_config import task_config as vel
    from aerial_gym.registry.task_registry import task_registry

    assert vel is task_registry.get_task_config(NAMES["velocity"]) and vel.controller_name == "lmf2_velocity_control"
    assert acc is task_registry.get_task_config(NAMES["acceleration"]) and acc.controller_name == "lmf2_acceleration_control"


def test_ray_cast_sensors_argument_is_opt_in():
    """lmf2 keeps enable_camera = True: without the argument use_warp=False raises as before; with it no sensor is created."""
    from aerial_gym_simulator_amd.config.robot_config import LMF2Cfg
    from aerial_gym_simulator_amd.sim.sim_builder import SimBuilder

    assert LMF2Cfg.sensor_config.enable_camera is True
    build = lambda args: SimBuilder().build_env("base_sim", "empty_env", "lmf2", "lmf2_velocity_control", "cpu", args=args, num_envs=4,  # noqa: E731
                                                use_warp=False, headless=True)
    for args in ({}, None, {"ray_cast_sensors": "on"}):
        with pytest.raises(ValueError, match="use_warp=True"):
            build(args)
    with pytest.raises(ValueError, match="ray_cast_sensors"):
        build({"ray_cast_sensors": False})
    env = build({"ray_cast_sensors": "off"})
    assert env.robot_manager.warp_sensor is None and "depth_range_pixels" not in env.get_obs()


@pytest.mark.parametrize("kind,k", KINDS)
def test_tasks_build_with_the_reference_attributes(kind, k):
    import aerial_gym_simulator_amd as ag

    cfg = ag.task_registry.get_task_config(NAMES[kind])
    with config_restored(cfg, CONFIG_KEYS):
        cfg.device = "cpu"
        t = ag.task_registry.make_task(NAMES[kind], num_envs=8, headless=True)
    for name in ("actions", "prev_actions", "actions_vehicle_frame", "prev_actions_vehicle_frame"):
        assert tuple(getattr(t, name).shape) == (8, 4)
    assert tuple(t.prev_dist.shape) == (8,) and tuple(t.target_position.shape) == (8, 3)
    assert set(t.task_obs) == {"observations", "priviliged_obs", "collisions", "rewards"} and t.task_obs["observations"].shape == (8, 17)
    assert t.terminations is t.obs_dict["crashes"] and t.truncations is t.obs_dict["truncations"]
    assert t.action_space.shape == (4,) and t.observation_space["observations"].shape == (13,)
    assert t.KIND == k
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.step(torch.zeros(8, 4))


def reward_outputs(g, kind, k):
    G = lambda n: g[kind + "_" + n]  # noqa: E731
    n = G("reward").shape[0]
    return R.reward(k, G("target"), G("position"), G("orientation"), G("vehicle_orientation"), G("body_linvel"), G("crashes_in"),
                    np.zeros(n, np.int32), G("actions"), G("prev_actions"), G("prev_dist"), G("prev_actions_vehicle_frame"), 800)


def obs_outputs(g):
    s = g["state"]
    return R.observation(g["target"], s[:, 0:3], s[:, 3:7], g["body_linvel"], g["body_angvel"], g["robot_actions"], g["z"])


def replay_glue(g, kind, k):
    """the step ordering of tests/sim2real_ref.py on the scripted simulator's recorded tensors -> arrays named like the golden's"""
    T, n = g[kind + "_rewards"].shape
    G = lambda name, t: g[kind + "_" + name][t]  # noqa: E731
    ref = R.TaskRef(k, n)
    out = {}
    buf = np.zeros((n, 4), np.float32)  # the caller's buffer, reused while the golden's caller reused it (steps 0-6)
    q_dict = G("pre_orientation", 0).copy()
    for t in range(T):
        ref.target = G("target", t).copy()
        if t < 7:
            buf[:] = G("action_in", t)
            handed = buf
        else:
            handed = G("action_in", t).copy()
        assert same(q_dict, G("pre_orientation", t))  # the sign-flipped quaternion of the previous observation is what the next step reads
        ref.pre_step(G("pre_position", t), q_dict, handed)
        r = ref.reward(G("robot_position", t), G("robot_orientation", t), G("robot_vehicle_orientation", t), G("robot_body_linvel", t),
                       G("crashes", t), G("sim_steps", t), int(g["episode_len_steps"]))
        obs, q_dict = ref.observation(G("post_robot_position", t), G("post_robot_orientation", t), G("post_robot_body_linvel", t),
                                      G("post_robot_body_angvel", t), G("post_robot_actions", t), G("z", t))
        rec = dict(prev_actions=ref.prev_actions, prev_dist=ref.prev_dist, action_after=handed, rewards=r["reward"],
                   terminations=r["crashes"], truncations=r["truncations"], reset_mask=r["reset_mask"].astype(np.uint8),
                   observations=obs, orientation_after=q_dict)
        if k == R.ACCELERATION:
            rec.update(actions_vehicle_frame=ref.actions_vehicle_frame, prev_actions_vehicle_frame=ref.prev_actions_vehicle_frame)
        for name, v in rec.items():
            out.setdefault(name, []).append(np.array(v, copy=True))
    return {name: np.stack(v) for name, v in out.items()}


def test_restatement_equals_the_correctly_rounded_reference_bit_for_bit():
    """every env of every golden: reward, crashes, vehicle-frame actions; observation and quaternion write-back (w < 0, w = +-0,
    yaw next to +-pi among the rows); every array the reference's real step() produced on the scripted simulator"""
    g = load_golden("sim2real_reward", CR)
    for kind, k in KINDS:
        r = reward_outputs(g, kind, k)
        assert same(r["reward"], g[kind + "_reward"]), kind
        assert np.array_equal(r["crashes"], g[kind + "_crashes_out"].astype(bool)), kind
        if k == R.ACCELERATION:
            assert same(r["actions_vehicle_frame"], g[kind + "_actions_vehicle_frame"])
        dist = r["dist"]
        assert (dist < 0.2).sum() > 50 and (dist > 10).sum() > 10 and 100 < (dist < g[kind + "_prev_dist"]).sum() < 668
    g = load_golden("sim2real_obs", CR)
    obs, q = obs_outputs(g)
    assert same(obs, g["obs"]) and same(q, g["orientation_after"])
    w = g["state"][:, 6]
    assert (w < 0).sum() > 20 and w[0] == 0 and not np.signbit(w[0]) and w[1] == 0 and np.signbit(w[1])
    assert not g["orientation_after"][0:2].any()  # sign(+-0) = 0: the reference zeroes the quaternion there
    g = load_golden("sim2real_glue", CR)
    for kind, k in KINDS:
        out = replay_glue(g, kind, k)
        for name, v in out.items():
            assert same(v, g[kind + "_" + name]), (kind, name)
        assert g[kind + "_truncations"].any() and g[kind + "_terminations"].any()
        # caller aliasing: while the buffer was reused, prev_actions of step t is what the buffer read at call t, i.e. the new
        # action itself (un-doubled); with fresh tensors it is the previous call's tensor as the task left it (doubled)
        assert same(g[kind + "_prev_actions"][3], g[kind + "_action_in"][3])
        assert same(g[kind + "_prev_actions"][9], g[kind + "_action_after"][8])
    assert same(g["acceleration_action_after"][:, :, 0:3], np.float32(2.0) * g["acceleration_action_in"][:, :, 0:3])
    assert same(g["velocity_action_after"], g["velocity_action_in"])


# largest |restatement - plain torch golden| measured on the CPU build the goldens were made with (the differences are torch's
# own last bits in exp / sin / cos / atan2: SLEEF, libm), per output over both kinds
MEASURED = {"reward": 1.9073486e-06, "actions_vehicle_frame": 0.0, "obs": 4.0233135e-07, "orientation_after": 0.0,
            "glue_rewards": 3.0517578e-05, "glue_observations": 4.1723251e-07}


def test_restatement_against_the_plain_torch_reference():
    """Against the reference run with torch's own elementary functions.  Measured here (max |difference| over every env, both
    kinds): reward 1.9e-06 (velocity 0.0, acceleration 1.9e-06: rewards are O(10) and multiply a difference of two distances by
    400-1200), vehicle-frame actions 0.0 (no elementary function), observation 4.0e-07, quaternion write-back 0.0; glue rewards
    3.1e-05 (the scripted simulator jumps by metres per step: rewards up to 1.2e4; 3.1e-05 = 2^-15 is one ulp of a
    reward of a few hundred), glue observations 4.2e-07.  The bound is four times the measured value (room for torch builds whose SLEEF / libm
    last bits differ); flags and everything without an elementary function are compared exactly."""
    got = {}
    g = load_golden("sim2real_reward")
    for kind, k in KINDS:
        r = reward_outputs(g, kind, k)
        assert np.array_equal(r["crashes"], g[kind + "_crashes_out"].astype(bool))
        got["reward"] = max(got.get("reward", 0.0), float(np.abs(r["reward"] - g[kind + "_reward"]).max()))
        if k == R.ACCELERATION:
            got["actions_vehicle_frame"] = float(np.abs(r["actions_vehicle_frame"] - g[kind + "_actions_vehicle_frame"]).max())
    g = load_golden("sim2real_obs")
    obs, q = obs_outputs(g)
    got["obs"] = float(np.abs(obs - g["obs"]).max())
    got["orientation_after"] = float(np.abs(q - g["orientation_after"]).max())
    g = load_golden("sim2real_glue")
    for kind, k in KINDS:
        out = replay_glue(g, kind, k)
        for name in ("terminations", "truncations", "reset_mask", "prev_actions", "action_after", "prev_dist"):
            assert same(out[name], g[kind + "_" + name]), (kind, name)
        got["glue_rewards"] = max(got.get("glue_rewards", 0.0), float(np.abs(out["rewards"] - g[kind + "_rewards"]).max()))
        got["glue_observations"] = max(got.get("glue_observations", 0.0), float(np.abs(out["observations"] - g[kind + "_observations"]).max()))
    print("sim2real restatement vs plain torch goldens (max abs):", got)
    for name, value in got.items():
        assert value <= 4.0 * MEASURED[name], (name, value, MEASURED[name])


@pytest.mark.parametrize("cr", [False, True])
def test_generator_reproduces_the_committed_goldens(cr, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_shells

    if not ref_shells.reference_available():
        pytest.skip("the reference tree is not on this machine")
    cmd = [sys.executable, os.path.join(ROOT, "tests", "golden_gen", "gen_golden_sim2real.py"), "--out", str(tmp_path)] + (["--cr"] if cr else [])
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    for name in ("sim2real_reward", "sim2real_obs", "sim2real_glue", "sim2real_config"):
        a, b = np.load(tmp_path / (name + ".npz")), load_golden(name, CR if cr else None)
        assert sorted(a.files) == sorted(b.files), name
        for key in b.files:
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), (name, key)
