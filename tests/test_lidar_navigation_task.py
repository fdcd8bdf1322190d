"""CPU: the LiDAR navigation task (magpie + magpie_acceleration_control + the 48 x 120 dome) pinned bit for bit.  The CPU oracle and
the numpy restatements the GPU tests compare against (tests/lidar_ref.py, and radar_ref.reward / reward_inputs with radar=False)
both equal tests/golden/cr/*.npz -- the reference's own code with correctly rounded elementary functions
(`python oracle/gen_golden_lidar_nav.py --cr`) -- with zero differing bits: reward, time to collision and pooled image without and
with the three noise rules, all 17 + 320 observation columns, what compute_rewards_and_crashes derives from general frames, and
every recorded output of the magpie's root-link-wrench sub-step."""
import os
import subprocess
import sys

import lidar_ref as L
import numpy as np
import pytest
from conftest import GOLDEN, ROOT, golden_params
from task_test_util import bits, load_golden

CR = "cr"
FIXTURES = ("reward_lidar_navigation", "lidar_image_obs", "obs_lidar_navigation", "step_magpie_acceleration",
            "reward_frames_lidar_navigation")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def low_rows(a, oh=16, ow=20):
    """the reference draws its low-value tensors for the pooled rows 10 .. 15 only: rows 0 .. 9 in front, [N, 16, 20]"""
    return np.concatenate([np.zeros((a.shape[0], oh - a.shape[1], ow), np.float32), a], axis=1)


def reward_args(g, pos_err=None, yaw_error=None):
    return (g["pos_err"] if pos_err is None else pos_err, g["vveh"], g["wbody"], g["yaw_error"] if yaw_error is None else yaw_error,
            g["crashes"], g["action"], g["prev_action"], g["time_to_collision"], float(g["curriculum_progress"]), g["rp"])


def image_args(g):
    return np.ascontiguousarray(g["pointcloud"][:, 0]), g["robot_position"], g["robot_linvel"]


def image_noise(g, tag=""):
    return g[tag + "noise_mask"], g[tag + "noise_val"], g[tag + "max_mask"], low_rows(g[tag + "low_mask"]), low_rows(g[tag + "low_val"])


def obs_args(g):
    return (g["state"][:, 0:3], g["qveh"], g["euler"], g["vbody"], g["wbody"], g["actions"], g["target"], g["target_yaw"], g["u_vec"],
            g["u_euler"], g["downsampled"])


def test_reward_equals_the_correctly_rounded_reference_bit_for_bit(orc):
    g = load_golden("reward_lidar_navigation", CR)
    assert g["reward"].shape == (768,)
    assert same(orc.reward_lidar_navigation(*reward_args(g)), g["reward"])
    assert same(L.lidar_reward(*reward_args(g)), g["reward"])
    assert (L.reward(*reward_args(g), radar=True) != g["reward"]).sum() >= 200  # the other side of the x-velocity clamp


def test_image_equals_the_correctly_rounded_reference_bit_for_bit(orc):
    g = load_golden("lidar_image_obs", CR)
    pc, pos, vel = image_args(g)
    noise, overlap = image_noise(g), image_noise(g, "overlap_")
    assert g["clean_ds"].size == g["noisy_ds"].size == g["overlap_ds"].size == 1920
    names = ("noise_mask", "noise_val", "max_mask", "low_mask", "low_val")
    for name, fn in (("oracle", lambda *masks: orc.lidar_image_obs(pc, pos, vel, **dict(zip(names, masks)))),
                     ("restatement", lambda *masks: L.image_obs(orc, pc, pos, vel, *masks))):
        clean, noisy, met = fn(), fn(*noise), fn(*overlap)
        assert same(clean[0], g["clean_ttc"]) and same(clean[1], g["clean_ds"]), name
        assert same(noisy[0], g["noisy_ttc"]) and same(noisy[1], g["noisy_ds"]), name
        assert same(met[0], g["overlap_ttc"]) and same(met[1], g["overlap_ds"]), name
    # the first fixture exercises each rule
    nm, mm, lm = (a.reshape(6, 320) == 1 for a in (noise[0], noise[2], noise[3]))
    assert (nm & ~mm & ~lm).sum() >= 20 and (mm & ~lm).sum() >= 10 and lm.sum() >= 5 and not lm[:, :200].any()
    # ... the second (the generator's first seed for which this holds) makes them meet: every pair of rules in one cell -- a later
    # rule wins, in the order noise, max, low -- and a low value in the pooled rows 10 and 15, the first and the last that hold one
    nm, mm, lm = (a.reshape(6, 320) == 1 for a in (overlap[0], overlap[2], overlap[3]))
    assert (nm & mm & ~lm).any() and (mm & lm).any() and (nm & lm & ~mm).any() and lm[:, 200:220].any() and lm[:, 300:320].any()
    for ds, (nm, mm, lm), lv in ((g["noisy_ds"], (a.reshape(6, 320) == 1 for a in (noise[0], noise[2], noise[3])), noise[4]),
                                 (g["overlap_ds"], (nm, mm, lm), overlap[4])):
        assert (ds[mm & ~lm] == np.float32(0.1)).all() and same(ds[lm], np.float32(1.0) / lv.reshape(6, 320)[lm])
        assert same(ds[~nm & ~mm & ~lm], g["clean_ds"][~nm & ~mm & ~lm]) and (ds[nm & ~mm & ~lm] < g["clean_ds"][nm & ~mm & ~lm]).all()


def test_observation_equals_the_correctly_rounded_reference_bit_for_bit(orc):
    """all 337 columns of the 96 rows, the yaw error of column 6 included"""
    g = load_golden("obs_lidar_navigation", CR)
    assert g["obs"].shape == (96, 337)
    s, qveh, euler, vbody, wbody, actions, target, tyaw, uv, ue, ds = obs_args(g)
    assert same(orc.obs_lidar_navigation(g["state"], euler, qveh, vbody, wbody, actions, target, tyaw, uv, ue, ds), g["obs"])
    assert same(L.obs(*obs_args(g)), g["obs"])
    wrapped = tyaw - g["obs"][:, 6]
    assert (np.abs(tyaw - L.ssa(euler[:, 2])) > np.pi).sum() >= 10 and np.abs(wrapped).max() > np.pi  # column 6 wraps in the fixture


def test_reward_inputs_equal_the_correctly_rounded_reference_bit_for_bit(orc):
    """compute_rewards_and_crashes (:472-553) on general frames: the vehicle-frame position error, the yaw error and the reward"""
    g = load_golden("reward_frames_lidar_navigation", CR)
    pe, ye = L.reward_inputs(g["target"], g["robot_position"], g["robot_vehicle_orientation"], g["robot_euler_angles"][:, 2], g["target_yaw"])
    assert same(pe, g["pos_err"]) and same(ye, g["yaw_error"])
    assert same(L.lidar_reward(*reward_args(g, pe, ye)), g["reward"])
    assert same(orc.reward_lidar_navigation(*reward_args(g, pe, ye)), g["reward"])
    # dropping either ssa shows
    once = L.ssa(g["target_yaw"] - g["robot_euler_angles"][:, 2])
    inner_only = g["target_yaw"] - L.ssa(g["robot_euler_angles"][:, 2])
    assert (bits(once) != bits(g["yaw_error"])).sum() >= 100 and (bits(inner_only) != bits(g["yaw_error"])).sum() >= 100


def test_reward_frames_fixture_is_what_it_claims():
    g = load_golden("reward_frames_lidar_navigation", CR)
    n = 768
    yaw, pi = g["robot_euler_angles"][:, 2], np.float32(np.pi)
    assert g["reward"].shape == (n,) and same(yaw[0:6], [pi, np.nextafter(pi, np.float32(0)), np.nextafter(pi, np.float32(4)), -pi,
                                                          np.nextafter(-pi, np.float32(0)), np.nextafter(-pi, np.float32(-4))])
    for lo, hi in ((np.pi - 0.5, np.pi), (np.pi, np.pi + 0.5), (-np.pi, -np.pi + 0.5), (-np.pi - 0.5, -np.pi)):
        assert ((yaw > lo) & (yaw < hi)).sum() >= 15, (lo, hi)
    d = g["target_yaw"] - L.ssa(yaw)
    assert (d > np.pi).sum() >= 50 and (d < -np.pi).sum() >= 50 and (np.abs(d) < np.pi).sum() >= 50
    dist = np.linalg.norm(g["pos_err"], axis=1)
    assert (dist < 1).sum() >= 50 and ((dist > 1) & (dist < 3)).sum() >= 50 and (dist > 3).sum() >= 50
    assert (~g["vveh"].any(axis=1)).sum() == 12 and 30 <= g["crashes"].sum() <= 150
    assert (g["reward"][g["crashes"]] == g["rp"][21]).all() and np.abs(g["yaw_error"]).max() <= pi
    q = g["robot_vehicle_orientation"]
    assert np.abs(q[:, 0:2]).max() < 1e-6 and np.abs(q[:, 2]).min() > 0 and np.abs(g["robot_position"]).max() > 10  # yaw-only, not the identity


def test_magpie_substep_equals_the_correctly_rounded_reference_bit_for_bit(orc):
    """BaseMultirotor.step with the wrench A u on the root body + the oracle integrator: every recorded output of all six steps (the
    last one with 30-fold actions), disturbance draws included"""
    g = load_golden("step_magpie_acceleration", CR)
    pd = golden_params(g)
    assert pd["root_link_mode"] == 1 and g["application_mask"].tolist() == [0]
    P = orc.make_params(pd)
    K = g["state"].shape[0]
    assert K == 6 and all(g["disturb"][k].any() for k in range(K))
    for k in range(K):
        st, th = g["state"][k].copy(), g["thrust_in"][k].copy()
        o = orc.substep(P, st, g["action"][k], th, g["kT"], g["tau_inc"], g["tau_dec"], g["Kp"], g["Kv"], g["KR"], g["Kw"],
                        disturb=g["disturb"][k], disturb_max=g["disturb_max"], integrate=True)
        for name, got in (("euler", o.euler), ("qveh", o.qveh), ("vveh", o.vveh), ("vbody", o.vbody), ("wbody", o.wbody),
                          ("wrench_cmd", o.wrench_cmd), ("action_after", o.action_clipped), ("thrust_out", th)):
            assert same(got, g[name][k]), (k, name)
        root = np.concatenate([g["force"][k][:, 0, :], g["torque"][k][:, 0, :]], axis=1)  # nothing acts on the prop bodies
        assert same(o.body_wrench, root) and not g["force"][k][:, 1:].any() and not g["torque"][k][:, 1:].any(), k
        if k + 1 < K:
            assert same(st, g["state"][k + 1]), k


def test_device_noise_restatement_is_the_rule_of_its_docstring(orc):
    """blocks 2c and 2c + 1 of stream RNG_LIDAR_NOISE per cell; the thresholds in float32; the low rule from its first row on"""
    n, cells, ow = 5, 24, 4
    steps = np.array([3, 3, 9, 0, 41])
    u = orc.rng_fill(77, steps, L.RNG_LIDAR_NOISE, 8 * cells).reshape(n, cells, 8)
    for r0 in (0, 3, 5, 6):
        nm, nv, mm, lm, lv = L.device_noise(orc, 77, steps, cells, ow, r0)
        assert np.array_equal(nm == 1, u[..., 0] < np.float32(0.03)) and set(np.unique(nm)) <= {0.0, 1.0}
        assert same(nv, np.float32(9.8) * u[..., 1] + np.float32(0.2)) and same(lv, np.float32(0.8) * u[..., 4] + np.float32(0.2))
        assert np.array_equal(mm == 1, u[..., 2] < np.float32(0.02))
        assert np.array_equal(lm == 1, (u[..., 3] < np.float32(0.02)) & (np.arange(cells)[None, :] >= r0 * ow))
    assert not np.array_equal(u[0], u[1])  # the same step, another env: other draws
    uv, ue = L.obs_draws(orc, 5, steps)
    assert same(np.concatenate([uv, ue], axis=1), orc.rng_fill(5, steps, L.RNG_OBS_NOISE, 6))


def test_fixtures_are_small():
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN, CR, name + ".npz")) < 512 * 1024, name


def test_generator_reproduces_the_committed_fixtures(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_shells

    if not ref_shells.reference_available():
        pytest.skip("the reference tree is not on this machine")
    cmd = [sys.executable, os.path.join(ROOT, "oracle", "gen_golden_lidar_nav.py"), "--cr", "--out", str(tmp_path)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    made = set(os.listdir(tmp_path))
    for name in FIXTURES:
        assert name + ".npz" in made, name
        a, b = np.load(tmp_path / (name + ".npz")), load_golden(name, CR)
        assert sorted(a.files) == sorted(b.files), name
        for key in b.files:
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), (name, key)
