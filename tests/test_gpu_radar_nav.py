"""GPU: the two kernels of the radar navigation task through the C ABI and the task end to end.  The comparator is tests/radar_ref.py
(a numpy restatement pinned to the reference's own code on the CPU by tests/test_radar_navigation_task.py): every kernel result is
compared with it bit for bit, and with the plain-torch goldens within the bounds of tests/test_gpu_lidar_nav.py."""
import ctypes as C

import numpy as np
import pytest
import radar_ref as R
import torch
from conftest import golden_params, rel_err
from task_test_util import host, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = "radar_navigation_task"
F = np.float32


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _harness(n):
    from gpu_harness import DynHarness

    return DynHarness(golden_params(load_golden("step_quad_velocity")), n)


class ImageRun:
    """agx_radar_image_obs on n envs of H x W points; the outputs are the middle rows of buffers whose first and last row carry
    canaries"""

    CANARY = -77.0

    def __init__(self, pc, position, linvel, ph=3, pw=6, env_index_base=0):
        from aerial_gym_simulator_amd import _lib

        self._lib = _lib
        self.n, self.Hh, self.W = pc.shape[0], pc.shape[1], pc.shape[2]
        self.ph, self.pw = ph, pw
        self.cells = (self.Hh // ph) * (self.W // pw)
        self.H = _harness(self.n)
        state = np.zeros((self.n, 13), np.float32)
        state[:, 0:3], state[:, 6], state[:, 7:10] = position, 1.0, linvel
        self.H.set(state=state)
        self.H.B.env_index_base = env_index_base
        self.pc = T(pc)
        self.ttc = torch.full((self.n + 2,), self.CANARY, device=DEV)
        self.ds = torch.full((self.n + 2, self.cells), self.CANARY, device=DEV)

    def __call__(self, noise=(None, None, None), device_noise=0, seed=0, step=0, pc=None):
        p, H = self._lib.dptr, self.H
        H.B.rng_seed, H.B.step_counter = seed, step
        self.ttc.fill_(self.CANARY)
        self.ds.fill_(self.CANARY)
        keep = [None if a is None else T(np.asarray(a, np.float32).reshape(self.n, self.cells)) for a in noise]
        self._lib.check(H.lib.agx_radar_image_obs(H.B, self.n, self.Hh, self.W, self.ph, self.pw, p(self.pc if pc is None else pc),
                                                  *[p(t) for t in keep], device_noise, p(self.ttc[1:]), p(self.ds[1:]), H.stream()),
                        "agx_radar_image_obs")
        torch.cuda.synchronize()
        ttc, ds = host(self.ttc), host(self.ds)
        assert (ttc[[0, -1]] == self.CANARY).all() and (ds[[0, -1]] == self.CANARY).all()  # the neighbours' rows
        return ttc[1:-1].copy(), ds[1:-1].copy()


def equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_radar_image_obs_on_the_golden_bit_exact(orc):
    g = load_golden("radar_image_obs")
    pc = np.ascontiguousarray(g["pointcloud"][:, 0])
    pos, vel = g["robot_position"], g["robot_linvel"]
    n = pc.shape[0]
    run = ImageRun(pc, pos, vel)
    clean = run()
    assert equal(clean, R.image_obs(orc, pc, pos, vel))
    assert rel_err(clean[0], g["clean_ttc"]) < 2e-6 and rel_err(clean[1], g["clean_ds"]) < 2e-6  # vs the reference's own code
    masks = (g["noise_mask"], g["noise_val"], g["invalid_mask"])
    noisy = run(masks)
    assert equal(noisy, R.image_obs(orc, pc, pos, vel, *masks)) and np.array_equal(noisy[0], clean[0])
    assert rel_err(noisy[1], g["noisy_ds"]) < 2e-6
    # a NULL pointer means no such mask, one by one
    assert equal(run((g["noise_mask"], g["noise_val"], None)), R.image_obs(orc, pc, pos, vel, g["noise_mask"], g["noise_val"], None))
    assert equal(run((None, None, g["invalid_mask"])), R.image_obs(orc, pc, pos, vel, None, None, g["invalid_mask"]))
    # the 16-byte-aligned cloud takes the 16-byte loads, the same cloud 4 bytes off the 4-byte loads: same bits
    assert run.pc.data_ptr() % 16 == 0 and (48 * 120) % 4 == 0
    shifted = torch.zeros(run.pc.numel() + 1, device=DEV)[1:].view_as(run.pc)
    shifted.copy_(run.pc)
    assert shifted.data_ptr() % 16 == 4
    assert equal(run(pc=shifted), clean) and equal(run(masks, pc=shifted), noisy)
    # device generator: stream RNG_RADAR_NOISE of (env, step), block c of pooled cell c
    seed, step = 1234567, 41
    dev = run(device_noise=1, seed=seed, step=step)
    drawn = R.device_noise(orc, seed, np.full(n, step), 320)
    assert equal(dev, R.image_obs(orc, pc, pos, vel, *drawn)) and np.array_equal(dev[0], clean[0])
    assert equal(run(device_noise=1, seed=seed, step=step, pc=shifted), dev)
    assert equal(run(device_noise=1, seed=seed, step=step), dev)  # the same (rng_seed, step_counter): the same result
    other = run(device_noise=1, seed=seed, step=step + 1)
    assert not np.array_equal(other[1] == -1.0, dev[1] == -1.0)  # another step: other masks
    assert equal(other, R.image_obs(orc, pc, pos, vel, *R.device_noise(orc, seed, np.full(n, step + 1), 320)))
    assert not np.array_equal(run(device_noise=1, seed=seed + 1, step=step)[1] == -1.0, dev[1] == -1.0)
    # env i under env_index_base = b is env i + b under base 0
    b = 2
    based = ImageRun(pc[b:], pos[b:], vel[b:], env_index_base=b)(device_noise=1, seed=seed, step=step)
    assert np.array_equal(based[1], dev[1][b:]) and np.array_equal(based[0], dev[0][b:])
    # every earlier stream keeps its id: the LiDAR kernel's draws on the same cloud differ from the radar's
    assert R.RNG_RADAR_NOISE == 11 and orc.RNG_LIDAR_NOISE == 5


def limit_clouds(rng, n, H, W):
    """points at ranges below 0.2 m, above 10 m and exactly at the robot position; env 0: a velocity that approaches some points;
    env 1: every point ahead (x > 0) and the velocity backwards -- it recedes from all of them; env 2: zero velocity"""
    pos = ((rng.random((n, 3)) - 0.5) * 4).astype(np.float32)
    dirs = rng.standard_normal((n, H, W, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    dirs[1, ..., 0] = np.abs(dirs[1, ..., 0]) + F(0.05)
    rng_img = (rng.random((n, H, W)) * 12 + 0.05).astype(np.float32)
    flat = rng_img.reshape(n, -1)
    flat[:, 0], flat[:, 1], flat[:, 2], flat[:, 3] = 0.1, 11.5, 1000.0, 0.0
    flat[:, -1] = 0.0  # ... and in the last point, which the tail of either load path reads twice
    pc = (pos[:, None, None, :] + dirs * rng_img[..., None]).astype(np.float32)
    at_robot = rng_img == 0
    pc[at_robot] = np.broadcast_to(pos[:, None, None, :], pc.shape)[at_robot]
    vel = (rng.standard_normal((n, 3)) * 2).astype(np.float32)
    vel[1] = (-1.5, 0.0, 0.0)
    vel[2] = 0.0
    return np.ascontiguousarray(pc), pos, vel


@pytest.mark.parametrize("H,W", [(3, 6), (6, 12), (9, 18), (7, 13)])
def test_radar_image_obs_at_its_limits(orc, H, W):
    """(3, 6): one cell, 18 points -- three of the four waves hold no point; (6, 12): the 16-byte path with 18 groups; (9, 18): 162
    points, no multiple of 4 -- the 4-byte path; (7, 13): remainder rows and columns are dropped as max_pool2d drops them"""
    n = 3
    rng = np.random.default_rng(100 * H + W)
    pc, pos, vel = limit_clouds(rng, n, H, W)
    run = ImageRun(pc, pos, vel)
    cells = (H // 3) * (W // 6)
    assert run.cells == cells == {(3, 6): 1, (6, 12): 4, (9, 18): 9, (7, 13): 4}[(H, W)]
    assert ((H * W) % 4 == 0) == ((H, W) == (6, 12)) and run.pc.data_ptr() % 16 == 0
    r = np.linalg.norm(pc - pos[:, None, None, :], axis=-1)
    assert (r < 0.2).any(axis=(1, 2)).all() and (r > 10).any(axis=(1, 2)).all() and (r == 0).any(axis=(1, 2)).all()
    clean = run()
    ref = R.image_obs(orc, pc, pos, vel)
    assert equal(clean, ref)
    assert clean[0][0] < 10.0 and clean[0][1] == 10.0 and clean[0][2] == 10.0  # approaching; receding from every point; at rest
    assert clean[1].min() >= F(0.1) and clean[1].max() <= 5.0
    masks = ((rng.random((n, cells)) < 0.5).astype(np.float32), (rng.random((n, cells)) * 9.8 + 0.2).astype(np.float32),
             (rng.random((n, cells)) < 0.5).astype(np.float32))
    assert equal(run(masks), R.image_obs(orc, pc, pos, vel, *masks))
    dev = run(device_noise=1, seed=99, step=7)
    assert equal(dev, R.image_obs(orc, pc, pos, vel, *R.device_noise(orc, 99, np.full(n, 7), cells)))


def test_radar_image_obs_argument_checks():
    from aerial_gym_simulator_amd import _lib

    run = ImageRun(np.zeros((1, 3, 6, 3), np.float32), np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32))
    H, p = run.H, _lib.dptr
    mask = torch.zeros(1, 1, device=DEV)
    bad = [
        (1, 0, 6, 3, 6, p(run.pc), None, None, None),        # no rows
        (1, 3, 6, 4, 6, p(run.pc), None, None, None),        # a pool taller than the image
        (1, 3, 6, 3, 6, None, None, None, None),             # no cloud
        (1, 3, 6, 3, 6, p(run.pc), p(mask), None, None),     # a noise mask without its values
        (1, 128, 128, 3, 6, p(run.pc), None, None, None),    # 64 KiB + 16 bytes of ranges
        (0, 3, 6, 3, 6, p(run.pc), None, None, None),
    ]
    for n, h, w, ph, pw, pc, nm, nv, im in bad:
        code = H.lib.agx_radar_image_obs(H.B, n, h, w, ph, pw, pc, nm, nv, im, 0, p(run.ttc[1:]), p(run.ds[1:]), H.stream())
        assert code != 0, (n, h, w, ph, pw)
    torch.cuda.synchronize()
    assert (host(run.ds) == run.CANARY).all()  # nothing was launched


def test_radar_device_noise_statistics():
    """n = 64 (20480 cells), every point at a range of exactly 5 m (robot at the origin, points of norm 5 in float32): a cell is -1
    (invalid), 1/5 (untouched) or 1 / (5 + (9.8 u + 0.2)) with u in [0, 1), i.e. within [1/15, 1/(5 + 0.2)] evaluated in float32.
    Shares: invalid 0.8 +- 0.015 of all cells, noisy 0.03 +- 0.015 of the others -- a little over five standard deviations each
    (sqrt(0.8 0.2 / 20480) = 0.0028, sqrt(0.03 0.97 / 4096) = 0.0027)."""
    n, H, W = 64, 48, 120
    pts = np.array([[5, 0, 0], [-5, 0, 0], [0, 5, 0], [0, -5, 0], [0, 0, 5], [0, 0, -5], [3, 4, 0], [0, -3, 4], [4, 0, -3]], np.float32)
    rng = np.random.default_rng(5)
    pc = np.ascontiguousarray(pts[rng.integers(0, len(pts), (n, H, W))])
    run = ImageRun(pc, np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32))
    ttc, ds = run(device_noise=1, seed=20251019, step=3)
    assert ds.size == 20480 and (ttc == 10.0).all()
    invalid, plain = ds == -1.0, ds == F(1.0) / F(5.0)
    noisy = ~invalid & ~plain
    lo, hi = F(1.0) / F(15.0), F(1.0) / (F(5.0) + F(0.2))
    assert (ds[noisy] >= lo).all() and (ds[noisy] <= hi).all()
    share_invalid, share_noisy = invalid.mean(), noisy.sum() / (~invalid).sum()
    print("radar device noise: invalid share %.4f, noisy share of the valid cells %.4f" % (share_invalid, share_noisy))
    assert abs(share_invalid - 0.8) <= 0.015 and abs(share_noisy - 0.03) <= 0.015


@pytest.mark.parametrize("n", [768, 1, 65, 257])
def test_reward_radar_navigation(orc, n):
    """the golden's leading n rows: rewards bit for bit against the restatement and within 1e-5 of the reference's own
    compute_reward; truncation, reset mask and reset flag as in the parent's test; entries past n untouched"""
    from aerial_gym_simulator_amd import _lib

    g = {k: v[:n] if v.ndim else v for k, v in load_golden("radar_reward").items()}
    g["rp"] = load_golden("radar_reward")["rp"]
    H = _harness(n)
    # identity vehicle frame at the origin: pos_err = target; euler z = 0: yaw error = ssa(target_yaw - ssa(0))
    state = np.zeros((n, 13), np.float32)
    state[:, 6] = 1.0
    derived = np.zeros((n, 16), np.float32)
    derived[:, 6] = 1.0
    derived[:, 7:10], derived[:, 13:16] = g["vveh"], g["wbody"]
    H.set(state=state, derived=derived)
    pad = 3
    crashes = torch.zeros(n + pad, dtype=torch.bool, device=DEV)
    crashes[:n] = T(g["crashes"])
    crashes[n:] = True
    trunc = torch.full((n + pad,), True, device=DEV)
    reset_mask = torch.full((n + pad,), 9, dtype=torch.uint8, device=DEV)
    sim_steps = torch.full((n + pad,), 500, dtype=torch.int32, device=DEV)
    sim_steps[:n] = torch.arange(n, dtype=torch.int32) % 130
    p = _lib.dptr
    H.B.crashes, H.B.truncations, H.B.reset_mask, H.B.sim_steps = p(crashes), p(trunc), p(reset_mask), p(sim_steps)
    tgt, tyaw = T(g["pos_err"].T.copy()), T(g["yaw_error"])
    act, pact = T(g["action"]), T(g["prev_action"])
    ttc = T(g["time_to_collision"])
    rp = (C.c_float * 22)(*[float(x) for x in g["rp"]])
    cpf = float(g["curriculum_progress"])
    pe_ref, ye_ref = R.reward_inputs(g["pos_err"], np.zeros((n, 3), np.float32), derived[:, 3:7], derived[:, 2], g["yaw_error"])
    assert np.array_equal(pe_ref, g["pos_err"])
    want = R.reward(pe_ref, g["vveh"], g["wbody"], ye_ref, g["crashes"], g["action"], g["prev_action"], g["time_to_collision"], cpf, g["rp"])
    trunc_ref = (np.arange(n) % 130) > 110
    for roc in (1, 0):
        pe, ppe = T(np.full((3, n), 7.0, np.float32)), torch.zeros(3, n, device=DEV)
        rew = torch.full((n + pad,), -55.0, device=DEV)
        H.reset_flag.zero_()
        _lib.check(H.lib.agx_reward_radar_navigation(H.B, n, p(tgt), p(tyaw), p(act), p(pact), p(ttc), rp, cpf, p(pe), p(ppe), 110, roc,
                                                     p(rew), H.stream()), "agx_reward_radar_navigation")
        torch.cuda.synchronize()
        r = host(rew)
        assert np.array_equal(r[:n], want), np.abs(r[:n] - want).max()
        assert rel_err(r[:n], g["reward"]) < 1e-5  # vs the reference's own compute_reward
        assert (r[n:] == -55.0).all()
        assert np.array_equal(host(pe).T, g["pos_err"]) and (host(ppe) == 7.0).all()  # prev <- cur, cur <- new
        reset_ref = trunc_ref | (g["crashes"] if roc else False)
        assert np.array_equal(host(trunc)[:n], trunc_ref) and host(trunc)[n:].all()
        assert np.array_equal(host(reset_mask)[:n].astype(bool), reset_ref) and (host(reset_mask)[n:] == 9).all()
        assert host(H.reset_flag).tolist() == [int(reset_ref.any()), 0]
    if n == 768:
        # the same inputs through the LiDAR entry point: its own formula, which this change leaves as it was
        lidar = R.reward(pe_ref, g["vveh"], g["wbody"], ye_ref, g["crashes"], g["action"], g["prev_action"], g["time_to_collision"], cpf,
                         g["rp"], radar=False)
        pe, ppe, rew = torch.zeros(3, n, device=DEV), torch.zeros(3, n, device=DEV), torch.zeros(n, device=DEV)
        _lib.check(H.lib.agx_reward_lidar_navigation(H.B, n, p(tgt), p(tyaw), p(act), p(pact), p(ttc), rp, cpf, p(pe), p(ppe), 110, 1,
                                                     p(rew), H.stream()), "agx_reward_lidar_navigation")
        torch.cuda.synchronize()
        assert np.array_equal(host(rew), lidar) and (lidar != want).sum() >= 200


def _make(name, n, strict, seed=3):
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    cfg = task_registry.get_task_config(name)
    old = {k: getattr(cfg, k) for k in ("seed", "num_envs", "headless", "device", "use_warp", "args")}
    cfg.device, cfg.args = DEV, {"strict_rng": strict}
    try:
        return task_registry.make_task(name, seed=seed, num_envs=n, headless=True)
    finally:
        for k, v in old.items():
            setattr(cfg, k, v)


@pytest.mark.parametrize("strict", [False, True])
def test_radar_navigation_task_end_to_end(orc, strict):
    """task_registry.make_task("radar_navigation_task") = lmf2_radar + lmf2_acceleration_control + the 48 x 120 radar in
    env_with_obstacles; 48 envs, 140 steps of a fixed random action (episodes of 110 steps: every env ends at least once)"""
    n, steps = 48, 140
    task = _make(NAME, n, strict)
    env, d = task.sim_env, task.obs_dict
    snap = {}
    real_image, real_reward = task.process_image_observation, task.compute_rewards_and_crashes

    def hooked_image():
        snap["image"] = {k: host(d[k]).copy() for k in ("depth_range_pixels", "robot_position", "robot_linvel")}
        return real_image()

    def hooked_reward(obs_dict):
        snap["reward"] = {k: host(d[k]).copy() for k in ("robot_position", "robot_vehicle_orientation", "robot_euler_angles",
                                                          "robot_vehicle_linvel", "robot_body_angvel", "crashes")}
        snap["reward"].update(target=host(task.target_position).copy(), target_yaw=host(task.target_yaw).copy(),
                              action=host(task.current_action).copy(), prev_action=host(task.prev_action).copy(),
                              ttc=host(task.time_to_collision).copy(), cpf=float(task.curriculum_progress_fraction))
        return real_reward(obs_dict)

    task.process_image_observation, task.compute_rewards_and_crashes = hooked_image, hooked_reward
    obs, *_ = task.reset()
    assert obs["observations"].shape == (n, 337) and task.task_config.robot_name == "lmf2_radar" and env.robot_name == "lmf2_radar"
    a = torch.rand(n, 4, device=DEV) * 2 - 1
    ended = 0
    for _ in range(steps):
        obs, rew, term, trunc, info = task.step(a)
        ended += int((term | trunc).sum())
    torch.cuda.synchronize()
    o = obs["observations"]
    assert o.shape == (n, 337) and torch.isfinite(o).all() and torch.isfinite(rew).all()
    cells = host(o[:, 17:])
    invalid = cells == -1.0
    assert (cells[~invalid] >= F(1.0) / F(20.0)).all() and (cells[~invalid] <= 5.0).all()  # 1 / [0.2, 10 (+ 10 of noise)]
    print("radar task, strict" if strict else "radar task, default", "share of invalid cells in the last step: %.4f" % invalid.mean())
    assert cells.size == 15360 and abs(invalid.mean() - 0.8) <= 0.02
    assert float(task.time_to_collision.min()) >= 0.0 and float(task.time_to_collision.max()) <= 10.0
    assert ended >= n
    assert tuple(d["depth_range_pixels"].shape) == (n, 1, 48, 120, 3)
    sensor = env.robot_manager.warp_sensor
    assert np.abs(host(sensor.ray_vectors) - orc.lidar_ray_table(48, 120, -60, 60, -60, 60)).max() < 1.2e-7
    assert torch.equal(task.prev_action, task.action_transformation_function(a))  # the last two actions were identical
    if not strict:
        assert task._noise is None
        return
    # strict mode: the last step's image and reward are the restatement's on the tensors the kernels read, bit for bit
    s = snap["image"]
    masks = [host(t).reshape(n, 320) for t in task._noise]
    assert set(np.unique(masks[0])) <= {0.0, 1.0} and not masks[1][masks[0] == 0].any() and (masks[1][masks[0] == 1] >= 0.2).all()
    ttc_ref, ds_ref = R.image_obs(orc, s["depth_range_pixels"][:, 0], s["robot_position"], s["robot_linvel"], *masks)
    assert np.array_equal(host(task.downsampled_lidar_data), ds_ref) and np.array_equal(host(task.time_to_collision), ttc_ref)
    assert np.array_equal(cells, ds_ref) and np.array_equal(invalid, masks[2] == 1)
    s = snap["reward"]
    pe, ye = R.reward_inputs(s["target"], s["robot_position"], s["robot_vehicle_orientation"], s["robot_euler_angles"][:, 2], s["target_yaw"])
    cfg = task.task_config
    rp = np.array([cfg.reward_parameters[k] for k in cfg.REWARD_PARAMETER_ORDER], np.float32)
    want = R.reward(pe, s["robot_vehicle_linvel"], s["robot_body_angvel"], ye, s["crashes"], s["action"], s["prev_action"], s["ttc"], s["cpf"], rp)
    assert np.array_equal(host(rew), want), np.abs(host(rew) - want).max()
    assert (s["robot_vehicle_linvel"][:, 0] < 0).any() and (s["robot_vehicle_linvel"][:, 0] > 0).any()


def test_two_strict_radar_tasks_of_one_seed_agree():
    n = 48
    runs = []
    a = (torch.rand(n, 4, generator=torch.Generator().manual_seed(8)) * 2 - 1).to(DEV)
    for _ in range(2):
        task = _make(NAME, n, True, seed=11)
        seq = [host(task.reset()[0]["observations"]).copy()]
        for _ in range(5):
            seq.append(host(task.step(a)[0]["observations"]).copy())
        runs.append(np.stack(seq))
        task.close()
    assert np.array_equal(runs[0], runs[1]) and (runs[0][-1, :, 17:] == -1.0).mean() > 0.7


def _step_calls(name, n, monkeypatch):
    """the library calls of one steady-state task.step() (every call goes through _lib.check(code, what)), in call order"""
    from aerial_gym_simulator_amd import _lib

    task = _make(name, n, False, seed=5)
    task.reset()
    actions = [torch.zeros(n, 4, device=DEV) for _ in range(5)]
    for a in actions[:4]:
        task.step(a)
    log, real = [], _lib.check

    def check(code, what=""):
        log.append(what)
        return real(code, what)

    monkeypatch.setattr(_lib, "check", check)
    task.step(actions[4])
    torch.cuda.synchronize()
    monkeypatch.setattr(_lib, "check", real)
    task.close()
    return log


def test_radar_step_launches_are_the_lidar_tasks(monkeypatch):
    """no speed gate: the step runs the parent's launches on the same bytes -- the condition is the launch list"""
    n = 40
    radar, lidar = _step_calls(NAME, n, monkeypatch), _step_calls("lidar_navigation_task", n, monkeypatch)
    swap = {"agx_lidar_image_obs": "agx_radar_image_obs", "agx_reward_lidar_navigation": "agx_reward_radar_navigation"}
    print("radar step:", radar)
    assert radar == [swap.get(x, x) for x in lidar] and all(v in radar for v in swap.values()) and len(radar) >= 8
