"""GPU: the three kernels of the LiDAR navigation task through the C ABI at their limits, bit for bit.  The comparators are
tests/lidar_ref.py and radar_ref.reward / reward_inputs (numpy restatements pinned to the reference's own code on the CPU by
tests/test_lidar_navigation_task.py) and the CPU oracle; equality is on the uint32 view.  Every output buffer is the middle of a
larger one whose first and last rows carry canaries."""
import ctypes as C
import os
import re

import lidar_ref as L
import numpy as np
import pytest
import torch
from conftest import ROOT, golden_params
from sim2real_ref import norm3
from task_test_util import bits, host, load_golden
from test_gpu_radar_nav import limit_clouds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CR = "cr"
F = np.float32
CANARY = -77.0
PAD = 3  # canary entries in front of and behind every output


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _harness(n):
    from gpu_harness import DynHarness

    return DynHarness(golden_params(load_golden("step_quad_velocity")), n)


def yaw_quat(yaw):
    """a vehicle-frame quaternion: yaw only"""
    yaw = np.asarray(yaw, np.float64)
    z = np.zeros_like(yaw)
    return np.stack([z, z, np.sin(yaw / 2), np.cos(yaw / 2)], axis=1).astype(np.float32)


class Guarded:
    """an output of `count` elements in the middle of a buffer filled with a canary value"""

    def __init__(self, count, dtype=torch.float32, canary=CANARY, pad=PAD):
        self.count, self.pad, self.canary = count, pad, canary
        self.full = torch.full((count + 2 * pad,), canary, dtype=dtype, device=DEV)
        self.view = self.full[pad:pad + count]

    def ptr(self):
        from aerial_gym_simulator_amd import _lib

        return _lib.dptr(self.view) if self.count else None

    def read(self):
        a = host(self.full)
        assert (a[: self.pad] == self.canary).all() and (a[self.pad + self.count:] == self.canary).all(), "a write outside the output"
        return a[self.pad:self.pad + self.count].copy()

    def untouched(self):
        return bool((host(self.full) == self.canary).all())


# ---- reward ---------------------------------------------------------------------------------------------------------------------
def identity_rows(g):
    """the rows of reward_lidar_navigation.npz as the kernel's inputs: the robot at the origin with an identity vehicle frame and
    zero yaw (pos_err = target; the yaw error is ssa(yaw_error - ssa(0)))"""
    n = g["pos_err"].shape[0]
    z3 = np.zeros((n, 3), np.float32)
    return dict(position=z3, qveh=yaw_quat(np.zeros(n)), euler_z=np.zeros(n, np.float32), target=g["pos_err"], target_yaw=g["yaw_error"],
                vveh=g["vveh"], wbody=g["wbody"], crashes=g["crashes"], action=g["action"], prev_action=g["prev_action"],
                ttc=g["time_to_collision"], cpf=float(g["curriculum_progress"]), rp=g["rp"])


def frame_rows(g):
    """the rows of reward_frames_lidar_navigation.npz: general positions, vehicle frames, Euler angles and targets"""
    return dict(position=g["robot_position"], qveh=g["robot_vehicle_orientation"], euler_z=g["robot_euler_angles"][:, 2], target=g["target"],
                target_yaw=g["target_yaw"], vveh=g["vveh"], wbody=g["wbody"], crashes=g["crashes"], action=g["action"],
                prev_action=g["prev_action"], ttc=g["time_to_collision"], cpf=float(g["curriculum_progress"]), rp=g["rp"])


def leading(rows, n):
    return {k: (np.ascontiguousarray(v[:n]) if isinstance(v, np.ndarray) and v.ndim and k != "rp" else v) for k, v in rows.items()}


def run_reward(rows, sim_steps, prev_pos_err, episode_len=110, roc=1, parity=0, radar=False):
    """one launch of agx_reward_lidar_navigation (radar: of agx_reward_radar_navigation) on the rows; returns what it wrote"""
    from aerial_gym_simulator_amd import _lib

    n = len(rows["target_yaw"])
    H = _harness(n)
    state = np.zeros((n, 13), np.float32)
    state[:, 0:3], state[:, 6] = rows["position"], 1.0
    derived = np.zeros((n, 16), np.float32)
    derived[:, 2], derived[:, 3:7], derived[:, 7:10], derived[:, 13:16] = rows["euler_z"], rows["qveh"], rows["vveh"], rows["wbody"]
    H.set(state=state, derived=derived)
    p = _lib.dptr
    crashes, steps = T(np.asarray(rows["crashes"], bool)), T(np.asarray(sim_steps, np.int32))
    trunc = Guarded(n, torch.bool, True)
    reset_mask = Guarded(n, torch.uint8, 9)
    reward = Guarded(n)
    pos_err, prev = Guarded(3 * n), Guarded(3 * n)
    pos_err.view.copy_(T(np.asarray(prev_pos_err, np.float32).T.copy()).reshape(-1))
    flags = torch.tensor([5, 5], dtype=torch.int32, device=DEV)
    flags[parity] = 0
    H.B.crashes, H.B.sim_steps, H.B.truncations, H.B.reset_mask = p(crashes), p(steps), trunc.ptr(), reset_mask.ptr()
    H.B.reset_flag, H.B.flag_parity = p(flags), parity
    tgt, tyaw, act, pact, ttc = T(np.asarray(rows["target"], np.float32).T.copy()), T(rows["target_yaw"]), T(rows["action"]), T(rows["prev_action"]), T(rows["ttc"])
    rp = (C.c_float * 22)(*[float(x) for x in rows["rp"]])
    fn = H.lib.agx_reward_radar_navigation if radar else H.lib.agx_reward_lidar_navigation
    _lib.check(fn(H.B, n, p(tgt), p(tyaw), p(act), p(pact), p(ttc), rp, rows["cpf"], pos_err.ptr(), prev.ptr(), episode_len, roc,
                  reward.ptr(), H.stream()), "agx_reward_lidar_navigation")
    torch.cuda.synchronize()
    return dict(reward=reward.read(), pos_err=pos_err.read().reshape(3, n).T, prev_pos_err=prev.read().reshape(3, n).T,
                trunc=trunc.read(), reset_mask=reset_mask.read(), reset_flag=host(flags).tolist())


def check_reward(rows, sim_steps, episode_len, roc, parity, radar=False):
    """the launch against the restatement: reward, pos_err, prev_pos_err <- pos_err, truncations, reset mask and reset flag"""
    n = len(rows["target_yaw"])
    prev_pos_err = (np.arange(3 * n, dtype=np.float32).reshape(n, 3) * F(0.25)) - F(7.0)
    got = run_reward(rows, sim_steps, prev_pos_err, episode_len, roc, parity, radar)
    pe, ye = L.reward_inputs(rows["target"], rows["position"], rows["qveh"], rows["euler_z"], rows["target_yaw"])
    want = L.reward(pe, rows["vveh"], rows["wbody"], ye, rows["crashes"], rows["action"], rows["prev_action"], rows["ttc"], rows["cpf"],
                    rows["rp"], radar=radar)
    assert same(got["reward"], want), (np.flatnonzero(bits(got["reward"]) != bits(want))[:8], np.abs(got["reward"] - want).max())
    assert same(got["pos_err"], pe) and same(got["prev_pos_err"], prev_pos_err)
    trunc = np.asarray(sim_steps) > episode_len
    reset = trunc | (np.asarray(rows["crashes"], bool) if roc else False)
    assert np.array_equal(got["trunc"], trunc) and np.array_equal(got["reset_mask"], reset.astype(np.uint8))
    flags = [5, 5]
    flags[parity] = int(reset.any())
    assert got["reset_flag"] == flags
    return got, pe, ye, want


@pytest.mark.parametrize("n", [768, 1, 65, 257])
@pytest.mark.parametrize("fixture", ["reward_lidar_navigation", "reward_frames_lidar_navigation"])
def test_reward_lidar_navigation_bit_for_bit(orc, fixture, n):
    """the leading n rows of the two correctly rounded fixtures (n = 1, 65, 257: a partly filled wave and block), with and without
    reset_on_collision, either flag parity.  On the frames fixture the kernel's outputs ARE the reference's: position error in the
    vehicle frame and reward equal the fixture itself."""
    g = load_golden(fixture, CR)
    rows = leading(frame_rows(g) if "frames" in fixture else identity_rows(g), n)
    sim_steps = np.arange(n) % 130
    for roc, parity in ((1, 0), (0, 1), (1, 1), (0, 0)):
        got, pe, ye, want = check_reward(rows, sim_steps, 110, roc, parity)
        if "frames" in fixture:
            assert same(got["pos_err"], g["pos_err"][:n]) and same(ye, g["yaw_error"][:n]) and same(got["reward"], g["reward"][:n])
        else:
            assert same(pe, g["pos_err"][:n])
    assert same(orc.reward_lidar_navigation(pe, rows["vveh"], rows["wbody"], ye, rows["crashes"], rows["action"], rows["prev_action"],
                                            rows["ttc"], rows["cpf"], rows["rp"]), got["reward"])


def test_reward_lidar_navigation_hand_placed_rows():
    """distances of exactly 0, 1 and 3 m, a robot at rest (the -0.2 branch), times to collision of 0 and 10 s, sim_steps at and one
    above the episode length, a crash together with a truncation -- and the radar instantiation differs on these rows"""
    g = load_golden("reward_frames_lidar_navigation", CR)
    n = 12
    rows = leading(frame_rows(g), n)
    rows = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in rows.items()}
    rows["rp"] = g["rp"]
    ident = yaw_quat(np.zeros(1))[0]
    for i, target in ((0, (0, 0, 0)), (1, (1, 0, 0)), (2, (0, -3, 0)), (3, (0, 0, 1))):
        rows["position"][i], rows["qveh"][i], rows["target"][i] = 0.0, ident, target
    rows["target"][4] = rows["position"][4]              # at the target in a general frame
    rows["vveh"][0], rows["vveh"][5] = 0.0, 0.0         # at rest
    rows["vveh"][1], rows["vveh"][2] = (1.5, 0.2, 0.0), (-1.5, 0.2, 0.0)  # forwards and backwards
    rows["ttc"][0:4] = (0.0, 10.0, 0.0, 10.0)
    rows["crashes"][:] = False
    rows["crashes"][[3, 7, 9]] = True
    episode_len = 40
    sim_steps = np.array([0, 40, 41, 41, 39, 40, 41, 40, 5, 41, 42, 1000], np.int32)  # 3 and 9: a crash and a truncation
    for roc, parity in ((1, 0), (0, 1)):
        got, pe, ye, lidar = check_reward(rows, sim_steps, episode_len, roc, parity)
        dist = norm3(pe)
        assert dist[0] == 0 and dist[1] == 1 and dist[2] == 3 and dist[3] == 1 and dist[4] == 0
        assert (got["reward"][[3, 7, 9]] == g["rp"][21]).all() and np.isfinite(got["reward"]).all()
        assert got["trunc"].tolist() == [False, False, True, True, False, False, True, False, False, True, True, True]
        _, _, _, radar = check_reward(rows, sim_steps, episode_len, roc, parity, radar=True)
        assert (bits(radar) != bits(lidar)).sum() >= 6 and bits(radar)[1] != bits(lidar)[1] and bits(radar)[2] != bits(lidar)[2]
    # a batch where nothing resets leaves the flag down
    rows["crashes"][:] = False
    got, *_ = check_reward(rows, np.zeros(n, np.int32), episode_len, 1, 1)
    assert got["reset_flag"] == [5, 0] and not got["reset_mask"].any()


# ---- observation ------------------------------------------------------------------------------------------------------------------
N_OBS_ROWS = 260


def obs_rows(cells):
    """260 general rows; rows 0 .. 3 are the edges: Euler angles at +-pi, just beyond, far beyond (+-4, +-2 pi), a target_yaw - yaw
    that wraps either way; row 2: the target AT the robot (a distance of 0: +-inf in columns 0 .. 2)"""
    rng = np.random.default_rng(1000 + cells)
    n, pi = N_OBS_ROWS, F(np.pi)
    r = dict(position=(rng.standard_normal((n, 3)) * 5).astype(np.float32), qveh=yaw_quat(rng.uniform(-np.pi, np.pi, n)),
             euler=rng.uniform(-2 * np.pi, 2 * np.pi, (n, 3)).astype(np.float32), vbody=rng.standard_normal((n, 3)).astype(np.float32),
             wbody=rng.standard_normal((n, 3)).astype(np.float32), actions=rng.standard_normal((n, 4)).astype(np.float32),
             target_yaw=rng.uniform(-np.pi, np.pi, n).astype(np.float32), downsampled=(rng.random((n, cells)) * 5).astype(np.float32),
             u_vec=rng.random((n, 3)).astype(np.float32), u_euler=rng.random((n, 3)).astype(np.float32))
    r["target"] = (r["position"] + rng.standard_normal((n, 3)) * 3).astype(np.float32)
    r["euler"][0] = (pi, -pi, pi)
    r["euler"][1] = (np.nextafter(pi, F(4)), np.nextafter(-pi, F(-4)), -pi)
    r["euler"][2] = (4.0, -4.0, np.nextafter(-pi, F(-4)))
    r["euler"][3] = (2 * pi, -2 * pi, np.nextafter(pi, F(4)))
    r["target_yaw"][0:4] = (-3.0, 3.0, 3.0, -3.0)
    r["target"][2] = r["position"][2]
    r["u_vec"][2] = (0.25, 0.75, 0.125)
    return r


def rows_slice(r, a, b):
    return {k: np.ascontiguousarray(v[a:b]) for k, v in r.items()}


def obs_want(r, u_vec=None, u_euler=None):
    return L.obs(r["position"], r["qveh"], r["euler"], r["vbody"], r["wbody"], r["actions"], r["target"], r["target_yaw"],
                 r["u_vec"] if u_vec is None else u_vec, r["u_euler"] if u_euler is None else u_euler, r["downsampled"])


class ObsRun:
    """agx_obs_lidar_navigation on the rows r"""

    def __init__(self, r, cells, env_index_base=0):
        from aerial_gym_simulator_amd import _lib

        self._lib, self.r, self.cells = _lib, r, cells
        self.n = n = len(r["target_yaw"])
        self.H = H = _harness(n)
        state = np.zeros((n, 13), np.float32)
        state[:, 0:3], state[:, 6] = r["position"], 1.0
        derived = np.concatenate([r["euler"], r["qveh"], np.zeros((n, 3), np.float32), r["vbody"], r["wbody"]], axis=1)
        H.set(state=state, derived=derived, actions=r["actions"])
        H.B.env_index_base = env_index_base
        self.tgt, self.tyaw = T(r["target"].T.copy()), T(r["target_yaw"])
        self.uv, self.ue = T(r["u_vec"]), T(r["u_euler"])
        self.ds = T(r["downsampled"]) if cells else None
        self.dim = 17 + cells
        self.obs = Guarded(n * self.dim, pad=self.dim)

    def __call__(self, host_draws=True, seed=0, step=0, uv=True, ue=True, check=True):
        p, H = self._lib.dptr, self.H
        H.B.rng_seed, H.B.step_counter = seed, step
        self.obs.full.fill_(CANARY)
        code = H.lib.agx_obs_lidar_navigation(H.B, self.n, p(self.tgt), p(self.tyaw), p(self.uv) if host_draws and uv else None,
                                              p(self.ue) if host_draws and ue else None, p(self.ds) if self.cells else None, self.cells,
                                              self.obs.ptr(), H.stream())
        torch.cuda.synchronize()
        if not check:
            return code
        self._lib.check(code, "agx_obs_lidar_navigation")
        return self.obs.read().reshape(self.n, self.dim)

    def bind_rows(self, parity):
        """exchange rows of both parities (plain stores: no step signal, no peer push) and the step's reward, crash and truncation
        flags that the row's tail carries"""
        p, H, n = self._lib.dptr, self.H, self.n
        self.rows = [Guarded(n * (self.dim + 3), pad=self.dim + 3) for _ in range(2)]
        rng = np.random.default_rng(n)
        self.step_reward = T(rng.standard_normal(n).astype(np.float32))
        H.crashes.copy_(T(rng.random(n) < 0.5))
        H.trunc.copy_(T(rng.random(n) < 0.5))
        H.B.step_rows[0], H.B.step_rows[1], H.B.step_reward, H.B.flag_parity = self.rows[0].ptr(), self.rows[1].ptr(), p(self.step_reward), parity
        return np.concatenate([host(self.step_reward)[:, None], host(H.crashes)[:, None].astype(np.float32),
                               host(H.trunc)[:, None].astype(np.float32)], axis=1)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 96, 257])
def test_obs_lidar_navigation_bit_for_bit(orc, n):
    """one wave per env, four envs per block: n = 1, 3, 5 and 257 leave the last block partly empty; cells around the 64-lane stride
    of the copy.  Host draws and the device generator; env_index_base; the exchange rows of either parity."""
    for cells in (0, 1, 63, 64, 65, 320):
        all_rows = obs_rows(cells)
        r = rows_slice(all_rows, 0, n)
        run = ObsRun(r, cells)
        want = obs_want(r)
        got = run()
        assert got.shape == (n, 17 + cells) and same(got, want), (cells, np.argwhere(bits(got) != bits(want))[:6])
        assert same(got, orc.obs_lidar_navigation(run.H.get("state"), r["euler"], r["qveh"], r["vbody"], r["wbody"], r["actions"], r["target"],
                                                  r["target_yaw"], r["u_vec"], r["u_euler"], r["downsampled"])), cells
        assert same(got[:, 17:], r["downsampled"]) and not np.isnan(got).any()
        if n >= 3:
            assert np.isinf(got[2, 0:3]).all() and got[2, 3] == 0 and (np.sign(got[2, 0:3]) == (-1, 1, -1)).all()
        # the device generator: six draws of stream RNG_OBS_NOISE per (env, step)
        seed, step = 99 + cells, 7 + n
        dev = run(host_draws=False, seed=seed, step=step)
        uv, ue = L.obs_draws(orc, seed, np.full(n, step))
        want_dev = obs_want(r, uv, ue)
        assert same(dev, want_dev) and not np.isnan(dev).any() and not same(dev[:, 0:6], got[:, 0:6]), cells
        assert same(run(host_draws=False, seed=seed, step=step + 1)[:, 6:], dev[:, 6:])  # the draws reach columns 0-2, 4 and 5 only
        # env i under env_index_base = b is env i + b under base 0
        b = 2
        if n > b:
            based = ObsRun(rows_slice(all_rows, b, n), cells, env_index_base=b)(host_draws=False, seed=seed, step=step)
            assert same(based, dev[b:]), cells
        # exchange rows: [obs | reward | crash | trunc] at the parity of the step, the other parity's buffer untouched
        for parity in (0, 1):
            tail = run.bind_rows(parity)
            got_rows = run()
            assert same(got_rows, want)
            assert same(run.rows[parity].read().reshape(n, 17 + cells + 3), np.concatenate([want, tail], axis=1)), (cells, parity)
            assert run.rows[parity ^ 1].untouched(), (cells, parity)
            dev_rows = run(host_draws=False, seed=seed, step=step)
            assert same(dev_rows, want_dev) and same(run.rows[parity].read().reshape(n, -1)[:, :17 + cells], want_dev)
            assert run.rows[parity ^ 1].untouched()


def test_obs_lidar_navigation_argument_checks():
    from aerial_gym_simulator_amd import _lib

    r = rows_slice(obs_rows(5), 0, 4)
    run = ObsRun(r, 5)
    H, p = run.H, _lib.dptr
    assert run(uv=False, check=False) != 0 and run(ue=False, check=False) != 0  # one of the two draws
    assert b"u_vec" in H.lib.agx_last_error()
    run.bind_rows(0)
    both = (H.B.step_rows[0], H.B.step_rows[1])
    for rows0, rows1, reward in ((both[0], None, p(run.step_reward)), (None, both[1], p(run.step_reward)), (both[0], both[1], None)):
        H.B.step_rows[0], H.B.step_rows[1], H.B.step_reward = rows0, rows1, reward
        assert run(check=False) != 0 and b"step_rows" in H.lib.agx_last_error()
    H.B.step_rows[0], H.B.step_rows[1], H.B.step_reward = None, None, None
    H.B.flag_parity = 2
    assert run(check=False) != 0
    H.B.flag_parity = 0
    run.cells = -1
    assert run(check=False) != 0
    run.cells = 5
    assert run.obs.untouched() and run.rows[0].untouched() and run.rows[1].untouched()  # nothing was launched
    assert same(run(), obs_want(r))


# ---- image ----------------------------------------------------------------------------------------------------------------------
class ImageRun:
    """agx_lidar_image_obs on n envs of H x W points"""

    def __init__(self, pc, position, linvel, ph=3, pw=6, env_index_base=0):
        from aerial_gym_simulator_amd import _lib

        self._lib = _lib
        self.n, self.Hh, self.W = pc.shape[0], pc.shape[1], pc.shape[2]
        self.ph, self.pw = ph, pw
        self.oh, self.ow = self.Hh // ph, self.W // pw
        self.cells = self.oh * self.ow
        self.H = _harness(self.n)
        state = np.zeros((self.n, 13), np.float32)
        state[:, 0:3], state[:, 6], state[:, 7:10] = position, 1.0, linvel
        self.H.set(state=state)
        self.H.B.env_index_base = env_index_base
        self.pc = T(pc)
        self.shifted = torch.zeros(self.pc.numel() + 1, device=DEV)[1:].view_as(self.pc)  # the same cloud 4 bytes off a 16-byte boundary
        self.shifted.copy_(self.pc)
        assert self.pc.data_ptr() % 16 == 0 and self.shifted.data_ptr() % 16 == 4
        self.ttc, self.ds = Guarded(self.n), Guarded(self.n * self.cells, pad=self.cells)

    def __call__(self, noise=(None,) * 5, low_row0=10, device_noise=0, seed=0, step=0, shifted=False):
        p, H = self._lib.dptr, self.H
        H.B.rng_seed, H.B.step_counter = seed, step
        self.ttc.full.fill_(CANARY)
        self.ds.full.fill_(CANARY)
        keep = [None if a is None else T(np.asarray(a, np.float32).reshape(self.n, self.cells)) for a in noise]
        self._lib.check(H.lib.agx_lidar_image_obs(H.B, self.n, self.Hh, self.W, self.ph, self.pw, low_row0, p(self.shifted if shifted else self.pc),
                                                  *[p(t) for t in keep], device_noise, self.ttc.ptr(), self.ds.ptr(), H.stream()),
                        "agx_lidar_image_obs")
        torch.cuda.synchronize()
        return self.ttc.read(), self.ds.read().reshape(self.n, self.cells)


def equal(a, b):
    return all(same(x, y) for x, y in zip(a, b))


def half_masks(rng, n, cells):
    """the five tensors with every mask set (exactly 1) in half of the cells; the other half holds 0, 0.5 and 2: not set"""
    mask = lambda: rng.choice(np.array([1.0, 0.0, 0.5, 2.0], np.float32), size=(n, cells), p=[0.5, 0.25, 0.125, 0.125])  # noqa: E731
    return (mask(), (rng.random((n, cells)) * 9.8 + 0.2).astype(np.float32), mask(), mask(), (rng.random((n, cells)) * 0.8 + 0.2).astype(np.float32))


def check_rules(ds, clean_ds, masks, ow, low_row0):
    """what the three rules mean, on top of the bit comparison: a later rule wins"""
    nm, nv, mm, lm, lv = masks
    low = (lm == 1) & (np.arange(ds.shape[1])[None, :] // ow >= low_row0)
    assert same(ds[low], F(1.0) / lv[low])
    assert (ds[(mm == 1) & ~low] == F(0.1)).all()
    rest = ~low & (mm != 1)
    assert same(ds[rest & (nm != 1)], clean_ds[rest & (nm != 1)]) and (ds[rest & (nm == 1)] < clean_ds[rest & (nm == 1)]).all()


@pytest.mark.parametrize("H,W", [(3, 6), (6, 12), (9, 18), (7, 13), (12, 12)])
def test_lidar_image_obs_at_its_limits(orc, H, W):
    """the radar test's limit clouds ((3, 6): one cell; (6, 12): the 16-byte path; (9, 18): no multiple of 4 points -- the 4-byte path;
    (7, 13): remainder rows and columns dropped) and (12, 12): four pooled rows, so that the low-value rule starts at the first row,
    at the last and past it.  Masks at half density: the three rules overlap, the order is noise, max, low."""
    n = 5
    rng = np.random.default_rng(100 * H + W)
    pc, pos, vel = limit_clouds(rng, n, H, W)
    run = ImageRun(pc, pos, vel)
    oh, ow, cells = H // 3, W // 6, (H // 3) * (W // 6)
    assert run.cells == cells == {(3, 6): 1, (6, 12): 4, (9, 18): 9, (7, 13): 4, (12, 12): 8}[(H, W)]
    vec4 = (H * W) % 4 == 0
    assert vec4 == ((H, W) in ((6, 12), (12, 12)))
    clean = run()
    assert equal(clean, L.image_obs(orc, pc, pos, vel)) and equal(clean, orc.lidar_image_obs(pc, pos, vel))
    assert equal(run(shifted=True), clean)  # the 4-byte loads: same bits
    assert clean[0][0] < 10.0 and clean[0][1] == 10.0 and clean[0][2] == 10.0  # approaching; receding from every point; at rest
    assert clean[1].min() >= F(0.1) and clean[1].max() <= 5.0
    masks = half_masks(rng, n, cells)
    none = (None,) * 5
    for r0 in sorted({0, oh - 1, oh}):
        want = L.image_obs(orc, pc, pos, vel, *masks, low_row0=r0)
        got = run(masks, low_row0=r0)
        assert equal(got, want) and same(got[0], clean[0]), r0
        assert equal(got, orc.lidar_image_obs(pc, pos, vel, low_row0=r0, **dict(zip(("noise_mask", "noise_val", "max_mask", "low_mask", "low_val"),
                                                                                     [a.reshape(n, oh, ow) for a in masks])))), r0
        check_rules(got[1], clean[1], masks, ow, r0)
        assert equal(run(masks, low_row0=r0, shifted=True), got), r0
        # each rule alone: a NULL pointer means no such mask
        for alone in ((0, 1), (2,), (3, 4)):
            some = tuple(masks[k] if k in alone else None for k in range(5))
            assert equal(run(some, low_row0=r0), L.image_obs(orc, pc, pos, vel, *some, low_row0=r0)), (r0, alone)
        # the device generator at another step, another seed and a non-zero env_index_base
        seed, step, b = 4242 + r0, 11 + H, 3
        dev = run(none, low_row0=r0, device_noise=1, seed=seed, step=step)
        drawn = L.device_noise(orc, seed, np.full(n, step), cells, ow, r0)
        assert equal(dev, L.image_obs(orc, pc, pos, vel, *drawn, low_row0=r0)), r0
        assert equal(run(none, low_row0=r0, device_noise=1, seed=seed, step=step, shifted=True), dev)
        based = ImageRun(pc[b:], pos[b:], vel[b:], env_index_base=b)(none, low_row0=r0, device_noise=1, seed=seed, step=step)
        assert equal(based, (dev[0][b:], dev[1][b:])), r0
    if cells == 8:  # the rules do meet, in cells of every pooled row
        nm, mm, lm = masks[0] == 1, masks[2] == 1, masks[3] == 1
        assert (nm & mm & lm).any() and (nm & mm & ~lm).any() and (mm & lm).any() and (nm & lm & ~mm).any() and (masks[0] == 2).any()
        assert lm[:, 0:2].any() and lm[:, 6:8].any()


def test_lidar_image_obs_golden_cloud_every_low_row(orc):
    """48 x 120, six envs, 1920 cells: masks at half density and the device generator with the low-value rule starting at the first
    pooled row, around the task's row 10, at the last row and past it"""
    g = load_golden("lidar_image_obs", CR)
    pc, pos, vel = np.ascontiguousarray(g["pointcloud"][:, 0]), g["robot_position"], g["robot_linvel"]
    n, ow, cells = 6, 20, 320
    run = ImageRun(pc, pos, vel)
    clean = run()
    assert same(clean[0], g["clean_ttc"]) and same(clean[1], g["clean_ds"])  # the reference's own numbers
    masks = half_masks(np.random.default_rng(48120), n, cells)
    lows = {}
    for r0 in (0, 9, 10, 11, 15, 16):
        got = run(masks, low_row0=r0)
        assert equal(got, L.image_obs(orc, pc, pos, vel, *masks, low_row0=r0)), r0
        check_rules(got[1], clean[1], masks, ow, r0)
        dev = run(low_row0=r0, device_noise=1, seed=31337, step=140)
        drawn = L.device_noise(orc, 31337, np.full(n, 140), cells, ow, r0)
        assert equal(dev, L.image_obs(orc, pc, pos, vel, *drawn, low_row0=r0)), r0
        assert equal(run(low_row0=r0, device_noise=1, seed=31337, step=140, shifted=True), dev), r0
        lows[r0] = int(drawn[3].sum())
    assert lows[16] == 0 and lows[0] > lows[10] > lows[15] > 0 and lows[9] > lows[10] > lows[11]  # one pooled row more or less shows


def test_lidar_image_obs_reads_a_ray_that_hit_nothing_as_max_range(orc):
    """the LiDAR ray-cast writes sensor position + kNoHitRay x direction for a ray that hits nothing; such a point reads 10 m"""
    src = open(os.path.join(ROOT, "aerial_gym_simulator_amd", "csrc", "agx_raycast.hip")).read()
    no_hit = F(re.search(r"constexpr float kNoHitRay = ([0-9.]+)f;", src).group(1))
    assert no_hit == 1000.0
    rng = np.random.default_rng(6)
    n, H, W = 3, 6, 12
    pos = ((rng.random((n, 3)) - 0.5) * 4).astype(np.float32)
    dirs = rng.standard_normal((n, H, W, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    ranges = (rng.random((n, H, W)) * 8 + 0.5).astype(np.float32)
    ranges[:, 0:3, 0:6] = no_hit  # the first pooled cell: misses only
    ranges[0] = no_hit            # env 0: nothing in sight
    pc = np.ascontiguousarray((pos[:, None, None, :] + dirs * ranges[..., None]).astype(np.float32))
    vel = np.ones((n, 3), np.float32)
    run = ImageRun(pc, pos, vel)
    got = run()
    assert equal(got, L.image_obs(orc, pc, pos, vel)) and equal(run(shifted=True), got)
    assert (got[1][:, 0] == F(0.1)).all() and (got[1][0] == F(0.1)).all() and (got[1][1:, 1:] > F(0.1)).all()


def test_lidar_image_obs_argument_checks():
    from aerial_gym_simulator_amd import _lib

    run = ImageRun(np.zeros((1, 3, 6, 3), np.float32), np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32))
    H, p = run.H, _lib.dptr
    mask = torch.zeros(1, 1, device=DEV)
    no = (None,) * 5
    bad = [
        (1, 0, 6, 3, 6, p(run.pc), no),                               # no rows
        (1, 3, 6, 4, 6, p(run.pc), no),                               # a pool taller than the image
        (1, 3, 6, 3, 7, p(run.pc), no),                               # ... and wider
        (1, 3, 6, 3, 6, None, no),                                    # no cloud
        (1, 3, 6, 3, 6, p(run.pc), (p(mask), None, None, None, None)),  # a noise mask without its values
        (1, 3, 6, 3, 6, p(run.pc), (None, None, None, p(mask), None)),  # a low mask without its values
        (1, 128, 128, 3, 6, p(run.pc), no),                           # 64 KiB + 16 bytes of ranges
        (0, 3, 6, 3, 6, p(run.pc), no),
    ]
    for n, h, w, ph, pw, pc, noise in bad:
        code = H.lib.agx_lidar_image_obs(H.B, n, h, w, ph, pw, 0, pc, *noise, 0, run.ttc.ptr(), run.ds.ptr(), H.stream())
        assert code != 0, (n, h, w, ph, pw)
    torch.cuda.synchronize()
    assert run.ds.untouched() and run.ttc.untouched()  # nothing was launched
    # values without their mask are allowed and change nothing
    assert equal(run((None, np.ones((1, 1)), None, None, np.ones((1, 1))), low_row0=0), run())


def test_lidar_device_noise_statistics():
    """n = 64 (20480 cells, 7680 of them in the pooled rows >= 10), every point at a range of exactly 5 m: a cell reads 1 / (0.8 u +
    0.2) > 1 (low value), 1 / 10 (max range), 1 / (5 + 9.8 u + 0.2) in [1 / 15, 1 / 5.2] (noise) or 1 / 5.  Each rule's share among the
    cells no later rule overwrote is its probability (the draws are independent) within five binomial standard deviations."""
    n, H, W, r0, ow = 64, 48, 120, 10, 20
    pts = np.array([[5, 0, 0], [-5, 0, 0], [0, 5, 0], [0, -5, 0], [0, 0, 5], [0, 0, -5], [3, 4, 0], [0, -3, 4], [4, 0, -3]], np.float32)
    rng = np.random.default_rng(5)
    pc = np.ascontiguousarray(pts[rng.integers(0, len(pts), (n, H, W))])
    run = ImageRun(pc, np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32))
    ttc, ds = run(low_row0=r0, device_noise=1, seed=20261020, step=3)
    assert ds.size == 20480 and (ttc == 10.0).all()
    plain, at_max, low = ds == F(1.0) / F(5.0), ds == F(0.1), ds > 1.0
    noisy = ~plain & ~at_max & ~low
    assert (ds[noisy] >= F(1.0) / F(15.0)).all() and (ds[noisy] <= F(1.0) / (F(5.0) + F(0.2))).all() and (ds[low] <= 5.0).all()
    low_rows = np.broadcast_to(np.arange(320)[None, :] // ow >= r0, ds.shape)
    assert not low[~low_rows].any() and low_rows.sum() == 7680
    sd = lambda p, count: np.sqrt(p * (1 - p) / count)  # noqa: E731
    shares = []
    for name, p, hits, among in (("low value, rows >= 10", 0.02, low, low_rows), ("max range", 0.02, at_max, ~low), ("noise", 0.03, noisy, ~low & ~at_max)):
        share, count = hits.sum() / among.sum(), int(among.sum())
        shares.append((name, share, count, 5 * sd(p, count)))
        print("lidar device noise: %s: share %.5f of %d cells (expected %.2f +- %.5f)" % (name, share, count, p, 5 * sd(p, count)))
    for name, share, count, bound in shares:
        assert abs(share - {"low value, rows >= 10": 0.02, "max range": 0.02, "noise": 0.03}[name]) <= bound, (name, share, count)
