"""Test helper: inputs, expected values and C-ABI callers for the obstacle kernels (agx_reset_assets, agx_scene_reset_refresh,
agx_assets_integrate, agx_prims_from_assets, agx_boxes_from_assets, agx_scene_transform).  Expected values come from the CPU
oracle (oracle/oracle.py); what the oracle has no function for (the SoA box layout, the env bounds from their draws) is restated
in numpy float32 with one rounding per operation.  Used by tests/test_gpu_obstacle_limits.py and tests/test_edge_cases.py."""
import numpy as np

DEV = "cuda:0"
PARKED = np.float32(-1000.0)  # asset_manager.py:71
SEL_THRESHOLD = np.float32(0.15)  # the device generator's bernoulli(0.15) of env_manager.py:283-295
BOUNDS_CFG = ([-2.0, -4.0, -3.0], [-1.0, -2.5, -2.0], [9.0, 2.5, 2.0], [10.0, 4.0, 3.0])  # lower min / max, upper min / max
RADIUS_FACTOR = np.float32(1.000001)  # box_from_asset: the bounding radius is rounded up by this much


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits_equal(a, b):
    """np.array_equal on the float32 bit patterns: the sign of a zero and the payload of an int kept in a float count"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def sentinel(shape, start=3.0):
    """distinct finite float32 values, negative and off the values any of the kernels writes: -(start + i / 4), exact in float32"""
    size = int(np.prod(shape))
    assert start + size / 4 < 2 ** 22  # i / 4 is exact below 2^22: every element differs from every other
    return (-(start + 0.25 * np.arange(size, dtype=np.float64))).astype(np.float32).reshape(shape)


def T(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def masks_for(n, rng):
    """name -> uint8 [n]: none, only the last env, all, random (with a set and a clear env where n allows both)"""
    rnd = (rng.random(n) < 0.5).astype(np.uint8)
    if n > 1:
        rnd[rng.integers(n)] = 1
        rnd[(int(np.flatnonzero(rnd)[0]) + 1) % n] = 0
    last = np.zeros(n, np.uint8)
    last[-1] = 1
    return {"none": np.zeros(n, np.uint8), "last": last, "all": np.ones(n, np.uint8), "random": rnd}


def random_ratio_ranges(rng, n, K):
    """min / max state ratios [n,K,13] that differ between assets and envs: position ratios inside [0, 1], Euler ranges over
    +-pi for even assets and over [0, 2 pi) for odd ones, every seventh asset with min == max"""
    lo, hi = np.zeros((n, K, 13), np.float32), np.zeros((n, K, 13), np.float32)
    lo[..., :3] = rng.uniform(0.0, 0.5, (n, K, 3))
    hi[..., :3] = lo[..., :3] + rng.uniform(0.0, 0.5, (n, K, 3)).astype(np.float32)
    lo[:, 0::2, 3:6], hi[:, 0::2, 3:6] = -np.pi, np.pi
    lo[:, 1::2, 3:6], hi[:, 1::2, 3:6] = 0.0, 2.0 * np.pi
    lo[..., 3:6] *= rng.uniform(0.5, 1.0, (n, K, 3)).astype(np.float32)
    hi[..., 3:6] *= rng.uniform(0.5, 1.0, (n, K, 3)).astype(np.float32)
    hi[:, 6::7] = lo[:, 6::7]
    return lo, hi


def env_bounds(ub):
    """the env bounds of the reset from their six draws (bounds_from_draws): float32, one rounding per operation"""
    c = [np.array(x, np.float32) for x in BOUNDS_CFG]
    ub = np.asarray(ub, np.float32)
    return (c[1] - c[0]) * ub[:, :3] + c[0], (c[3] - c[2]) * ub[:, 3:] + c[2]


def device_draws(orc, seed, episodes, base, K):
    """(ub [n,6], usel [n], u [n,K,13]) of the device generator for envs base .. base + n - 1 in their episodes[i]-th reset.
    orc.rng_fill keys a row by its index: the rows below `base` are drawn as well and dropped."""
    ep = np.concatenate([np.zeros(base, np.int32), np.asarray(episodes, np.int32)])
    ub = orc.rng_fill(seed, ep, orc.RNG_BOUNDS, 6)[base:]
    usel = orc.rng_fill(seed, ep, orc.RNG_ASSET_SEL, 1)[base:, 0]
    u = np.stack([orc.rng_fill(seed, ep, orc.RNG_ASSETS + a, 6)[base:] for a in range(K)], axis=1)
    return ub, usel, np.concatenate([u, np.zeros(u.shape[:2] + (7,), np.float32)], axis=2)


def episodes_with_both_outcomes(orc, seed, n, base=0):
    """non-zero, distinct episode counts such that the device generator's `sel` is true for even envs and false for odd ones"""
    ep = np.zeros(n, np.int32)
    for i in range(n):
        for c in range(1 + 400 * i, 400 * (i + 1)):  # ranges that do not overlap: distinct between envs
            usel = orc.rng_fill(seed, np.full(base + i + 1, c, np.int32), orc.RNG_ASSET_SEL, 1)[-1, 0]  # (rows are keyed by index)
            if (usel < SEL_THRESHOLD) == (i % 2 == 0):
                ep[i] = c
                break
        assert ep[i] != 0, "no episode count with the wanted outcome"
    return ep


class ResetCase:
    """One agx_reset_assets call: its draws (host tensors or the device generator), the oracle's expected asset_state and the
    C-ABI call.  `init` is the asset buffer before the call (a sentinel pattern unless given)."""

    def __init__(self, orc, n, K, mask, lo, hi, num_obstacles, num_keep, device_rng, rng, seed=0xDEADBEEF12345, episodes=None,
                 base=0, sel=None, init=None):
        self.orc, self.n, self.K, self.device_rng, self.seed, self.base = orc, n, K, device_rng, seed, base
        self.mask = np.ascontiguousarray(mask, np.uint8)
        self.lo, self.hi, self.num_obstacles, self.num_keep = lo, hi, int(num_obstacles), int(num_keep)
        # per-env episode counts: non-zero and distinct
        self.episodes = (1 + rng.permutation(4 * n)[:n]).astype(np.int32) if episodes is None else np.asarray(episodes, np.int32)
        assert (self.episodes != 0).all() and len(np.unique(self.episodes)) == n
        if device_rng:
            self.ub, usel, self.u = device_draws(orc, seed, self.episodes, base, K)
            self.sel = usel < SEL_THRESHOLD
            self.u1 = self.u2 = None
        else:
            self.ub = rng.random((n, 6)).astype(np.float32)
            self.sel = (rng.random(n) < 0.5) if sel is None else np.asarray(sel, bool)
            self.u1, self.u2 = rng.random((n, K, 13)).astype(np.float32), rng.random((n, K, 13)).astype(np.float32)
            self.u = np.where(self.sel[:, None, None], self.u2, self.u1)
        self.bmin, self.bmax = env_bounds(self.ub)
        self.init = sentinel((n, K, 13)) if init is None else init
        self.ref = self.init.copy()
        orc.reset_assets(self.mask, self.u, self.sel.astype(np.uint8), lo, hi, self.bmin, self.bmax, self.num_obstacles, self.num_keep,
                         self.ref)

    def ratio(self):
        """the sampled state ratios [n,K,6] (float32, one rounding per operation)"""
        return (self.hi[..., :6] - self.lo[..., :6]) * self.u[..., :6] + self.lo[..., :6]

    def n_active(self):
        """the active-count rule, per env"""
        half, full = max(self.num_obstacles // 2, self.num_keep // 2), max(self.num_obstacles, self.num_keep)
        return np.where(self.sel, half, full)

    def buffers(self, parity=0, flag=None):
        """(AgxEnvBuffers, AgxResetArgs, tensors to keep alive): this parity's flag word 1, the other one 0, unless `flag` is given"""
        import torch

        from aerial_gym_simulator_amd import _lib

        B, R = _lib.AgxEnvBuffers(), _lib.AgxResetArgs()
        words = [0, 0]
        words[parity] = 1
        keep = dict(mask=T(self.mask), flag=torch.tensor(words if flag is None else flag, dtype=torch.int32, device=DEV),
                    ep=T(self.episodes))
        B.reset_mask, B.reset_flag, B.flag_parity = _lib.dptr(keep["mask"]), _lib.dptr(keep["flag"]), parity
        B.episode_count, B.env_index_base = _lib.dptr(keep["ep"]), self.base
        for i in range(3):
            R.lower_bound_min[i], R.lower_bound_max[i] = BOUNDS_CFG[0][i], BOUNDS_CFG[1][i]
            R.upper_bound_min[i], R.upper_bound_max[i] = BOUNDS_CFG[2][i], BOUNDS_CFG[3][i]
        R.seed = self.seed
        if not self.device_rng:
            keep.update(ulo=T(self.ub[:, :3]), uhi=T(self.ub[:, 3:]), ustate=torch.zeros(self.n, 13, device=DEV), u1=T(self.u1),
                        u2=T(self.u2), usel=T(self.sel.astype(np.float32)))
            R.u_bounds_lo, R.u_bounds_hi, R.u_state = _lib.dptr(keep["ulo"]), _lib.dptr(keep["uhi"]), _lib.dptr(keep["ustate"])
        keep.update(lo=T(self.lo), hi=T(self.hi))
        return B, R, keep

    def run(self, parity=0, flag=None):
        """agx_reset_assets -> (asset_state after, episode_count after)"""
        import torch

        from aerial_gym_simulator_amd import _lib

        B, R, keep = self.buffers(parity, flag)
        st = T(self.init)
        d = _lib.dptr
        draws = (None, None, None) if self.device_rng else (d(keep["u1"]), d(keep["u2"]), d(keep["usel"]))
        _lib.check(_lib.load().agx_reset_assets(B, self.n, self.K, R, *draws, d(keep["lo"]), d(keep["hi"]), self.num_obstacles,
                                                self.num_keep, d(st), _lib.current_stream(DEV)), "agx_reset_assets")
        torch.cuda.synchronize()
        return st.cpu().numpy(), keep["ep"].cpu().numpy()


def boxes_soa_ref(asset_state, half, init=None, mask=None):
    """the collision boxes agx_boxes_from_assets writes, [K][11][n]: rows 0..6 the pose, 7..9 the half extents, 10 the bounding
    radius sqrt((h0 h0 + h1 h1) + h2 h2) * 1.000001 in float32 with one rounding per operation; masked-out envs keep `init`"""
    n, K = asset_state.shape[:2]
    h = np.asarray(half, np.float32)
    out = np.zeros((K, 11, n), np.float32)
    out[:, 0:7] = np.transpose(asset_state[..., 0:7], (1, 2, 0))
    out[:, 7:10] = np.transpose(h, (1, 2, 0))
    radius = np.sqrt((h[..., 0] * h[..., 0] + h[..., 1] * h[..., 1]) + h[..., 2] * h[..., 2]) * RADIUS_FACTOR
    assert radius.dtype == np.float32
    out[:, 10] = radius.T
    if mask is not None:
        keep = ~np.asarray(mask, bool)
        out[:, :, keep] = init[:, :, keep]
    return out


def mixed_quats(rng, shape):
    """quaternions (x, y, z, w) of norm 1, 2 and 1e-3 over all of SO(3), every fifth one the identity"""
    from scene_util import random_quats

    q = random_quats(rng, shape).reshape(-1, 4)
    q *= np.float32([1.0, 2.0, 1.0e-3])[np.arange(len(q)) % 3][:, None]
    q[::5] = np.float32([0.0, 0.0, 0.0, 1.0])
    return np.ascontiguousarray(q.reshape(tuple(np.atleast_1d(shape)) + (4,)), np.float32)


def random_asset_state(rng, n, K):
    """[n,K,13]: positions in +-10 m, mixed_quats, random twists"""
    st = rng.uniform(-10.0, 10.0, (n, K, 13)).astype(np.float32)
    st[..., 3:7] = mixed_quats(rng, (n, K))
    return st


def run_scene_transform(tri_local, tri_asset, asset_state, mask, init):
    import torch

    from aerial_gym_simulator_amd import _lib

    n, nt = tri_local.shape[:2]
    d = _lib.dptr
    t = [T(tri_local), T(np.asarray(tri_asset, np.int32)), T(asset_state), T(mask) if mask is not None else None, T(init)]
    _lib.check(_lib.load().agx_scene_transform(n, nt, asset_state.shape[1], d(t[0]), d(t[1]), d(t[2]), d(t[3]), d(t[4]),
                                               _lib.current_stream(DEV)), "agx_scene_transform")
    torch.cuda.synchronize()
    return t[4].cpu().numpy()
