"""GPU: agx_imu_update / agx_imu_reset through the C ABI against the CPU oracle (orc.imu_update, orc.imu_reset) and the restated
Philox streams (orc.rng_fill, imu_ref.py), where tests/test_gpu_imu.py does not look: a partial 256-thread block (n = 300) and a
single env, the k-fold of the bias walk, the enable switches, every clamp on both sides, a tilted gravity and gravity_compensation,
masked resets at both flag parities, and both kernels' device generators bit by bit.

Gates: 1e-5 (measurement) and 1e-6 (bias, mount quaternion) in conftest.rel_err, the gates of test_gpu_imu.py's chain test; the
normals of the device generator within imu_ref.Z_TOL of their float64 restatement, a bound put together there from its terms."""
import numpy as np
import pytest
import torch
from conftest import golden_params, load_golden, rel_err
from imu_ref import SQRT_DT, Z_MAX, Z_TOL, imu_args, reset_draws, sensor_force, slot_normals, update_normals

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [300, 1]  # a full 256-thread block and a partial one; one env
GRAVITY = (0.0, 0.0, -9.81)
TILTED = (1.3, -2.1, -9.0)
MAX_SUBSTEPS = 32  # AGX_MAX_SUBSTEPS
# The sensor's limits are the reference's (BaseImuConfig: 100 m/s^2, 10 rad/s); densities, initial bias and mount range differ from
# channel to channel, so that a swapped index shows, and are large enough for the gates to see them: with the reference's
# bias_std (1e-6, 2.7e-5) one increment of the walk, bias_std * sqrt_dt * z, is below the 1e-6 gate on the bias.
CFG = dict(bias_std=np.float32([0.02, 0.03, 0.04, 0.05, 0.06, 0.07]), noise_std=np.float32([0.01, 0.02, 0.03, 0.04, 0.05, 0.06]),
           max_value=np.float32([100, 100, 100, 10, 10, 10]), max_bias_init=np.float32([0.1, 0.2, 0.3, 0.4, 0.5, 0.6]),
           min_rot_deg=np.float32([-2, -3, -1]), max_rot_deg=np.float32([2, 1, 4]))


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def unit_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


class Imu:
    """a DynHarness with the IMU's own tensors; inputs and results as reference-layout numpy arrays"""

    def __init__(self, n, seed=0):
        from aerial_gym_simulator_amd import _lib
        from gpu_harness import DynHarness

        self.n, self.lib_mod = n, _lib
        self.H = DynHarness(golden_params(load_golden("step_quad_velocity")), n)
        self.cfg, self.mass = CFG, 1.24
        self.bias, self.sq, self.meas = torch.zeros(n, 6, device=DEV), torch.zeros(n, 4, device=DEV), torch.zeros(n, 6, device=DEV)
        self.body_force = torch.zeros(3, n, device=DEV)
        self.H.B.body_force = _lib.dptr(self.body_force)
        self.H.B.rng_seed = seed

    def args(self, world_frame, **kw):
        return imu_args(self.cfg, self.mass, world_frame, **kw)

    def motion(self, quat, wbody, body_force):
        n = self.n
        state, derived = np.zeros((n, 13), np.float32), np.zeros((n, 16), np.float32)
        state[:, 3:7], derived[:, 13:16] = quat, wbody
        self.H.set(state=state, derived=derived)
        self.body_force.copy_(T(np.asarray(body_force, np.float32).T))

    def update(self, A, k, sensor_quat, bias, z_noise=None, z_bias=None, step=0):
        """one agx_imu_update call -> (measurement, bias after); z_noise [n, 6] and z_bias [k, n, 6], or neither: the device generator"""
        p, H = self.lib_mod.dptr, self.H
        self.sq.copy_(T(sensor_quat))
        self.bias.copy_(T(bias))
        self.meas.fill_(777.0)
        H.B.step_counter = step
        zn = T(z_noise) if z_noise is not None else None
        zb = T(z_bias) if z_bias is not None else None
        assert zb is None or tuple(zb.shape) == (k, self.n, 6) or k == 0
        self.lib_mod.check(H.lib.agx_imu_update(H.B, self.n, k, A, p(self.sq), p(zn) if zn is not None else None,
                                                p(zb) if zb is not None else None, p(self.bias), p(self.meas), H.stream()), "agx_imu_update")
        torch.cuda.synchronize()
        return self.meas.cpu().numpy(), self.bias.cpu().numpy()

    def reset(self, A, mask, bias, sensor_quat, u_bias=None, u_rot=None, parity=0, flags=None, episodes=None, env_base=0):
        """one agx_imu_reset call -> (bias, mount quaternions); u_bias / u_rot or neither: the device generator"""
        p, H = self.lib_mod.dptr, self.H
        self.bias.copy_(T(bias))
        self.sq.copy_(T(sensor_quat))
        H.reset_mask.copy_(torch.from_numpy(np.ascontiguousarray(mask, np.uint8)))
        fl = [0, 0]
        fl[parity] = 1
        H.reset_flag.copy_(torch.tensor(fl if flags is None else flags, dtype=torch.int32))
        H.B.flag_parity, H.B.env_index_base = parity, env_base
        if episodes is not None:
            H.episode_count.copy_(torch.from_numpy(np.ascontiguousarray(episodes, np.int32)))
        ub, ur = (T(u_bias), T(u_rot)) if u_bias is not None else (None, None)
        self.lib_mod.check(H.lib.agx_imu_reset(H.B, self.n, A, p(ub) if ub is not None else None, p(ur) if ur is not None else None,
                                               p(self.bias), p(self.sq), H.stream()), "agx_imu_reset")
        torch.cuda.synchronize()
        H.B.flag_parity, H.B.env_index_base = 0, 0
        return self.bias.cpu().numpy(), self.sq.cpu().numpy()


def mounts(orc, cfg, rng, n):
    """mount quaternions inside the config's range, as a reset makes them"""
    bias, sq = np.zeros((n, 6), np.float32), np.zeros((n, 4), np.float32)
    orc.imu_reset(np.ones(n, np.uint8), rng.random((n, 6)), rng.random((n, 3)), cfg["max_bias_init"], np.deg2rad(cfg["min_rot_deg"]),
                  np.deg2rad(cfg["max_rot_deg"]), bias, sq)
    return bias, sq


def random_inputs(orc, I, rng):
    n = I.n
    bias0, sq = mounts(orc, I.cfg, rng, n)
    quat, wbody = unit_quats(rng, n), rng.normal(size=(n, 3)).astype(np.float32)
    body_force = (rng.normal(size=(n, 3)) * 6.0).astype(np.float32)
    I.motion(quat, wbody, body_force)
    return dict(quat=quat, wbody=wbody, body_force=body_force, sq=sq, bias0=bias0)


def oracle_update(orc, I, x, world_frame, k, z_noise, z_bias, *, gravity=GRAVITY, g_world=None, enable_noise=1, enable_bias=1):
    """k calls of orc.imu_update on the same inputs, the last call's measurement; k = 0: the measurement with the bias as it is.
    The force sensor's reading is body_force + m R^T gravity with the TRUE gravity; the oracle subtracts g_world."""
    cfg, g_world = I.cfg, gravity if g_world is None else g_world
    force = sensor_force(x["body_force"], I.mass, x["quat"], gravity)
    bias = x["bias0"].copy()
    for s in range(max(k, 1)):
        zb = z_bias[s] if k > 0 else np.zeros((I.n, 6), np.float32)
        meas = orc.imu_update(I.mass, np.float32(g_world), SQRT_DT, world_frame, enable_noise, enable_bias, cfg["bias_std"], cfg["noise_std"],
                              cfg["max_value"], force, x["quat"], x["wbody"], x["sq"], z_noise, zb, bias)
    return meas, bias


# ---------------------------------------------------------------------------------------------------------------- the k-fold
@pytest.mark.parametrize("frame", ["body", "world"])
@pytest.mark.parametrize("k", [0, 1, 2, 10, MAX_SUBSTEPS])
@pytest.mark.parametrize("n", SIZES)
def test_k_substeps_in_one_call_equal_k_oracle_updates(orc, n, k, frame):
    """k bias increments and the last sub-step's noise; k = 0 leaves the bias bit for bit"""
    rng = np.random.default_rng(1000 * n + 10 * k + (frame == "world"))
    I = Imu(n)
    x = random_inputs(orc, I, rng)
    zn = rng.normal(size=(n, 6)).astype(np.float32)
    zb = rng.normal(size=(max(k, 1), n, 6)).astype(np.float32)
    got, bias = I.update(I.args(frame == "world"), k, x["sq"], x["bias0"], zn, zb)
    ref, ref_bias = oracle_update(orc, I, x, frame == "world", k, zn, zb)
    assert rel_err(got, ref) < 1e-5
    assert rel_err(bias, ref_bias) < 1e-6
    if k == 0:
        assert np.array_equal(bias.view(np.uint32), x["bias0"].view(np.uint32))
    else:
        assert np.abs(bias - x["bias0"]).min(axis=0).max() > 0 and np.abs(bias - x["bias0"]).max() > 1e-3  # and it walked


# ---------------------------------------------------------------------------------------------------------------- switches
@pytest.mark.parametrize("n", SIZES)
def test_enable_switches(orc, n):
    """the four (enable_bias, enable_noise) pairs against the oracle; both off = a run fed all-zero normals, bit for bit, measured
    from the bias-free, noise-free signal; the bias walks on whatever enable_bias says (the reference calls update_bias regardless)"""
    rng = np.random.default_rng(2000 + n)
    I = Imu(n)
    x = random_inputs(orc, I, rng)
    k = 3
    zn, zb = rng.normal(size=(n, 6)).astype(np.float32), rng.normal(size=(k, n, 6)).astype(np.float32)
    out = {}
    for eb in (0, 1):
        for en in (0, 1):
            got, bias = I.update(I.args(False, enable_bias=eb, enable_noise=en), k, x["sq"], x["bias0"], zn, zb)
            ref, ref_bias = oracle_update(orc, I, x, False, k, zn, zb, enable_bias=eb, enable_noise=en)
            assert rel_err(got, ref) < 1e-5, (eb, en)
            assert rel_err(bias, ref_bias) < 1e-6 and not np.array_equal(bias, x["bias0"]), (eb, en)
            out[eb, en] = got, bias
    assert all(np.array_equal(out[key][1], out[1, 1][1]) for key in out)  # one bias walk, whatever the switches
    zeros = I.update(I.args(False, enable_bias=0, enable_noise=0), k, x["sq"], np.zeros((n, 6), np.float32), np.zeros((n, 6), np.float32),
                     np.zeros((k, n, 6), np.float32))
    assert np.array_equal(out[0, 0][0].view(np.uint32), zeros[0].view(np.uint32))
    assert rel_err(out[1, 0][0] - out[0, 0][0], out[1, 1][1]) < 1e-5        # the bias enters once, the walked one
    noise = zn.astype(np.float64) * I.cfg["noise_std"].astype(np.float64) / float(SQRT_DT)
    assert rel_err(out[0, 1][0] - out[0, 0][0], noise) < 1e-5               # ... and the noise density


# ---------------------------------------------------------------------------------------------------------------- saturation
@pytest.mark.parametrize("frame", ["body", "world"])
def test_every_channel_saturates_on_both_sides(orc, frame):
    """forces and body rates far past the limits, +-inf forces among them: a clamped entry is +-max_value exactly, and the oracle
    clamps each of the six channels on each side at least once.  (An infinite force passes the rotations as NaN; fminf / fmaxf
    and the oracle's comparisons both answer +max_value there.  NaN inputs themselves are left out: torch.min differs.)"""
    n = 300
    rng = np.random.default_rng(3000 + (frame == "world"))
    I = Imu(n)
    x = random_inputs(orc, I, rng)
    x["body_force"][:200] *= np.float32(60.0)  # |a| up to ~ 6 * 60 / 1.24 * 3 sigma: far past 100 m/s^2
    x["wbody"][:200] *= np.float32(25.0)       # past 10 rad/s
    x["body_force"][296, 0], x["body_force"][297, 1], x["body_force"][298, 2], x["body_force"][299] = np.inf, -np.inf, np.inf, -np.inf
    I.motion(x["quat"], x["wbody"], x["body_force"])
    zn, zb = rng.normal(size=(n, 6)).astype(np.float32), rng.normal(size=(1, n, 6)).astype(np.float32)
    got, _ = I.update(I.args(frame == "world"), 1, x["sq"], x["bias0"], zn, zb)
    ref, _ = oracle_update(orc, I, x, frame == "world", 1, zn, zb)
    mx = I.cfg["max_value"]
    hi, lo = ref == mx, ref == -mx
    assert hi.any(axis=0).all() and lo.any(axis=0).all(), (hi.sum(axis=0), lo.sum(axis=0))  # every (channel, sign), and on finite inputs:
    assert hi[:296].any(axis=0).all() and lo[:296].any(axis=0).all()
    assert np.isfinite(got).all() and (np.abs(got) <= mx).all()
    assert np.array_equal(got[hi], ref[hi]) and np.array_equal(got[lo], ref[lo])
    assert np.array_equal(np.abs(got[296:, :3]), np.broadcast_to(mx[:3], (4, 3)))
    free = ~(hi | lo)
    assert free.sum() > n and rel_err(got[free], ref[free]) < 1e-5


# ---------------------------------------------------------------------------------------------------------------- gravity
@pytest.mark.parametrize("frame", ["body", "world"])
@pytest.mark.parametrize("case", ["tilted", "gravity_compensation"])
@pytest.mark.parametrize("n", SIZES)
def test_gravity_vector_and_gravity_compensation(orc, n, case, frame):
    """a gravity that is not (0, 0, -9.81), and g_world = 0 (gravity_compensation = True): the force sensor's reading holds the
    true gravity either way, the sensor subtracts g_world.  A kernel that rebuilds the reading from g_world is off by |g| there."""
    rng = np.random.default_rng(4000 + n + (frame == "world"))
    I = Imu(n)
    x = random_inputs(orc, I, rng)
    g_world = TILTED if case == "tilted" else (0.0, 0.0, 0.0)
    zn, zb = rng.normal(size=(n, 6)).astype(np.float32), rng.normal(size=(2, n, 6)).astype(np.float32)
    got, bias = I.update(I.args(frame == "world", gravity=TILTED, g_world=g_world), 2, x["sq"], x["bias0"], zn, zb)
    ref, ref_bias = oracle_update(orc, I, x, frame == "world", 2, zn, zb, gravity=TILTED, g_world=g_world)
    print("max |measurement - oracle| on the accelerometer channels:", np.abs(got - ref)[:, :3].max())
    assert rel_err(got, ref) < 1e-5
    assert rel_err(bias, ref_bias) < 1e-6


def test_gravity_compensation_reads_zero_at_hover(orc):
    """known answer: thrust m g along body z, level, at rest, ideal sensor: +g along z without the flag, 0 with it"""
    I = Imu(1)
    quat, zero = np.float32([[0, 0, 0, 1]]), np.zeros((1, 6), np.float32)
    I.motion(quat, np.zeros((1, 3), np.float32), np.float32([[0, 0, I.mass * 9.81]]))
    for g_world, want in ((GRAVITY, 9.81), ((0.0, 0.0, 0.0), 0.0)):
        got, _ = I.update(I.args(False, g_world=g_world, enable_bias=0, enable_noise=0), 1, quat, zero, zero, zero[None])
        assert np.abs(got[0] - np.float32([0, 0, want, 0, 0, 0])).max() < 1e-5, (g_world, got)


def test_update_refuses_a_g_world_that_is_neither_zero_nor_the_gravity():
    """g_world = gravity * (1 - gravity_compensation): a caller that fills g_world and leaves `gravity` at zero (the struct before
    the field existed) is told so, before any launch"""
    I = Imu(1)
    quat, zero = np.float32([[0, 0, 0, 1]]), np.zeros((1, 6), np.float32)
    I.motion(quat, np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32))
    for gravity, g_world in (((0.0, 0.0, 0.0), GRAVITY), (GRAVITY, TILTED)):
        with pytest.raises(RuntimeError, match="g_world"):
            I.update(I.args(False, gravity=gravity, g_world=g_world), 1, quat, zero, zero, zero[None])
        assert (I.meas == 777.0).all()  # nothing ran


# ---------------------------------------------------------------------------------------------------------------- masked reset
@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("pattern", ["none", "last", "all", "random"])
def test_masked_reset(orc, pattern, parity):
    """draws handed in: the envs of the mask match orc.imu_reset, all others keep bias and mount quaternion bit for bit; with this
    parity's flag word clear and the other one set nothing changes at all"""
    n = 300
    rng = np.random.default_rng(5000 + parity)
    mask = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "random": rng.random(n) < 0.4}.get(pattern)
    if pattern == "last":
        mask = np.arange(n) == n - 1  # env 299: the partial block
    I = Imu(n)
    bias0, sq0 = (rng.normal(size=(n, 6)) * 0.3).astype(np.float32), unit_quats(rng, n)
    ub, ur = rng.random((n, 6)).astype(np.float32), rng.random((n, 3)).astype(np.float32)
    A = I.args(False)
    bias, sq = I.reset(A, mask, bias0, sq0, ub, ur, parity=parity)
    ref_bias, ref_sq = bias0.copy(), sq0.copy()
    orc.imu_reset(mask, ub, ur, I.cfg["max_bias_init"], np.deg2rad(I.cfg["min_rot_deg"]), np.deg2rad(I.cfg["max_rot_deg"]), ref_bias, ref_sq)
    assert np.array_equal(bias[~mask].view(np.uint32), bias0[~mask].view(np.uint32))
    assert np.array_equal(sq[~mask].view(np.uint32), sq0[~mask].view(np.uint32))
    assert rel_err(bias, ref_bias) < 1e-6 and rel_err(sq, ref_sq) < 1e-6
    if mask.any():
        assert not (bias[mask] == bias0[mask]).all(axis=1).any() and not (sq[mask] == sq0[mask]).all(axis=1).any()
    flags = [0, 0]
    flags[parity ^ 1] = 1
    bias, sq = I.reset(A, np.ones(n, bool), bias0, sq0, ub, ur, parity=parity, flags=flags)
    assert np.array_equal(bias.view(np.uint32), bias0.view(np.uint32)) and np.array_equal(sq.view(np.uint32), sq0.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- device generator
@pytest.mark.parametrize("n", SIZES)
def test_reset_device_generator_is_the_documented_stream(orc, n):
    """NULL draws == the same call fed orc.rng_fill(seed, episode_count, RNG_IMU_RESET, 9): columns 0-5 the bias, 6-8 the mount;
    with env_index_base = b the rows are rows b .. of an (n + b)-env run"""
    seed, base = 0x5EED0123456789AB, 41
    rng = np.random.default_rng(6000 + n)
    episodes = rng.integers(0, 1000, n + base).astype(np.int32)
    mask = np.ones(n + base, bool)
    mask[::7] = False
    big = Imu(n + base, seed)
    bias0, sq0 = (rng.normal(size=(n + base, 6)) * 0.3).astype(np.float32), unit_quats(rng, n + base)
    A = big.args(False)
    dev_bias, dev_sq = big.reset(A, mask, bias0, sq0, episodes=episodes)
    ub, ur = reset_draws(orc, seed, episodes)
    fed_bias, fed_sq = big.reset(A, mask, bias0, sq0, ub, ur, episodes=episodes)
    assert np.array_equal(dev_bias, fed_bias) and np.array_equal(dev_sq, fed_sq)
    assert np.array_equal(dev_bias[~mask], bias0[~mask]) and np.array_equal(dev_sq[~mask], sq0[~mask])
    assert np.array_equal(big.H.episode_count.cpu().numpy(), episodes)  # the IMU reset reads the episode, it does not count it
    small = Imu(n, seed)
    sm_bias, sm_sq = small.reset(A, mask[base:], bias0[base:], sq0[base:], episodes=episodes[base:], env_base=base)
    assert np.array_equal(sm_bias, dev_bias[base:]) and np.array_equal(sm_sq, dev_sq[base:])
    other = big.reset(A, mask, bias0, sq0, episodes=episodes + 1)[0]
    assert not np.array_equal(other[mask], dev_bias[mask])  # keyed by the episode


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("n", SIZES)
def test_update_device_generator_normals_are_the_documented_slots(orc, n, k):
    """The normals themselves.  noise_std = sqrt_dt = 1, bias off, no motion, no gravity, no clamp: the measurement IS the six noise
    normals of slot 2 (k - 1).  Noise off, bias_std = 1: the bias after one call is the sum of slots 2 s + 1 (times 1).  Both
    within imu_ref.Z_TOL of the float64 restatement -- |z| <= 5.77, the float32 angle, the correctly rounded sincos, 2 ulp on r,
    half an ulp on the product: 6.4e-6 -- the bias sum plus its k float32 additions."""
    seed, step = 0xABCDEF0123, 4321
    I = Imu(n, seed)
    cfg = dict(bias_std=np.ones(6), noise_std=np.ones(6), max_value=np.full(6, 1e30), max_bias_init=np.zeros(6), min_rot_deg=np.zeros(3),
               max_rot_deg=np.zeros(3))
    ident, zero = np.tile(np.float32([0, 0, 0, 1]), (n, 1)), np.zeros((n, 6), np.float32)
    I.motion(ident, np.zeros((n, 3)), np.zeros((n, 3)))
    zn, zb = update_normals(orc, seed, n, step, k)
    none = dict(gravity=(0.0, 0.0, 0.0), sqrt_dt=1.0)
    meas, _ = I.update(imu_args(cfg, 1.0, False, enable_bias=0, **none), k, ident, zero, step=step)
    err = np.abs(meas - zn).max()
    print("noise normals: max |device - float64| =", err, "bound", Z_TOL)
    assert err <= Z_TOL
    _, bias = I.update(imu_args(cfg, 1.0, False, enable_noise=0, **none), k, ident, zero, step=step)
    tol = k * Z_TOL + k * (k * Z_MAX) * 2.0 ** -24  # k normals, and k additions rounded at magnitudes up to k |z|max
    err = np.abs(bias - zb.sum(axis=0)).max()
    print("bias walk: max |device - float64| =", err, "bound", tol)
    assert err <= tol
    if n > 1:  # the restated normals are normals: the twelve-slot sample has unit spread and the slots differ
        z = slot_normals(orc, seed, n, step, 2 * k)
        assert abs(z.std() - 1.0) < 0.05 and abs(z.mean()) < 0.05 and np.abs(z).max() <= Z_MAX
        assert k == 1 or np.abs(z[:, 0] - z[:, 2]).max() > 1.0


@pytest.mark.parametrize("frame", ["body", "world"])
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("n", SIZES)
def test_update_device_generator_full_configuration(orc, n, k, frame):
    """a full configuration on the device generator == the same call fed the restated normals as float32, within the chain test's
    gates, rows of a run with env_index_base > 0 included; another step_counter gives other numbers"""
    seed, steps, base = 0x0123456789ABCDEF, (7, 8), 41
    rng = np.random.default_rng(7000 + n + k)
    I = Imu(n, seed)
    x = random_inputs(orc, I, rng)
    A = I.args(frame == "world")
    outs = []
    for step in steps:
        got, bias = I.update(A, k, x["sq"], x["bias0"], step=step)
        zn, zb = update_normals(orc, seed, n, step, k)
        fed, fed_bias = I.update(A, k, x["sq"], x["bias0"], zn.astype(np.float32), zb.astype(np.float32), step=step)
        assert rel_err(got, fed) < 1e-5 and rel_err(bias, fed_bias) < 1e-6, step
        outs.append((got, bias))
    assert not np.isclose(outs[0][0], outs[1][0]).all(axis=1).any()  # every env draws anew in the next step
    assert not (outs[0][1] == outs[1][1]).all(axis=1).any()
    I.H.B.env_index_base = base
    got, bias = I.update(A, k, x["sq"], x["bias0"], step=steps[0])
    I.H.B.env_index_base = 0
    zn, zb = update_normals(orc, seed, n, steps[0], k, env_base=base)
    fed, fed_bias = I.update(A, k, x["sq"], x["bias0"], zn.astype(np.float32), zb.astype(np.float32), step=steps[0])
    assert rel_err(got, fed) < 1e-5 and rel_err(bias, fed_bias) < 1e-6
    assert not np.isclose(got, outs[0][0]).all(axis=1).any()
