"""CPU: the host half of single-launch position steps (include/aerial_gym_hip.h, AgxPositionStepPlan.proof_*).

agx_step_proof_decide turns the record the kernels leave in mapped host memory into the form of the next step -- two launches,
ONE launch in which some env certainly resets (ANY), ONE launch in which none can (NONE) -- and is driven here with synthetic
records: seqlock and tag arithmetic, voided records, the horizon's ends, the "none" proof's limits.  agx_step_proof_witness_bit
is the device's rule for the horizon bits (the same __host__ __device__ function), and agx_step_proof_travel the bound both
proofs rest on: it must bound the displacement of the oracle's integrator driven at full thrust."""
import ctypes as C
import math

import numpy as np
import pytest

from aerial_gym_simulator_amd import _lib

TWO, ANY, NONE = 0, 1, 2
R = {name: i for i, name in enumerate(_lib.PROOF_REASONS)}
D = _lib.PROOF_HORIZON
M31 = 0x7FFFFFFF
DT, VMAX = 0.01, 100.0


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def f2u(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def record(tag, horizon=0, max_steps=0, dist=0.0, speed=0.0, reset=False, begin=None):
    r = np.zeros(_lib.PROOF_RECORD_WORDS, np.uint32)
    r[0], r[1], r[2], r[3], r[4], r[5] = tag, horizon, max_steps, f2u(dist), f2u(speed), 1 if reset else 0
    r[7] = tag if begin is None else begin
    return r


def decide(lib, rec, now, min_tag=1, L=500, roc=1, dv=0.46):
    q = _lib.AgxStepProofQuery(now_tag=now & M31, min_tag=min_tag & M31, episode_len=L, reset_on_collision=roc, dt=DT,
                               max_linear_velocity=VMAX, dv=dv)
    why = C.c_int32(-1)
    mode = lib.agx_step_proof_decide(rec.ctypes.data, C.byref(q), C.byref(why))
    return mode, _lib.PROOF_REASONS[why.value]


def test_no_record_torn_read_and_void(lib):
    assert decide(lib, record(0), 5) == (TWO, "no_record")
    assert decide(lib, record(10, horizon=1 << 2, begin=11), 12) == (TWO, "torn")  # a write in progress
    assert decide(lib, record(10, horizon=1 << 2, begin=9), 12) == (TWO, "torn")
    assert decide(lib, record(10, horizon=1 << 2), 12) == (ANY, "proved")
    # the host touched the state after step 9 (tag 10): min_tag 11 voids the record, min_tag 10 does not
    assert decide(lib, record(10, horizon=1 << 2), 12, min_tag=11) == (TWO, "void")
    assert decide(lib, record(10, horizon=1 << 2), 12, min_tag=10) == (ANY, "proved")
    assert decide(lib, record(10, max_steps=3), 12, min_tag=12) == (TWO, "void")
    assert lib.agx_step_proof_decide(None, None, None) == TWO


def test_tag_arithmetic(lib):
    # k = now - tag: a record of this very step or of a later one proves nothing; nor does one more than 64 steps old
    assert decide(lib, record(12, horizon=~0 & 0xFFFFFFFE), 12) == (TWO, "tag")
    assert decide(lib, record(13, horizon=~0 & 0xFFFFFFFE), 12) == (TWO, "tag")
    assert decide(lib, record(100, max_steps=1), 164, roc=0) == (NONE, "proved")
    assert decide(lib, record(100, max_steps=1), 165, roc=0) == (TWO, "tag")
    # 31-bit wrap-around: tag 2^31 - 2, now 2 -> k = 4
    tag = M31 - 1
    assert decide(lib, record(tag, horizon=1 << 4), 2, min_tag=tag) == (ANY, "proved")
    assert decide(lib, record(tag, horizon=1 << 3), 2, min_tag=tag) == (NONE, "proved")
    assert decide(lib, record(tag, horizon=1 << 4), 2, min_tag=1) == (TWO, "void")  # min_tag after the wrap: tag is older


def test_horizon_k1_kD_and_beyond(lib):
    t = 1000
    for k in (1, 2, D - 1, D):
        assert decide(lib, record(t, horizon=1 << k, reset=True), t + k) == (ANY, "proved"), k
        assert decide(lib, record(t, horizon=(~(1 << k)) & 0xFFFFFFFF, reset=True), t + k) == (TWO, "reset_no_witness"), k
    # k > D: no horizon bit can cover it, whatever the record says
    assert decide(lib, record(t, horizon=0xFFFFFFFF, reset=True), t + D + 1) == (TWO, "reset_no_witness")
    assert decide(lib, record(t, horizon=0xFFFFFFFF, max_steps=10), t + D + 1) == (NONE, "proved")
    # bit 0 is not a horizon (k = 0 is the recorded step itself)
    assert decide(lib, record(t, horizon=1, reset=True), t) == (TWO, "tag")


def test_none_proof_limits(lib):
    t, L = 50, 40
    # no truncation while max(sim_steps) + k <= L
    assert decide(lib, record(t, max_steps=30, dist=1.0, speed=1.0), t + 10, L=L) == (NONE, "proved")
    assert decide(lib, record(t, max_steps=30, dist=1.0, speed=1.0), t + 11, L=L) == (TWO, "may_truncate")
    # no crash while max dist + travel(k) < 8
    k = 5
    travel = lib.agx_step_proof_travel(k, 2.0, DT, VMAX, 0.46, 0)
    assert decide(lib, record(t, max_steps=1, dist=7.9 - travel, speed=2.0), t + k, L=L) == (NONE, "proved")
    assert decide(lib, record(t, max_steps=1, dist=8.0 - travel, speed=2.0), t + k, L=L) == (TWO, "may_crash")
    assert decide(lib, record(t, max_steps=1, dist=float("nan"), speed=0.0), t + 1, L=L) == (TWO, "may_crash")
    assert decide(lib, record(t, max_steps=1, dist=float("inf"), speed=0.0), t + 1, L=L) == (TWO, "may_crash")
    assert decide(lib, record(t, max_steps=1, dist=1.0, speed=float("nan")), t + 1, L=L) == (TWO, "may_crash")
    # crashes that do not reset do not matter
    assert decide(lib, record(t, max_steps=1, dist=float("nan"), speed=0.0), t + 1, L=L, roc=0) == (NONE, "proved")
    # a step with a reset gives no "none" proof
    assert decide(lib, record(t, max_steps=1, dist=1.0, reset=True), t + 1, L=L) == (TWO, "reset_no_witness")


def test_witness_rule(lib):
    L, dv = 100, 0.46

    def bit(steps, dist, speed, roc=1):
        return lib.agx_step_proof_witness_bit(L, roc, steps, dist, speed, DT, VMAX, dv)

    assert bit(L, 50.0, 90.0) == 1 << 1  # k = 1: truncates in the next step whatever it does
    assert bit(L - D + 1, 1.0, 0.0) == 1 << D
    assert bit(L - D, 1.0, 0.0) == 0  # k = D + 1: beyond the horizon
    assert bit(L + 1, 1.0, 0.0) == 0  # (k = 0: cannot happen to an env that did not reset)
    k = 10
    travel = lib.agx_step_proof_travel(k - 1, 3.0, DT, VMAX, dv, 1)
    assert travel == pytest.approx(((k - 1) * DT * min(VMAX, 3.0 + (k - 1) * dv)) * 1.01 + 1e-3, rel=1e-6)
    assert bit(L - k + 1, 7.99 - travel, 3.0) == 1 << k
    assert bit(L - k + 1, 8.0 - travel, 3.0) == 0  # could crash before it truncates
    assert bit(L - k + 1, 8.0 - travel, 3.0, roc=0) == 1 << k  # ... which does not reset it
    for d in (float("nan"), -float("nan")):
        assert bit(L, d, 0.0) == 0 and bit(L, d, 0.0, roc=0) == 0  # NaN distances are never witnesses
    assert bit(L - k + 1, 1.0, float("nan")) == 0


def test_dv_of_the_base_quadrotor(lib):
    from conftest import golden_params, load_golden
    from gpu_harness import product_params

    pd = golden_params(load_golden("step_quad_position"))
    P = product_params(pd)
    want = (pd["num_motors"] * max(abs(pd["max_thrust"]), abs(pd["min_thrust"])) / pd["mass"] + 9.81) * pd["dt"] * 1.1
    assert lib.agx_step_proof_dv(C.byref(P)) == pytest.approx(want, rel=1e-5)


def test_travel_bounds_the_oracle_integrator_at_full_thrust(lib):
    """From random states (speeds up to 20 m/s, any attitude and spin), the oracle's integrator driven by the largest body force
    the motors can give (all motors at max_thrust, thrust along body z, random torques): after every m <= D steps the robot is no
    further from where it started than either travel bound."""
    import oracle as orc
    from conftest import golden_params, load_golden
    from gpu_harness import product_params

    pd = golden_params(load_golden("step_quad_position"))
    P, Pc = orc.make_params(pd), product_params(pd)
    dv = lib.agx_step_proof_dv(C.byref(Pc))
    rng = np.random.default_rng(7)
    n = 512
    st = np.zeros((n, 13), np.float32)
    st[:, 0:3] = rng.uniform(-5, 5, (n, 3))
    q = rng.normal(size=(n, 4))
    st[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    v = rng.normal(size=(n, 3))
    st[:, 7:10] = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0, 20, (n, 1))
    st[:, 10:13] = rng.uniform(-10, 10, (n, 3))
    st[: n // 4, 7:10] = 0.0  # (from rest)
    st[: n // 8, 3:7] = [0, 0, 0, 1]  # (level, thrust straight up: with gravity the slowest; below: upside down, with it)
    st[n // 8: n // 4, 3:7] = [1, 0, 0, 0]
    p0 = st[:, 0:3].astype(np.float64).copy()
    speed0 = np.linalg.norm(st[:, 7:10], axis=1).astype(np.float32)
    wrench = np.zeros((n, 6), np.float32)
    wrench[:, 2] = pd["num_motors"] * pd["max_thrust"]
    for m in range(1, D + 1):
        wrench[:, 3:6] = rng.uniform(-0.05, 0.05, (n, 3))
        orc.integrate(P, st, wrench)
        disp = np.linalg.norm(st[:, 0:3].astype(np.float64) - p0, axis=1)
        for per_env in (1, 0):
            bound = np.array([lib.agx_step_proof_travel(m, float(s), pd["dt"], pd["max_linear_velocity"], dv, per_env) for s in speed0])
            assert (disp <= bound).all(), (m, per_env, float((disp - bound).max()))
    assert math.isfinite(float(disp.max()))
