"""GPU parity tests of the dynamics path: HIP kernels (through the C ABI) vs the CPU oracle on
the same inputs, and vs the golden vectors of the reference.  Tolerance: fp32 state within
1e-5 per step (north_star); flags bit-exact."""
import numpy as np
import pytest
from aerial_gym_simulator_amd import _lib as _agx_lib
import torch
from conftest import elem_err, err_where_reference_is_defined, golden_params, load_golden, max_abs, max_rel, rel_err

pytestmark = pytest.mark.gpu

STEP_CASES = ["quad_position", "quad_velocity", "quad_attitude", "quad_acceleration", "quad_no_control",
              "octarotor_position", "octarotor_velocity", "octarotor_fully_actuated", "quad_rates", "quad_velocity_steering"]
TOL = 1e-5


def _angle_err(a, b):
    d = np.abs(a - b)
    return float(np.minimum(d, 2 * np.pi - d).max())


def _derived_split(d):
    return d[:, 0:3], d[:, 3:7], d[:, 7:10], d[:, 10:13], d[:, 13:16]


STATE_PARTS = (("position", slice(0, 3)), ("quaternion", slice(3, 7)), ("linvel", slice(7, 10)), ("angvel", slice(10, 13)))
EXACT = 0.0  # vs the oracle: the kernels evaluate the same IEEE operation sequence (DESIGN.md "numerics")


def state_gate(parity, tag, got, ref, gate=TOL, ctx=None, ref_cr=None):
    """north_star: fp32 state within 1e-5 per step.  vs the oracle (and vs the reference evaluated with correctly rounded
    elementary functions, tests/golden/cr/) the gate is 0 (bit-exact); vs the reference's recorded numbers it is
    |err| <= 1e-5 max(1, |x|) for EVERY component, body rates included (`elem_err`; rounds 1-2 needed 3e-5 there), with
    the plain absolute maximum recorded next to it (|angvel| reaches 12 rad/s in the clipped-action cases)."""
    for name, sl in STATE_PARTS:
        if gate == EXACT:
            parity.check(f"{tag}/{name}", max_abs(got[:, sl], ref[:, sl]), EXACT, "abs (bit-exact)", ctx)
        elif ref_cr is None:
            parity.record(f"{tag}/{name} [abs]", max_abs(got[:, sl], ref[:, sl]), None, "abs")
            parity.check(f"{tag}/{name}", elem_err(got[:, sl], ref[:, sl]), gate, "|err| / max(1, |x|)", ctx)
        else:
            # 1e-5 wherever the reference's own answer is defined to 1e-5; where its result depends on its math library by more
            # than half of that (`ref_cr`: the same code, same inputs, correctly rounded functions) the kernels must return
            # the correctly rounded answer exactly (conftest.err_where_reference_is_defined)
            worst, n_undef, exact_there = err_where_reference_is_defined(got[:, sl], ref[:, sl], ref_cr[:, sl], gate)
            parity.record(f"{tag}/{name} [abs, all elements]", max_abs(got[:, sl], ref[:, sl]), None, "abs")
            parity.record(f"{tag}/{name} [elements where the reference's own libm spread > gate / 2]", n_undef, None, "count")
            parity.check(f"{tag}/{name}", worst, gate, "|err| / max(1, |x|)", ctx)
            assert exact_there, (tag, name, ctx, "not the correctly rounded answer where the reference is ill-conditioned")


def _substeps_vs_cr_reference(parity, case, H):
    """The same launch on the inputs of tests/golden/cr/step_<case>.npz -- the reference's own torch code with correctly
    rounded elementary functions (oracle/cr_torch.py) -- BIT FOR BIT, no oracle in between: derived tensors, controller
    wrench, motor thrusts and the next state (reference control + the integrator restated from PhysX)."""
    g = load_golden("step_" + case, cr=True)
    K = g["state"].shape[0]
    H.set(kT=g["kT"], tau_inc=g["tau_inc"], tau_dec=g["tau_dec"])
    H.set_gains(g["Kp"], g["Kv"], g["KR"], g["Kw"])
    for k in range(K):
        H.set(state=g["state"][k], thrust=g["thrust_in"][k])
        if g["disturb"].any():
            H.set_disturb(g["disturb"][k][None], g["disturb_max"])
        H.substeps(g["action"][k], 1)
        tag = f"substep_vs_reference_with_correctly_rounded_functions[{case}]"
        e, qv, vv, vb, wb = _derived_split(H.get("derived"))
        for name, got, ref in (("euler", e, g["euler"][k]), ("qveh", qv, g["qveh"][k]), ("vveh", vv, g["vveh"][k]),
                               ("vbody", vb, g["vbody"][k]), ("wbody", wb, g["wbody"][k]), ("thrust", H.get("thrust"), g["thrust_out"][k])):
            parity.check(f"{tag}/{name}", max_abs(got, ref), EXACT, "abs (bit-exact)", k)
        if "no_control" not in case:
            parity.check(f"{tag}/wrench", max_abs(H.get("wrench"), g["wrench_cmd"][k]), EXACT, "abs (bit-exact)", k)
        if k + 1 < K:
            parity.check(f"{tag}/next_state", max_abs(H.get("state"), g["state"][k + 1]), EXACT, "abs (bit-exact)", k)


@pytest.mark.parametrize("case", STEP_CASES)
def test_single_substep_vs_oracle_and_golden(orc, parity, case):
    """One physics sub-step through the C ABI on the reference's recorded inputs, per step:
    * vs the CPU oracle: state, motor thrusts, derived tensors and the controller wrench BIT-EXACT;
    * vs the reference's own outputs (goldens): derived body-frame velocities / vehicle quaternion / Euler angles,
      controller wrench, and the next state (reference control + oracle integrator) within 1e-5 max(1, |x|) per
      component; motor thrusts within 1e-5 of the thrust full scale (2 N quad, 6.25 N octarotor)."""
    single_substep_vs_oracle_and_golden(orc, parity, case)


def single_substep_vs_oracle_and_golden(orc, parity, case, edge=False):
    """the comparison of test_single_substep_vs_oracle_and_golden on the fixture tests/golden/step_<case>.npz; edge=True (the
    fixtures of tests/edge_cases_util.py): the gates against the reference's recorded numbers are those of
    edge_cases_util.gates_vs_reference (the same 1e-5, at most 1 % of an array where the reference's own answer is undefined)"""
    from gpu_harness import DynHarness

    g = load_golden("step_" + case)
    pd = golden_params(g)
    n = g["state"].shape[1]
    P = orc.make_params(pd)
    H = DynHarness(pd, n)
    H.set(kT=g["kT"], tau_inc=g["tau_inc"], tau_dec=g["tau_dec"])
    H.set_gains(g["Kp"], g["Kv"], g["KR"], g["Kw"])
    K = g["state"].shape[0]
    fs = max(abs(pd["max_thrust"]), abs(pd["min_thrust"]))
    _substeps_vs_cr_reference(parity, case, H)
    for k in range(K):
        st, th = g["state"][k].copy(), g["thrust_in"][k].copy()
        dist = g["disturb"][k] if g["disturb"][k].any() else None
        o = orc.substep(P, st, g["action"][k], th, g["kT"], g["tau_inc"], g["tau_dec"], g["Kp"], g["Kv"], g["KR"],
                        g["Kw"], disturb=dist, disturb_max=g["disturb_max"], integrate=True)
        H.set(state=g["state"][k], thrust=g["thrust_in"][k])
        if dist is not None:
            H.set_disturb(dist[None], g["disturb_max"])
        H.substeps(g["action"][k], 1)
        gs, gt, gd = H.get("state"), H.get("thrust"), H.get("derived")
        state_gate(parity, f"substep_vs_oracle[{case}]", gs, st, EXACT, ctx=k)
        if edge:
            from edge_cases_util import gates_vs_reference

            e, qv, vv, vb, wb = _derived_split(gd)
            parity.check(f"substep_thrust_vs_oracle[{case}]", max_abs(gt, th), EXACT, "abs (bit-exact)", k)
            parity.check(f"substep_euler_vs_oracle[{case}]", _angle_err(e, o.euler), EXACT, "rad (bit-exact)", k)
            for name, got, ref in (("qveh", qv, o.qveh), ("vveh", vv, o.vveh), ("vbody", vb, o.vbody), ("wbody", wb, o.wbody)):
                parity.check(f"substep_{name}_vs_oracle[{case}]", max_abs(got, ref), EXACT, "abs (bit-exact)", k)
            if "no_control" not in case:
                parity.check(f"substep_wrench_vs_oracle[{case}]", max_abs(H.get("wrench"), o.wrench_cmd), EXACT, "abs (bit-exact)", k)
            gates_vs_reference(parity, "substep", case, g, k, dict(euler=e, qveh=qv, vveh=vv, vbody=vb, wbody=wb, wrench=H.get("wrench"),
                                                                   thrust=gt, next_state=gs), fs)
            assert np.array_equal(H.get("actions"), g["action"][k])
            continue
        if k + 1 < K:  # the generator advanced the reference's wrench with the oracle integrator: state[k + 1]
            state_gate(parity, f"substep_vs_reference_next_state[{case}]", gs, g["state"][k + 1], ctx=k,
                       ref_cr=g["state_next_cr"][k] if "state_next_cr" in g.files else None)
        parity.check(f"substep_thrust_vs_oracle[{case}]", max_abs(gt, th), EXACT, "abs (bit-exact)", k)
        parity.check(f"substep_thrust_vs_reference[{case}]", max_abs(gt, g["thrust_out"][k]) / fs, TOL, "abs / full-scale thrust", k)
        e, qv, vv, vb, wb = _derived_split(gd)
        parity.check(f"substep_euler_vs_oracle[{case}]", _angle_err(e, o.euler), EXACT, "rad (bit-exact)", k)
        parity.check(f"substep_euler_vs_reference[{case}]", _angle_err(e, g["euler"][k]), TOL, "rad", k)
        for name, got, ref, gold in (("qveh", qv, o.qveh, g["qveh"][k]), ("vveh", vv, o.vveh, g["vveh"][k]),
                                     ("vbody", vb, o.vbody, g["vbody"][k]), ("wbody", wb, o.wbody, g["wbody"][k])):
            parity.check(f"substep_{name}_vs_oracle[{case}]", max_abs(got, ref), EXACT, "abs (bit-exact)", k)
            parity.check(f"substep_{name}_vs_reference[{case}]", elem_err(got, gold), TOL, "|err| / max(1, |x|)", k)
        if "no_control" not in case:
            parity.check(f"substep_wrench_vs_oracle[{case}]", max_abs(H.get("wrench"), o.wrench_cmd), EXACT, "abs (bit-exact)", k)
            parity.record(f"substep_wrench_vs_reference[{case}] [abs]", max_abs(H.get("wrench"), g["wrench_cmd"][k]), None, "abs")
            parity.check(f"substep_wrench_vs_reference[{case}]", elem_err(H.get("wrench"), g["wrench_cmd"][k]), TOL, "|err| / max(1, |x|)", k)
        assert np.array_equal(H.get("actions"), g["action"][k])  # robot_actions: what the policy handed in (un-clipped)


@pytest.mark.parametrize("case", ["quad_position", "octarotor_velocity"])
def test_fused_k_substeps_equal_k_launches(orc, parity, case):
    """10 fused sub-steps == 10 oracle sub-steps (config 3/4 use 10, env_with_obstacles.py:29)."""
    from gpu_harness import DynHarness

    g = load_golden("step_" + case)
    pd = golden_params(g)
    n = g["state"].shape[1]
    P = orc.make_params(pd)
    K = 10
    H = DynHarness(pd, n)
    H.set(kT=g["kT"], tau_inc=g["tau_inc"], tau_dec=g["tau_dec"], state=g["state"][0], thrust=g["thrust_in"][0])
    H.set_gains(g["Kp"], g["Kv"], g["KR"], g["Kw"])
    rng = np.random.default_rng(5)
    dist = np.zeros((K, n, 7), np.float32)
    use_dist = case.startswith("octarotor")
    if use_dist:
        dist[:, :, 0] = rng.random((K, n)) < 0.3
        dist[:, :, 1:] = rng.random((K, n, 6))
        H.set_disturb(dist, g["disturb_max"])
    st, th = g["state"][0].copy(), g["thrust_in"][0].copy()
    act = g["action"][0]
    for s in range(K):
        o = orc.substep(P, st, act, th, g["kT"], g["tau_inc"], g["tau_dec"], g["Kp"], g["Kv"], g["KR"], g["Kw"],
                        disturb=dist[s] if use_dist else None, disturb_max=g["disturb_max"])
    H.substeps(act, K)
    # 10 fused free-running sub-steps == 10 oracle sub-steps, bit for bit
    state_gate(parity, f"fused_10_substeps_vs_oracle[{case}]", H.get("state"), st, EXACT)
    parity.check(f"fused_10_substeps_thrust[{case}]", max_abs(H.get("thrust"), th), EXACT, "abs (bit-exact)")
    # derived tensors are those of the LAST sub-step's pre-physics state (stale by one step)
    parity.check(f"fused_10_substeps_body_velocities[{case}]",
                 max_abs(H.get("derived")[:, 10:16], np.concatenate([o.vbody, o.wbody], axis=1)), EXACT, "abs (bit-exact)")
    assert np.array_equal(H.get("prev_actions"), act)  # appendix A #2
    assert int(H.sim_steps.cpu()[0]) == 1


def test_collision_flags_bit_exact(orc):
    from gpu_harness import DynHarness

    g = load_golden("step_quad_position")
    pd = golden_params(g)
    n, K = 256, 24
    rng = np.random.default_rng(11)
    state = np.zeros((n, 13), np.float32)
    state[:, 0:3] = rng.uniform(-2, 2, (n, 3))
    state[:, 6] = 1
    boxes = np.zeros((n, K, 10), np.float32)
    boxes[..., 0:3] = rng.uniform(-2.5, 2.5, (n, K, 3))
    q = rng.normal(size=(n, K, 4))
    boxes[..., 3:7] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    boxes[..., 7:10] = rng.uniform(0.05, 0.6, (n, K, 3))
    H = DynHarness(pd, n)
    H.set(state=state, thrust=np.full((n, 4), 0.6, np.float32), kT=np.full((n, 4), 1.2e-5, np.float32),
          tau_inc=np.full((n, 4), 0.04, np.float32), tau_dec=np.full((n, 4), 0.04, np.float32))
    H.set_gains(*(np.tile(g[k][:1], (n, 1)) for k in ("Kp", "Kv", "KR", "Kw")))
    H.set_boxes(boxes)
    act = np.zeros((n, 4), np.float32)
    act[:, 0:3] = state[:, 0:3]  # hold position
    H.substeps(act, 1)
    got = H.crashes.cpu().numpy()
    # the predicate is evaluated on the post-step position: feed the kernel's own state to the oracle
    crashes = np.zeros(n, np.uint8)
    orc.collide_sphere_boxes(pd["collision_radius"], H.get("state"), boxes, crashes)
    assert np.array_equal(got, crashes.astype(bool))
    assert 0.1 < crashes.mean() < 0.9
    # the stand-alone entry point (EnvManager.compute_observations, env_manager.py:358-362): OR-accumulates from the current state
    from aerial_gym_simulator_amd import _lib

    state2 = H.get("state").copy()
    state2[:, 0:3] = rng.uniform(-2, 2, (n, 3))
    H.set(state=state2)
    pre = (rng.random(n) < 0.2)
    H.crashes.copy_(torch.from_numpy(pre).to(H.crashes.dtype))
    _lib.check(H.lib.agx_collide_spheres_boxes(H.P, H.B, n, H.stream()))
    torch.cuda.synchronize()
    want = pre.astype(np.uint8)
    orc.collide_sphere_boxes(pd["collision_radius"], state2, boxes, want)
    assert np.array_equal(H.crashes.cpu().numpy().astype(bool), want.astype(bool))
    assert (want.astype(bool) & ~pre).any() and (pre & want.astype(bool)).any()  # new hits and kept flags


def test_reward_obs_position(orc):
    from gpu_harness import DynHarness

    g = load_golden("reward_position")
    pd = golden_params(load_golden("step_quad_position"))
    n = g["state"].shape[0]
    H = DynHarness(pd, n)
    derived = np.zeros((n, 16), np.float32)
    derived[:, 3:7], derived[:, 10:13], derived[:, 13:16] = g["qveh"], g["vbody"], g["wbody"]
    H.set(state=g["state"], derived=derived)
    H.crashes.copy_(torch.from_numpy(g["crashes_in"]))
    H.sim_steps.copy_(torch.arange(n, dtype=torch.int32) % 7 + 498)
    r = H.reward_position(g["target"], 500)
    assert max_abs(r, g["reward"]) < TOL  # rewards are O(1..20): absolute
    assert np.array_equal(H.crashes.cpu().numpy(), g["crashes_out"])
    trunc = (np.arange(n) % 7 + 498) > 500
    assert np.array_equal(H.trunc.cpu().numpy(), trunc)
    assert np.array_equal(H.reset_mask.cpu().numpy().astype(bool), g["crashes_out"] | trunc)
    assert int(H.reset_flag.cpu()[0]) == 1 and int(H.reset_flag.cpu()[1]) == 0
    assert np.array_equal(H.obs_position(g["target"]), g["obs"])


def test_reward_navigation(orc, parity):
    from gpu_harness import DynHarness

    g = load_golden("reward_navigation")
    pd = golden_params(load_golden("step_quad_velocity"))
    n = g["state"].shape[0]
    H = DynHarness(pd, n)
    derived = np.zeros((n, 16), np.float32)
    derived[:, 3:7] = g["qveh"]
    H.set(state=g["state"], derived=derived, actions=g["action"], prev_actions=g["prev_action"])
    H.crashes.copy_(torch.from_numpy(g["crashes"]))
    r, pe, ppe = H.reward_navigation(g["target"], g["rp"], float(g["curriculum_progress"]), g["prev_pos_err"],
                                     np.zeros_like(g["pos_err"]), 100)
    assert max_abs(pe, g["pos_err"]) < TOL
    assert np.array_equal(ppe, g["prev_pos_err"])
    # navigation rewards span -100 (collision penalty) .. +40: |err| <= 1e-5 * max(1, |r|) element by element
    parity.record("reward_navigation_vs_reference/abs", max_abs(r, g["reward"]), None)
    parity.check("reward_navigation_vs_reference/rel(floor 1)", max_rel(r, g["reward"], 1.0), 2 * TOL, "rel(floor 1)")


def test_reset_masked_vs_oracle(orc):
    from gpu_harness import DynHarness

    g = load_golden("trace_position_64")
    pd = golden_params(g)
    n = g["init_state"].shape[0]
    H = DynHarness(pd, n)
    ranges = dict(tau_inc=(0.04, 0.04), tau_dec=(0.04, 0.04), kT=(0.00000926312, 0.00001826312))
    rng = np.random.default_rng(3)
    mask = (rng.random(n) < 0.4).astype(np.uint8)
    state0 = g["state_after_step"][10]
    H.set(state=state0, thrust=g["init_thrust"], kT=g["init_kT"], tau_inc=g["init_tau_inc"], tau_dec=g["init_tau_dec"])
    H.sim_steps.fill_(7)
    u = dict(u_bounds_lo=rng.random((n, 3)), u_bounds_hi=rng.random((n, 3)), u_state=g["init_u_state"],
             u_tau_inc=g["init_u_tau_inc"], u_tau_dec=g["init_u_tau_dec"], u_thrust=g["init_u_thrust"], u_kT=g["init_u_kT"])
    e = 1.0
    H.reset_masked(mask, u, ranges, g["min_init_state"], g["max_init_state"], ([-e] * 3, [-e] * 3, [e] * 3, [e] * 3))
    ref = state0.copy()
    orc.reset_robot_state(mask, g["init_u_state"], g["min_init_state"], g["max_init_state"], -np.ones((n, 3), np.float32),
                          np.ones((n, 3), np.float32), ref)
    got = H.get("state")
    assert np.array_equal(got, ref)  # quat_from_euler uses the shared sin / cos kernel: bit-exact
    m = mask.astype(bool)
    assert np.array_equal(got[~m], state0[~m])
    assert max_rel(H.get("thrust")[m], g["init_thrust"][m], 1e-2) < 1e-6  # same draws as the reference's initial reset
    assert np.array_equal(H.get("thrust")[~m], g["init_thrust"][~m])
    assert max_rel(H.get("kT")[m], g["init_kT"][m]) < 1e-6  # kT ~ 1e-5: a relative gate (an absolute one would pass anything)
    steps = H.sim_steps.cpu().numpy()
    assert np.all(steps[m] == 0) and np.all(steps[~m] == 7)
    # derived refreshed for ALL envs
    eu, qv, vv, vb, wb = orc.update_states(got)
    assert np.array_equal(H.get("derived")[:, 3:7], qv) and np.array_equal(H.get("derived")[:, 13:16], wb)
    # nothing happens when no env resets
    before = H.get("derived").copy()
    H.set(state=state0)
    H.reset_masked(np.zeros(n, np.uint8), u, ranges, g["min_init_state"], g["max_init_state"], ([-e] * 3, [-e] * 3, [e] * 3, [e] * 3))
    assert np.array_equal(H.get("derived"), before)


def test_large_batch_properties(orc):
    """BASELINE config-2 size (8192 envs): shard-concatenation equivalence (envs independent) and
    agreement with the oracle on a random subset."""
    from gpu_harness import DynHarness

    g = load_golden("step_quad_position")
    pd = golden_params(g)
    n = 8192
    rng = np.random.default_rng(0)
    idx = rng.integers(0, g["state"].shape[1], n)
    state, thrust = g["state"][0][idx], g["thrust_in"][0][idx]
    state = (state + rng.normal(scale=0.05, size=state.shape)).astype(np.float32)
    state[:, 3:7] /= np.linalg.norm(state[:, 3:7], axis=1, keepdims=True)
    act = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
    arrs = dict(kT=g["kT"][idx], tau_inc=g["tau_inc"][idx], tau_dec=g["tau_dec"][idx])
    H = DynHarness(pd, n)
    H.set(state=state, thrust=thrust, **arrs)
    H.set_gains(g["Kp"][idx], g["Kv"][idx], g["KR"][idx], g["Kw"][idx])
    H.substeps(act, 3)
    full = H.get("state")
    half = n // 2
    for lo in (0, half):
        Hs = DynHarness(pd, half)
        Hs.set(state=state[lo:lo + half], thrust=thrust[lo:lo + half], **{k: v[lo:lo + half] for k, v in arrs.items()})
        Hs.set_gains(*(g[k][idx][lo:lo + half] for k in ("Kp", "Kv", "KR", "Kw")))
        Hs.substeps(act[lo:lo + half], 3)
        assert np.array_equal(Hs.get("state"), full[lo:lo + half])  # bit-identical: no cross-env coupling
    sub = rng.choice(n, 512, replace=False)
    st, th = state[sub].copy(), thrust[sub].copy()
    P = orc.make_params(pd)
    for _ in range(3):
        orc.substep(P, st, act[sub], th, arrs["kT"][sub], arrs["tau_inc"][sub], arrs["tau_dec"][sub], g["Kp"][idx][sub],
                    g["Kv"][idx][sub], g["KR"][idx][sub], g["Kw"][idx][sub])
    assert np.array_equal(full[sub], st)  # 3 fused sub-steps at 8192 envs: bit-exact


def test_device_rng_reset_is_the_documented_philox_stream(orc):
    """Sync-free mode: agx_reset_masked with NULL draw tensors == the same reset fed with the
    oracle's restatement of Philox4x32-10 keyed by (seed; env, episode, stream)."""
    from gpu_harness import DynHarness

    g = load_golden("step_octarotor_velocity")
    pd = golden_params(g)
    n, M = 96, 8
    seed = 0x1234ABCD5678EF01
    rng = np.random.default_rng(9)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    episodes = rng.integers(0, 50, n).astype(np.int32)
    ranges = dict(tau_inc=(0.01, 0.03), tau_dec=(0.005, 0.005), kT=(1e-5, 2e-5))
    gmin = np.arange(12, dtype=np.float32) * 0.1 + 1.0
    gmax = gmin + 0.5
    bounds_cfg = ([-2.0, -4.0, -3.0], [-1.0, -2.5, -2.0], [9.0, 2.5, 2.0], [10.0, 4.0, 3.0])
    lo_s = np.array([0.1, 0.15, 0.15, 0, 0, -0.5, 1, -0.2, -0.2, -0.2, -0.2, -0.2, -0.2], np.float32)
    hi_s = np.array([0.2, 0.85, 0.85, 0, 0, 0.5, 1, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2], np.float32)
    st0 = g["state"][0][np.arange(n) % 64]
    results = []
    for device_rng in (True, False):
        H = DynHarness(pd, n)
        H.set(state=st0, thrust=np.ones((n, M), np.float32))
        H.episode_count.copy_(torch.from_numpy(episodes))
        if device_rng:
            u = dict(seed=seed, randomize_gains=1)
        else:
            ub = orc.rng_fill(seed, episodes, orc.RNG_BOUNDS, 6)
            mot = orc.rng_fill(seed, episodes, orc.RNG_MOTOR, 4 * M).reshape(n, M, 4)
            u = dict(u_bounds_lo=ub[:, :3], u_bounds_hi=ub[:, 3:], u_state=orc.rng_fill(seed, episodes, orc.RNG_STATE, 13),
                     u_gains=orc.rng_fill(seed, episodes, orc.RNG_GAINS, 12), u_tau_inc=mot[..., 0], u_tau_dec=mot[..., 1],
                     u_thrust=mot[..., 2], u_kT=mot[..., 3])
        H.reset_masked(mask, u, ranges, lo_s, hi_s, bounds_cfg, gains_minmax=(gmin, gmax))
        results.append({k: H.get(k) for k in ("state", "thrust", "tau_inc", "tau_dec", "gains", "bmin", "bmax", "derived")})
        ep = H.episode_count.cpu().numpy()
        assert np.array_equal(ep, episodes + mask)
    for k in results[0]:
        assert np.array_equal(results[0][k], results[1][k]), k
    m = mask.astype(bool)
    assert np.all(results[0]["bmin"][m, 0] <= -1.0) and np.all(results[0]["bmin"][m, 0] >= -2.0)
    assert np.all(results[0]["bmin"][~m] == -1.0)  # untouched envs keep the harness default
    # uniforms are in [0,1) and not degenerate
    us = orc.rng_fill(seed, episodes, orc.RNG_STATE, 13)
    assert us.min() >= 0.0 and us.max() < 1.0 and 0.4 < us.mean() < 0.6


def test_fused_epilogue_equals_separate_kernels(orc):
    """agx_env_step with the position-task epilogue == agx_dynamics_substeps + agx_reward_position."""
    from aerial_gym_simulator_amd import _lib
    from gpu_harness import DynHarness, to_soa

    g = load_golden("step_quad_position")
    pd = golden_params(g)
    n = g["state"].shape[1]
    out = []
    for fused in (False, True):
        H = DynHarness(pd, n)
        st = g["state"][0].copy()
        st[:8, 0] = 9.5  # beyond the 8 m crash radius
        H.set(kT=g["kT"], tau_inc=g["tau_inc"], tau_dec=g["tau_dec"], state=st, thrust=g["thrust_in"][0])
        H.set_gains(g["Kp"], g["Kv"], g["KR"], g["Kw"])
        H.sim_steps.copy_(torch.arange(n, dtype=torch.int32) % 5 + 97)
        tgt = to_soa(np.zeros((n, 3), np.float32), H.dev)
        rew = torch.zeros(n, device=H.dev)
        a = torch.from_numpy(g["action"][0]).to(H.dev)
        if fused:
            T = _lib.AgxTaskArgs()
            T.kind, T.episode_len, T.reset_on_collision = _lib.TASK_POSITION, 100, 1
            T.target, T.reward = _lib.dptr(tgt), _lib.dptr(rew)
            _lib.check(H.lib.agx_env_step(H.P, H.B, n, _lib.dptr(a), 2, T, H.stream()))
        else:
            _lib.check(H.lib.agx_dynamics_substeps(H.P, H.B, n, _lib.dptr(a), 2, H.stream()))
            _lib.check(H.lib.agx_reward_position(H.B, n, _lib.dptr(tgt), 100, 1, _lib.dptr(rew), H.stream()))
        torch.cuda.synchronize()
        out.append((H.get("state"), rew.cpu().numpy(), H.crashes.cpu().numpy(), H.trunc.cpu().numpy(),
                    H.reset_mask.cpu().numpy(), H.reset_flag.cpu().numpy()))
    for a_, b_ in zip(*out):
        assert np.array_equal(a_, b_)
    assert out[0][2][:8].all() and out[0][5][0] == 1


def test_device_disturbance_stream(orc):
    """apply_disturbance with in-kernel draws == oracle sub-steps fed with the restated Philox stream."""
    from gpu_harness import DynHarness

    g = load_golden("step_octarotor_velocity")
    pd = golden_params(g)
    n, K, seed, step, prob = g["state"].shape[1], 4, 0xABCDEF0123, 321, 0.3
    P = orc.make_params(pd)
    H = DynHarness(pd, n)
    H.set(kT=g["kT"], tau_inc=g["tau_inc"], tau_dec=g["tau_dec"], state=g["state"][0], thrust=g["thrust_in"][0])
    H.set_gains(g["Kp"], g["Kv"], g["KR"], g["Kw"])
    for i in range(6):
        H.B.disturb_max[i] = float(g["disturb_max"][i])
    H.B.disturb_prob, H.B.step_counter, H.B.rng_seed = prob, step, seed
    st, th = g["state"][0].copy(), g["thrust_in"][0].copy()
    occ_total = 0
    for s in range(K):
        u = orc.rng_fill(seed, np.full(n, step, np.int32), (1 << 20) + s, 7)
        d = u.copy()
        d[:, 0] = (u[:, 0] < prob).astype(np.float32)
        occ_total += int(d[:, 0].sum())
        orc.substep(P, st, g["action"][0], th, g["kT"], g["tau_inc"], g["tau_dec"], g["Kp"], g["Kv"], g["KR"], g["Kw"],
                    disturb=d, disturb_max=g["disturb_max"])
    H.substeps(g["action"][0], K)
    assert occ_total > 10
    assert np.array_equal(H.get("state"), st)  # 4 fused sub-steps with in-kernel draws: bit-exact
    # and it really was applied: without disturbance the result differs
    H2 = DynHarness(pd, n)
    H2.set(kT=g["kT"], tau_inc=g["tau_inc"], tau_dec=g["tau_dec"], state=g["state"][0], thrust=g["thrust_in"][0])
    H2.set_gains(g["Kp"], g["Kv"], g["KR"], g["Kw"])
    H2.substeps(g["action"][0], K)
    assert rel_err(H2.get("state"), st) > 1e-4


@pytest.mark.parametrize("case", ["quad_position", "quad_velocity", "quad_attitude", "quad_rates", "quad_acceleration",
                                  "quad_velocity_steering", "octarotor_fully_actuated", "octarotor_position", "octarotor_velocity"])
@pytest.mark.parametrize("k", [1, 4])
def test_four_lanes_per_env_kernels_cover_the_six_lee_laws(case, k, monkeypatch):
    """Every Lee law of the quadrotor and the three laws of the octarotor (fully actuated = BASELINE configs[3], Lee position,
    Lee velocity, control/__init__.py:94-96: two motors per lane; recorded disturbance draws included) have a
    four-lanes-per-env kernel (k_env_step_quad_position for one position-control sub-step, k_env_step_quad_loop<M, CTRL>
    otherwise): agx_env_step_kernel names it, and k sub-steps from the golden case's recorded states / actions / gains give
    bit for bit the buffers of the one-lane kernel (agx_set_option("env_step_quad", 0))."""
    import ctypes as C

    from gpu_harness import DynHarness

    g = load_golden("step_" + case)
    pd = golden_params(g)
    n = g["state"].shape[1]
    outs = {}
    for quad in ("0", "1"):
        _agx_lib.set_option("env_step_quad", int(quad))
        H = DynHarness(pd, n)
        H.set(kT=g["kT"], tau_inc=g["tau_inc"], tau_dec=g["tau_dec"])
        H.set_gains(g["Kp"], g["Kv"], g["KR"], g["Kw"])
        buf = C.create_string_buffer(128)
        H.lib.agx_env_step_kernel(H.P, H.B, n, k, None, buf, 128)
        name = buf.value.decode()
        if quad == "1":
            assert name.startswith("k_env_step_quad_position" if (case == "quad_position" and k == 1) else "k_env_step_quad_loop<"), name
        else:
            assert name.startswith("k_env_step<8," if case.startswith("octarotor") else "k_env_step<4,"), name
        got = []
        for s in range(g["state"].shape[0]):
            H.set(state=g["state"][s], thrust=g["thrust_in"][s])
            if g["disturb"].any():  # the octarotor's recorded disturbance draws, the same in each of the k sub-steps
                H.set_disturb(np.repeat(g["disturb"][s][None], k, axis=0), g["disturb_max"])
            H.substeps(g["action"][s], k)
            got.append([H.get(x).copy() for x in ("state", "thrust", "derived", "wrench")])
        outs[quad] = got
    for s, (a, b) in enumerate(zip(outs["0"], outs["1"])):
        for name, x, y in zip(("state", "thrust", "derived", "wrench"), a, b):
            assert np.array_equal(x, y), (case, k, s, name, np.abs(x - y).max())


@pytest.mark.parametrize("pattern", ["none", "one", "all", "random"])
@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])  # one lane, a partial wave, the exact wave, one over, a partial second 256-thread workgroup
def test_reset_set_entry_at_wave_edges(n, parity, pattern):
    """agx_reset_set through the C ABI, with and without reset_on_collision: reset_mask = crashes * reset_on_collision | truncations
    for every env (the mask starts at 7: a lane that was not written shows), the flag word of this parity = some env resets, the
    other parity's word and the two inputs unchanged.  `one`: a single crashed env, the last one (the last, partial wave)."""
    from task_test_util import Buffers, host

    crashes, trunc = np.zeros(n, bool), np.zeros(n, bool)
    if pattern == "one":
        crashes[n - 1] = True
    elif pattern == "all":
        crashes[:], trunc[:] = True, True
    elif pattern == "random":
        rng = np.random.default_rng(1000 * n + parity)
        crashes, trunc = rng.random(n) < 0.3, rng.random(n) < 0.2
    for roc in (0, 1):
        H = Buffers(n, np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32), crashes=crashes, parity=parity)
        H.truncations.copy_(torch.from_numpy(trunc))
        H.reset_flag[parity ^ 1] = 5
        _agx_lib.check(H.lib.agx_reset_set(H.B, n, roc, H.stream()), "agx_reset_set")
        torch.cuda.synchronize()
        mask = (crashes & bool(roc)) | trunc
        assert np.array_equal(host(H.reset_mask), mask.astype(np.uint8)), (roc, np.flatnonzero(host(H.reset_mask) != mask))
        flags = host(H.reset_flag)
        assert flags[parity] == int(mask.any()) and flags[parity ^ 1] == 5, (roc, flags)
        assert np.array_equal(host(H.crashes), crashes) and np.array_equal(host(H.truncations), trunc)
