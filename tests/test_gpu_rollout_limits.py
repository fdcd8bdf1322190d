"""GPU: agx_env_rollout / k_env_step_rollout at the C ABI, against the CPU restatement tests/rollout_ref.py (oracle.substep,
oracle.collide_sphere_boxes, oracle.rng_fill) and against a twin harness driven by T calls of agx_dynamics_substeps with
buf->step_counter advanced by hand -- the eager loop at the ABI.  Reached here and not through EnvManager: motor constants in RPS,
drag (with a disturbance: the split root sum), per-env and uniform gains, six motors, velocity steering, obstacles in the
256-thread instances and above 64 KiB of LDS, the device generator with several sub-steps and across the 31-bit wrap of the stream
index, the wrench buffer, record tables in any order, and every refusal of the entry.

Every run: 256 sentinel elements behind every buffer, the record and first_crash; crashes / truncations start as ones, sim_steps at
distinct values, actions / prev_actions / wrench at distinct non-zero values, the record as NaN.  Every comparison is
np.array_equal (the twin's on the bit patterns)."""
import copy
import ctypes as C
import re

import numpy as np
import pytest
import torch

import rollout_ref as rr
from aerial_gym_simulator_amd import _lib
from edge_cases_util import arrangement
from gpu_harness import product_params
from task_test_util import bits
from test_gpu_collision_flags import GUARD, SENTINEL, GuardedHarness

pytestmark = pytest.mark.gpu

N = 70  # one full wave and a partial one
N_WIDE = 65537 + 3  # 256-thread workgroups, the last one partial (tests/test_gpu_body_force.py)
DRAG = dict(lin_drag_linear=[0.031, 0.047, 0.059], lin_drag_quadratic=[0.023, 0.037, 0.053], ang_drag_linear=[0.0011, 0.0017, 0.0023],
            ang_drag_quadratic=[0.0007, 0.0013, 0.0019])
DMAX = np.array([0.75, 0.75, 0.75, 0.004, 0.004, 0.004], np.float32)
END = ("state", "derived", "thrust", "actions", "prev_actions", "wrench", "crashes", "truncations", "sim_steps")


# ---- harnesses -----------------------------------------------------------------------------------------------------------------
def make_harness(x, boxes=None, P=None):
    """a GuardedHarness holding the inputs `x` of rollout_ref.reference (and the box scene): the set-up of the module docstring"""
    H = GuardedHarness(x["pd"], x["n"])
    if P is not None:
        H.P = P
    H.set(state=x["state"], thrust=x["thrust"], kT=x["kT"], tau_inc=x["tau_inc"], tau_dec=x["tau_dec"], actions=x["actions0"],
          prev_actions=x["prev_actions0"], wrench=x["wrench0"], derived=x["derived0"])
    H.set_gains(*x["gains"])
    if boxes is not None:
        H.set_boxes(boxes)
    H.crashes.fill_(1)
    H.trunc.fill_(1)
    H.sim_steps.copy_(torch.from_numpy(x["sim_steps0"].copy()))
    if x["disturb"] is not None:
        seed, step0, prob, dmax, base = x["disturb"]
        H.B.rng_seed, H.B.step_counter, H.B.disturb_prob, H.B.env_index_base = seed, step0, prob, base
        for c in range(6):
            H.B.disturb_max[c] = float(dmax[c])
    if x["uniform"]:  # the arm that reads gains and motor time constants from the parameter block (behind every rebind())
        H.B.gains = H.B.motor_tau_inc = H.B.motor_tau_dec = None
    return H


def end_buffers(H):
    out = {k: H.get(k) for k in ("state", "derived", "thrust", "actions", "prev_actions", "wrench")}
    out.update(crashes=H.crashes.cpu().numpy(), truncations=H.trunc.cpu().numpy(), sim_steps=H.sim_steps.cpu().numpy())
    return out


def raw_buffers(H):
    """every allocation of the harness with its guard band, and what the last rollout() call allocated"""
    out = {k: raw.clone() for k, (raw, numel) in H.raw.items()}
    out.update({"rollout_" + k: raw.clone() for k, (raw, numel) in getattr(H, "rollout_raw", {}).items()})
    return out


def same_raw(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)


def check_guards(H):
    H.check_guards()
    for name, (raw, numel) in H.rollout_raw.items():
        assert bool((raw[numel:] == SENTINEL).all()), f"{name}: written behind its end"


def all_sources(M):
    return [(_lib.REC_STATE, c) for c in range(13)] + [(_lib.REC_DERIVED, c) for c in range(16)] + [(_lib.REC_THRUST, j) for j in range(M)] + \
        [(_lib.REC_CRASH, 0)]


def shuffled_tables(M, seed=1):
    """every source of an M-motor robot once, in a shuffled order, over two tables of up to 32 channels"""
    src = all_sources(M)
    order = np.random.default_rng(seed).permutation(len(src))
    src = [src[i] for i in order]
    assert src != sorted(src)
    return [src[:32], src[32:]]


def launch_args(x, raw_script=None, substeps=None):
    """(substeps, per_step) of the call: the scalar count when every step has the same, else the array and its largest entry"""
    ks = x["ks"]
    if raw_script is None and len(set(ks)) == 1:
        return ks[0], None
    return (max(ks) if substeps is None else substeps), (ks if raw_script is None else raw_script)


def run_rollout(x, table, boxes=None, raw_script=None, substeps=None, first_crash=True, P=None):
    H = make_harness(x, boxes, P)
    k, per_step = launch_args(x, raw_script, substeps)
    rc, rec, first = H.rollout(x["actions"], len(x["ks"]), k, per_step=per_step, record=table, first_crash=first_crash, guard=GUARD,
                               sentinel=SENTINEL)
    assert rc == 0, (rc, H.lib.agx_last_error().decode())
    check_guards(H)
    return end_buffers(H), rec, first


def run_twin(x, boxes=None, P=None):
    """T calls of agx_dynamics_substeps, buf->step_counter advanced by hand: (end buffers, per-step record dict, first_crash)"""
    H = make_harness(x, boxes, P)
    T, step0 = len(x["ks"]), int(H.B.step_counter)
    rec = dict(state=[], derived=[], thrust=[], crash=[])
    for t in range(T):
        H.B.step_counter = (step0 + t) & 0x7FFFFFFF
        H.substeps(np.array(x["actions"] if x["actions"].ndim == 2 else x["actions"][t]), x["ks"][t])  # (a writable copy)
        rec["state"].append(H.get("state"))
        rec["derived"].append(H.get("derived"))
        rec["thrust"].append(H.get("thrust"))
        rec["crash"].append(H.crashes.cpu().numpy().astype(bool))
    H.check_guards()
    rec = {k: np.stack(v) for k, v in rec.items()}
    first = np.where(rec["crash"].any(0), rec["crash"].argmax(0), -1).astype(np.int32)
    return end_buffers(H), rec, first


def check(x, ref, boxes=None, tables=None, **launch):
    """the four checks of every case; `ref` carries the crash flags of `boxes`.  Returns the end buffers of the last launch."""
    M = x["pd"]["num_motors"]
    for key in ("state", "derived", "thrust"):  # 4. the oracle's values are finite
        assert np.isfinite(getattr(ref, key)).all() and np.isfinite(ref.end[key]).all(), key
    twin_end, twin_rec, twin_first = run_twin(x, boxes, launch.get("P"))
    ends = []
    for table in (shuffled_tables(M) if tables is None else tables):
        end, rec, first = run_rollout(x, table, boxes, **launch)
        ends.append(end)
        for key in END:  # 1. the oracle, 2. the twin
            assert np.array_equal(end[key], ref.end[key]), ("oracle", key, np.nonzero(end[key] != ref.end[key])[0][:8].tolist())
            assert np.array_equal(bits(end[key]), bits(twin_end[key])), ("twin", key)
        if first is not None:
            assert np.array_equal(first, ref.first_crash) and np.array_equal(first, twin_first)
        if table:
            assert rec.shape == (ref.T, len(table), ref.n) and not np.isnan(rec).any()  # 3. no NaN is left in the record
            for c, (src, comp) in enumerate(table):
                assert np.array_equal(rec[:, c], rr.record_channel(ref, src, comp)), ("oracle", src, comp)
                twin = (twin_rec["state"], twin_rec["derived"], twin_rec["thrust"], twin_rec["crash"][..., None].astype(np.float32))[src][:, :, comp]
                assert np.array_equal(bits(rec[:, c]), bits(twin)), ("twin", src, comp)
    for end in ends[1:]:  # the end buffers do not depend on what was recorded
        for key in END:
            assert np.array_equal(bits(end[key]), bits(ends[0][key])), key
    return ends[0]


# ---- laws and robots ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["quad_position", "quad_velocity", "quad_attitude", "quad_rates", "quad_acceleration", "quad_velocity_steering",
                                  "quad_no_control", "octarotor_fully_actuated", "octarotor_velocity", "tinyprop_no_control"])
def test_laws_and_robots_of_the_step_fixtures(orc, case):
    """per-env kT / tau / gains as the fixtures carry them, a schedule whose rows differ, 2 sub-steps x 4 steps; the wrench buffer is
    compared in every case (quad_no_control: zeros over the non-zero start), tinyprop and the quadrotors have use_rps"""
    x, ref = rr.reference(case, N, 21, [2] * 4, held=False, slow=np.ones(N, bool))
    assert not np.array_equal(x["actions"][0], x["actions"][1])
    if case in ("tinyprop_no_control", "quad_velocity"):
        assert x["pd"]["use_rps"] == 1 and (x["kT"] != 1.0).all()  # (without use_rps the kernels take kT = 1)
    end = check(x, ref)
    assert (end["wrench"] != x["wrench0"]).all()
    if case.endswith("no_control"):
        assert not end["wrench"].any()


@pytest.mark.parametrize("case", ["quad_velocity", "octarotor_fully_actuated"])
def test_uniform_gains_and_time_constants_from_the_parameter_block(orc, case):
    """buf->gains, motor_tau_inc and motor_tau_dec null: the oracle is fed the uniform values pack_robot_params puts into the block"""
    x, ref = rr.reference(case, N, 22, [3] * 3, held=True, slow=np.ones(N, bool), uniform=True)
    P = product_params(x["pd"])
    assert np.array_equal(np.array(P.gains_uniform[:], np.float32), np.concatenate([g[0] for g in x["gains"]]))
    assert np.float32(P.tau_inc_uniform) == x["tau_inc"][0, 0] and np.float32(P.tau_dec_uniform) == x["tau_dec"][0, 0]
    check(x, ref)
    y, other = rr.reference(case, N, 22, [3] * 3, held=True, slow=np.ones(N, bool))
    assert not np.array_equal(other.end["state"], ref.end["state"])  # the per-env constants of the fixture end elsewhere


def six_motor_inputs(n, seed):
    """the six-motor parameter block of tests/test_gpu_com_offset.py -- the quadrotor's block with num_motors = 6: its 6 x 4
    matrices read with a row length of 6, zeros behind them -- as a parameter dict both sides are built from"""
    state, action, m = rr.start("quad_position", n, seed, slow=np.ones(n, bool))
    pd4 = m["pd"]
    pd = dict(pd4, num_motors=6, motor_dir=list(pd4["motor_dir"]) + [0.0, 0.0])
    for name in ("alloc", "alloc_pinv", "wrench_map"):
        pd[name] = [float(v) for v in np.ravel(pd4[name])] + [0.0] * 12
    P6 = copy.copy(product_params(pd4))
    P6.num_motors = 6
    assert bytes(product_params(pd)) == bytes(P6)
    wide = lambda a: np.ascontiguousarray(a[:, np.arange(6) % 4] * np.float32([1, 1, 1, 1, 0.9, 1.1]))  # noqa: E731
    m6 = dict(m, pd=pd, thrust=wide(m["thrust"]), kT=wide(m["kT"]), tau_inc=wide(m["tau_inc"]), tau_dec=wide(m["tau_dec"]))
    return state, action, m6


def test_six_motors(orc):
    start = six_motor_inputs(N, 23)
    # one sub-step first: agx_dynamics_substeps equals the oracle for these parameters
    x, one = rr.reference("quad_position", N, 23, [1], start_at=start)
    end, rec, first = run_twin(x)
    for key in ("state", "thrust", "derived", "wrench"):
        assert np.array_equal(end[key], one.end[key]), key
    assert (one.end["thrust"][:, 4:] != x["thrust"][:, 4:]).any()
    x, ref = rr.reference("quad_position", N, 23, [2, 1, 3, 2], held=False, start_at=start)
    check(x, ref)


# ---- drag and the device generator's disturbance --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["drag", "drag_disturbed", "drag_disturbed_root_link"])
def test_drag(orc, mode):
    """non-zero linear, quadratic and angular drag; with the device disturbance the root body's sum is formed first (split_root);
    in root-link mode it is the running sum again"""
    upd = dict(DRAG, root_link_mode=1) if mode.endswith("root_link") else DRAG
    disturb = None if mode == "drag" else (0x5EED1234, 40, 0.3, DMAX, 3)
    x, ref = rr.reference("quad_velocity", N, 24, [3] * 4, held=False, slow=np.ones(N, bool), pd_update=upd, disturb=disturb)
    y, clean = rr.reference("quad_velocity", N, 24, [3] * 4, held=False, slow=np.ones(N, bool), disturb=disturb,
                            pd_update=dict(root_link_mode=upd.get("root_link_mode", 0)))
    assert (clean.end["state"][:, 7:13] != ref.end["state"][:, 7:13]).any(axis=1).all()  # the drag is felt by every env
    assert disturb is None or ref.applied > 0
    check(x, ref)


@pytest.mark.parametrize("step0", [321, 0x7FFFFFFE])
def test_device_disturbance_with_three_substeps_per_step(orc, step0):
    """k = 3, T = 5, disturb_prob = 0.3, env_index_base = 5; from step_counter = 0x7FFFFFFE the steps 2 and 3 draw at the stream
    indices 0 and 1"""
    disturb = (0xABCDEF0123, step0, 0.3, DMAX, 5)
    x, ref = rr.reference("octarotor_velocity", N, 25, [3] * 5, slow=np.ones(N, bool), disturb=disturb)
    y, clean = rr.reference("octarotor_velocity", N, 25, [3] * 5, slow=np.ones(N, bool))
    assert ref.applied > 10 and not np.array_equal(clean.end["state"], ref.end["state"])
    z, unshifted = rr.reference("octarotor_velocity", N, 25, [3] * 5, slow=np.ones(N, bool), disturb=disturb[:4] + (0,))
    assert not np.array_equal(unshifted.end["state"], ref.end["state"])  # the row offset matters
    check(x, ref)


# ---- sub-step scripts, with and without boxes ----------------------------------------------------------------------------------------
def scene_for(script, K, n=N, seed=11, held=True, classes=rr.CLASSES):
    plan = rr.plan_for(n, K, classes)
    x, ref = rr.reference("quad_velocity", n, seed, script, held=held, slow=np.array([c == "near" for c in plan["cls"]]))
    boxes, meta = rr.scenes(ref.traj, x["r"], np.random.default_rng(seed + 1), plan)
    assert int(meta.ambiguous.sum()) == 0
    full = rr.with_boxes(ref, boxes)
    assert np.array_equal(full.crash, meta.want)
    return x, full, boxes, meta


@pytest.mark.parametrize("held", [True, False], ids=["held", "schedule"])
@pytest.mark.parametrize("with_boxes", [False, True], ids=["empty", "boxes"])
@pytest.mark.parametrize("script", [[1, 0, 2, 1, 3], [0, 0, 0], [0, 2], [3, 1], [32]], ids=lambda s: "-".join(map(str, s)))
def test_substep_scripts(orc, script, with_boxes, held):
    x, ref, boxes, meta = scene_for(script, 3, held=held)
    if not with_boxes:
        ref, boxes = rr.with_boxes(ref, None), None
    end = check(x, ref, boxes)
    if not any(script):  # nothing but the counters may change
        for key, was in (("state", x["state"]), ("derived", x["derived0"]), ("thrust", x["thrust"]), ("actions", x["actions0"]),
                         ("prev_actions", x["prev_actions0"]), ("wrench", x["wrench0"])):
            assert np.array_equal(bits(end[key]), bits(was)), key
        assert not end["crashes"].any() and not end["truncations"].any() and np.array_equal(end["sim_steps"], x["sim_steps0"] + 3)
    elif with_boxes:
        assert ref.crash.any() and (ref.first_crash >= 0).any() and (ref.first_crash < 0).any()


@pytest.mark.parametrize("held", [True, False], ids=["held", "schedule"])
@pytest.mark.parametrize("with_boxes", [False, True], ids=["empty", "boxes"])
def test_counts_outside_the_launch_are_cut(orc, with_boxes, held):
    """substeps = 3 with an array that holds -5 and 40: cut to 0 and 3; the oracle and the twin get the cut counts"""
    raw, cut = [2, -5, 40, 1, 3], [2, 0, 3, 1, 3]
    x, ref, boxes, meta = scene_for(cut, 3, held=held)
    if not with_boxes:
        ref, boxes = rr.with_boxes(ref, None), None
    check(x, ref, boxes, raw_script=raw, substeps=3)


# ---- obstacles --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [53, 70])
@pytest.mark.parametrize("K", [1, 3, 17])
def test_scene_classes(orc, K, n):
    """every scene class of rollout_ref.scenes under quad_velocity, on the script that expresses them all"""
    x, ref, boxes, meta = scene_for([1, 0, 2, 1, 3], K, n=n, seed=30 + K)
    assert set(meta.cls) == set(rr.CLASSES) and all(meta.cls.count(c) >= 2 for c in rr.CLASSES)
    check(x, ref, boxes)


def test_scene_classes_with_one_count_for_every_step(orc):
    """the scalar sub-step count (no array): k = 4, T = 6, K = 5"""
    x, ref, boxes, meta = scene_for([4] * 6, 5, seed=36, held=False)
    assert ref.crash.any(1).sum() >= 2
    check(x, ref, boxes)


# ---- 256-thread instances ------------------------------------------------------------------------------------------------------------------
WIDE_HITS = {0: "first", 63: "last", 64: "two", 255: "first", 256: "last", 65535: "two", 65536: "first", N_WIDE - 3: "two", N_WIDE - 2: "last",
             N_WIDE - 1: "first", 1000: "near", 1001: "near"}


def wide_scene(script, seed):
    cls = ["parked"] * N_WIDE
    for i, c in WIDE_HITS.items():
        cls[i] = c
    x, ref = rr.reference("quad_velocity", N_WIDE, seed, script, held=False, slow=np.array([c == "near" for c in cls]))
    boxes, meta = rr.scenes(ref.traj, x["r"], np.random.default_rng(seed + 1), dict(K=2, cls=cls))
    assert int(meta.ambiguous.sum()) == 0
    full = rr.with_boxes(ref, boxes)
    hit = full.crash.any(0)
    # env 0, env n - 1, envs of the last (partial) workgroup, envs on both sides of a wave edge and of a workgroup edge
    assert hit[[0, 63, 64, 255, 256, 65535, 65536, N_WIDE - 3, N_WIDE - 2, N_WIDE - 1]].all() and hit.sum() == 10
    assert 65536 // 256 == (N_WIDE - 1) // 256 == N_WIDE // 256 and N_WIDE % 256 != 0  # the last workgroup holds four envs
    return x, full, boxes


def test_wide_without_boxes(orc):
    """n = 65 540: k_env_step_rollout<4, VELOCITY, WIDE = false>, 256-thread workgroups.  Oracle and twin cover ALL envs."""
    x, ref = rr.reference("quad_velocity", N_WIDE, 41, [2, 2], held=False, slow=np.ones(N_WIDE, bool))
    check(x, ref, tables=shuffled_tables(4)[:1])


def test_wide_with_boxes(orc):
    """K = 2 boxes, k = 4, T = 2: traj[(sub * 3 + c) * 256 + tid].  Oracle and twin cover ALL envs."""
    x, ref, boxes = wide_scene([4, 4], 42)
    check(x, ref, boxes, tables=shuffled_tables(4)[1:])


def test_wide_above_64_kib_of_lds(orc):
    """the script [22, 21] with boxes: 22 x 3 x 256 x 4 B = 67 584 B of dynamic LDS, the smallest count above the 64 KiB a launch
    gets without opting in, so launch_env_rollout takes its hipFuncSetAttribute branch (a launch that asks for more than the
    function's limit fails, and agx_env_rollout would return AGX_E_LAUNCH).  Oracle and twin cover ALL envs."""
    assert 22 * 3 * 256 * 4 == 67584 > 64 * 1024 >= 21 * 3 * 256 * 4
    x, ref, boxes = wide_scene([22, 21], 43)
    check(x, ref, boxes, tables=[[(_lib.REC_CRASH, 0), (_lib.REC_STATE, 2), (_lib.REC_DERIVED, 15), (_lib.REC_THRUST, 3)]])


# ---- record tables -----------------------------------------------------------------------------------------------------------------------
def test_record_tables(orc):
    """all 38 sources of an eight-motor robot over two shuffled launches (as in every case above), one channel alone, no record,
    no first_crash, neither: the end buffers are the same bits every time"""
    x, ref = rr.reference("octarotor_velocity", N, 51, [2, 1, 3], held=False, slow=np.ones(N, bool))
    tables = shuffled_tables(8)
    assert sorted(tables[0] + tables[1]) == sorted(all_sources(8)) and len(tables[0]) == 32 and len(tables[1]) == 6
    end = check(x, ref, tables=tables + [[(_lib.REC_DERIVED, 2)]])
    x, ref, boxes, meta = scene_for([1, 0, 2, 1, 3], 3, seed=52)
    end = check(x, ref, boxes, tables=[[(_lib.REC_DERIVED, 2)], None])
    for table, first_crash in (([(_lib.REC_CRASH, 0)], False), (None, False)):
        got, rec, first = run_rollout(x, table, boxes, first_crash=first_crash)
        assert first is None
        for key in END:
            assert np.array_equal(bits(got[key]), bits(end[key])), key
        if table:
            assert np.array_equal(rec[:, 0], ref.crash.astype(np.float32)) and ref.crash.any()


# ---- one env has the same bits wherever it sits ---------------------------------------------------------------------------------------------
def take(x, idx):
    y = dict(x, n=len(idx), gains=tuple(g[idx] for g in x["gains"]))
    for key in ("state", "thrust", "kT", "tau_inc", "tau_dec", "actions0", "prev_actions0", "wrench0", "derived0", "sim_steps0"):
        y[key] = np.ascontiguousarray(x[key][idx])
    y["actions"] = np.ascontiguousarray(x["actions"][idx] if x["actions"].ndim == 2 else x["actions"][:, idx])
    return y


@pytest.mark.parametrize("rotate,cut", [(17, None), (5, 1), (29, 63)])
def test_an_env_has_the_same_bits_wherever_it_sits(orc, rotate, cut):
    x, ref, boxes, meta = scene_for([1, 0, 2, 1, 3], 3, seed=61, held=False)
    table = shuffled_tables(4)[0]
    end, rec, first = run_rollout(x, table, boxes)
    idx = arrangement(N, rotate, cut)
    got, rec2, first2 = run_rollout(take(x, idx), table, boxes[idx])
    for key in END:
        assert np.array_equal(bits(got[key]), bits(end[key][idx])), key
    assert np.array_equal(bits(rec2), bits(rec[:, :, idx])) and np.array_equal(first2, first[idx])
    assert cut == 1 or (first2 >= 0).any()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _record(channels, pairs, out):
    rec = _lib.AgxRolloutRecord()
    rec.channels, rec.out = channels, out
    for c, (src, comp) in enumerate(pairs):
        rec.source[c], rec.component[c] = src, comp
    return rec


def test_refusals_name_the_reason_and_write_nothing(orc):
    x, ref, boxes, meta = scene_for([2, 2, 2], 3, seed=71)
    H = make_harness(x, boxes)
    T, M = 3, 4
    scratch = torch.zeros(16 * N, device=H.dev)
    out = torch.full((T * 33 * N + GUARD,), float("nan"), device=H.dev)
    H.raw["record_out"] = (out, out.numel())
    good = [(_lib.REC_STATE, 0), (_lib.REC_CRASH, 0)]
    rec = lambda pairs, channels=None, null=False: _record(len(pairs) if channels is None else channels, pairs, None if null else out.data_ptr())  # noqa: E731
    buf = lambda **kw: ("buf", kw)  # noqa: E731
    P_wrench, P_five = copy.copy(H.P), copy.copy(H.P)
    P_wrench.controller, P_five.num_motors = _lib.CTRL_IDS["wrench"], 5
    p = scratch.data_ptr()
    cases = [
        (dict(steps=0), -1, r"steps must be >= 1 \(got 0\)"),
        (dict(substeps=-1), -1, "substeps out of range: -1"),
        (dict(substeps=33), -1, "substeps out of range: 33"),
        (dict(actions_per_step=2), -1, "actions_per_step is 0 .* got 2"),
        (dict(actions=None), -1, "null actions"),
        (dict(P=P_wrench), -1, "AGX_CTRL_WRENCH"),
        (dict(P=P_five), -3, "num_motors 5"),
        (buf(disturb=p), -1, "buf->disturb is set"),
        (buf(body_force=p), -1, "buf->body_force is set"),
        (buf(step_counter_dev=p), -1, "buf->step_counter_dev is set"),
        (buf(step_rows=(p, p), step_reward=p), -1, "exchange rows / peer push are bound"),
        (buf(push_world=1), -1, "exchange rows / peer push are bound"),
        (buf(motor_kT=None), -1, "null motor_kT with use_rps"),
        (dict(record=rec(good, null=True)), -1, "record->out is null"),
        (dict(record=rec(good, channels=0)), -1, r"record->channels 0 outside 1\.\.32"),
        (dict(record=rec(good, channels=33)), -1, r"record->channels 33 outside 1\.\.32"),
        (dict(record=rec([(_lib.REC_STATE, 0), (4, 0)])), -1, "record channel 1: unknown source 4"),
        (dict(record=rec([(-1, 0)])), -1, "record channel 0: unknown source -1"),
        (dict(record=rec([(_lib.REC_STATE, 13)])), -1, r"component 13 outside 0\.\.12 of source 0"),
        (dict(record=rec([(_lib.REC_STATE, -1)])), -1, r"component -1 outside 0\.\.12 of source 0"),
        (dict(record=rec([(_lib.REC_DERIVED, 16)])), -1, r"component 16 outside 0\.\.15 of source 1"),
        (dict(record=rec([(_lib.REC_THRUST, M)])), -1, r"component 4 outside 0\.\.3 of source 2"),
        (dict(record=rec([(_lib.REC_CRASH, 1)])), -1, r"component 1 outside 0\.\.0 of source 3"),
        (dict(record=rec(good + [(_lib.REC_DERIVED, 5), (_lib.REC_STATE, 0)])), -1, r"record channels 0 and 3 name the same \(source, component\)"),
    ]
    cases += [(buf(launch_flags=(1 << b) - (1 << 32 if b == 31 else 0)), -1, "launch_flags must be 0") for b in range(32)]
    cases += [(buf(**{name: None}), -1, "null env buffer")
              for name in ("state", "derived", "actions", "prev_actions", "motor_thrust", "crashes", "truncations", "sim_steps")]
    assert x["pd"]["use_rps"] == 1
    before = raw_buffers(H)
    pristine = bytes(H.B)
    for what, code, message in cases:
        kw = dict(actions=x["actions"], steps=T, substeps=2, record=good, guard=GUARD, sentinel=SENTINEL)
        if isinstance(what, tuple):
            for name, value in what[1].items():
                if name == "step_rows":
                    H.B.step_rows[0], H.B.step_rows[1] = value
                else:
                    setattr(H.B, name, value)
        else:
            kw.update(what)
        rc, rec_out, first = H.rollout(**kw)
        text = H.lib.agx_last_error().decode()
        C.memmove(C.byref(H.B), pristine, len(pristine))
        assert rc == code, (what, rc, text)
        assert "agx_env_rollout" in text or code == -3, text
        assert re.search(message, text), (what, text)
        assert same_raw({k: v for k, v in raw_buffers(H).items() if not k.startswith("rollout_")}, before), (what, "a refused call wrote")
        if rec_out is not None:
            assert np.isnan(rec_out).all(), what
        assert (first == -7).all(), what
        check_guards(H)
    # ... and the same harness still runs: the buffers were left as they were
    rc, rec_out, first = H.rollout(x["actions"], T, 2, record=good, guard=GUARD, sentinel=SENTINEL)
    assert rc == 0 and np.array_equal(first, ref.first_crash) and np.array_equal(end_buffers(H)["state"], ref.end["state"])
    assert np.array_equal(rec_out[:, 1], ref.crash.astype(np.float32))
