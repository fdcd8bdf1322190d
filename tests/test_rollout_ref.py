"""CPU: tests/rollout_ref.py -- the restatement of T task-free env steps the GPU tests of agx_env_rollout compare with
(tests/test_gpu_rollout_limits.py) -- against the pieces it is made of, and the box scenes it builds against what they were built
for.  No GPU."""
import numpy as np
import pytest

import collision_cases as cc
import rollout_ref as rr
from task_test_util import bits

SCRIPTS = ([1, 0, 2, 1, 3], [0, 0, 0], [0, 2], [3, 1], [32], [0, 3])


def _init(n, A, M):
    return rr.initial(n, A, M, 3)


@pytest.mark.parametrize("case,k", [("quad_velocity", 4), ("octarotor_fully_actuated", 3)])
def test_one_step_is_the_base_of_the_collision_cases(orc, case, k):
    state, action, m = cc._base(case, 37, k, 9)
    pd = m["pd"]
    init = _init(37, pd["num_actions"], pd["num_motors"])
    ref = rr.oracle_rollout(pd, state, m["thrust"], m["kT"], m["tau_inc"], m["tau_dec"], m["gains"], action, [k], **init)
    assert np.array_equal(bits(ref.end["state"]), bits(m["final_state"])) and np.array_equal(bits(ref.end["thrust"]), bits(m["final_thrust"]))
    assert len(ref.traj) == 1 and np.array_equal(bits(ref.traj[0]), bits(m["traj"]))
    assert np.array_equal(bits(ref.state[0]), bits(m["final_state"])) and np.array_equal(bits(ref.thrust[0]), bits(m["final_thrust"]))
    # the derived tensors are those of the state BEFORE the last sub-step, the wrench the last sub-step's
    st, th = state.copy(), m["thrust"].copy()
    P = orc.make_params(pd)
    for _ in range(k - 1):
        orc.substep(P, st, action.copy(), th, m["kT"], m["tau_inc"], m["tau_dec"], *m["gains"])
    stale = np.concatenate(orc.update_states(st), axis=1)
    assert np.array_equal(bits(ref.end["derived"]), bits(stale))
    o = orc.substep(P, st, action.copy(), th, m["kT"], m["tau_inc"], m["tau_dec"], *m["gains"])
    assert np.array_equal(bits(ref.end["wrench"]), bits(o.wrench_cmd))
    assert np.array_equal(ref.end["sim_steps"], init["sim_steps0"] + 1) and not ref.end["truncations"].any() and not ref.crash.any()
    assert (ref.first_crash == -1).all()


@pytest.mark.parametrize("T,k", [(5, 1), (3, 4)])
def test_steps_of_k_substeps_are_one_step_of_all_of_them(orc, T, k):
    x, ref = rr.reference("quad_velocity", 37, 4, [k] * T)
    x1, one = rr.reference("quad_velocity", 37, 4, [T * k])
    for key in ("state", "thrust", "derived", "wrench"):
        assert np.array_equal(bits(ref.end[key]), bits(one.end[key])), key
    assert np.array_equal(bits(np.concatenate(ref.traj)), bits(one.traj[0]))
    assert np.array_equal(ref.end["sim_steps"], x["sim_steps0"] + T) and np.array_equal(one.end["sim_steps"], x["sim_steps0"] + 1)


@pytest.mark.parametrize("script", [[1], [2], [0], [1, 0], [0, 0]])
def test_action_history_rule(orc, script):
    """k >= 2: both histories hold the step's action; k = 1: prev takes what cur held; k = 0: neither moves"""
    x, ref = rr.reference("quad_velocity", 5, 6, script, held=False)
    a, a0, p0 = x["actions"], x["actions0"], x["prev_actions0"]
    want = {(1,): (a0, a[0]), (2,): (a[0], a[0]), (0,): (p0, a0), (1, 0): (a0, a[0]), (0, 0): (p0, a0)}[tuple(script)]
    assert np.array_equal(bits(ref.end["prev_actions"]), bits(want[0])) and np.array_equal(bits(ref.end["actions"]), bits(want[1]))
    assert not np.array_equal(a0, p0) and not np.array_equal(a0, a[0])
    if not any(script):  # nothing but the counters moves
        for key, was in (("state", x["state"]), ("thrust", x["thrust"]), ("derived", x["derived0"])):
            assert np.array_equal(bits(ref.end[key]), bits(was)), key
        assert np.array_equal(bits(ref.end["wrench"]), bits(x["wrench0"]))
        for t in range(len(script)):
            assert np.array_equal(bits(ref.state[t]), bits(x["state"])) and np.array_equal(bits(ref.derived[t]), bits(x["derived0"]))


def _scene(script, K, n=70, seed=11):
    plan = rr.plan_for(n, K)
    x, ref = rr.reference("quad_velocity", n, seed, script, slow=np.array([c == "near" for c in plan["cls"]]))
    boxes, meta = rr.scenes(ref.traj, x["r"], np.random.default_rng(seed + 1), plan)
    return x, ref, boxes, meta


@pytest.mark.parametrize("K", [1, 3, 17])
@pytest.mark.parametrize("script", SCRIPTS)
def test_scene_classes_carry_the_flags_they_were_built_for(orc, script, K):
    x, ref, boxes, meta = _scene(script, K)
    full = rr.with_boxes(ref, boxes)
    T, n = len(script), 70
    assert int(meta.ambiguous.sum()) == 0
    assert np.array_equal(full.crash, meta.want) and np.array_equal(full.crash, meta.flags64)
    first = np.array([next((t for t in range(T) if meta.want[t, i]), -1) for i in range(n)], np.int32)
    assert np.array_equal(full.first_crash, first) and np.array_equal(full.end["crashes"], meta.want[-1].astype(np.uint8))
    run = [t for t, k in enumerate(script) if k > 0]
    by = {c: [i for i in range(n) if meta.cls[i] == c] for c in rr.CLASSES}
    for c in ("near", "parked"):
        assert not meta.want[:, by[c]].any()
    if not run:
        assert len(by["parked"]) == n and not meta.want.any()
        return
    assert len(by["first"]) >= 2 and len(by["last"]) >= 2 and len(by["near"]) >= 2 and len(by["parked"]) >= 2
    for i in by["first"]:
        assert meta.want[:, i].tolist() == [t == run[0] for t in range(T)]
    for i in by["last"]:
        assert meta.want[:, i].tolist() == [t == run[-1] for t in range(T)]
    if len(run) >= 2:
        assert len(by["two"]) >= 2
        for i in by["two"]:
            assert meta.want[:, i].sum() == 2 and full.first_crash[i] == run[0]
    if script in ([1, 0, 2, 1, 3], [3, 1]):  # the stale LDS rows: a hit at the last sub-step, the successor (k = 1) misses
        t = 2 if len(script) == 5 else 0
        assert len(by["stale"]) >= 2
        at = np.concatenate([[0], np.cumsum(script)])
        for i in by["stale"]:
            assert meta.want[:, i].tolist() == [s == t for s in range(T)] and script[t + 1] == 1
            hit = (meta.d64[:, i] < x["r"]).any(-1)
            assert hit.sum() == 1 and hit[at[t + 1] - 1]
    if script == [1, 0, 2, 1, 3]:
        assert len(by["then_zero"]) >= 2
        for i in by["then_zero"]:
            assert meta.want[:, i].tolist() == [True, False, False, False, False]
    # the near misses reach the predicate on every step that runs; a hit box does on its step
    assert meta.passes_cull[run][:, by["near"]].all()
    assert (meta.passes_cull & (meta.d64.min(0)[None] < x["r"])).any()


def test_inputs_depend_on_the_seed_alone_and_are_read_only(orc):
    a = _scene([1, 0, 2, 1, 3], 3)
    b = _scene([1, 0, 2, 1, 3], 3)
    c = _scene([1, 0, 2, 1, 3], 3, seed=12)
    arrays = lambda s: ([v for v in s[0].values() if isinstance(v, np.ndarray)] + [s[1].state, s[1].derived, s[1].thrust, s[1].crash,  # noqa: E731
                        s[1].first_crash, *s[1].traj, *(v for v in s[1].end.values() if v is not None), s[2], s[3].want, s[3].flags64])
    for u, v in zip(arrays(a), arrays(b)):
        assert np.array_equal(bits(u), bits(v)) and not u.flags.writeable
    assert not np.array_equal(a[2], c[2]) and not np.array_equal(a[0]["state"], c[0]["state"])
    assert all(not g.flags.writeable for g in a[0]["gains"])


def test_disturbance_draws_follow_the_device_stream(orc):
    """the rows are offset by env_index_base, the stream index wraps at 31 bits, and the sub-step picks the stream"""
    dmax = np.array([0.75, 0.75, 0.75, 0.004, 0.004, 0.004], np.float32)
    x, ref = rr.reference("octarotor_velocity", 9, 5, [3, 3, 3, 3], disturb=(77, 0x7FFFFFFE, 0.3, dmax, 4))
    x0, clean = rr.reference("octarotor_velocity", 9, 5, [3, 3, 3, 3])
    assert ref.applied > 0 and not np.array_equal(ref.end["state"], clean.end["state"])
    # steps 2 and 3 draw at the indices 0 and 1: the same rollout started there, from the state step 1 left, ends in the same bits
    m = dict(pd=x["pd"], thrust=ref.thrust[1], kT=x["kT"], tau_inc=x["tau_inc"], tau_dec=x["tau_dec"], gains=x["gains"])
    y, tail = rr.reference("octarotor_velocity", 9, 5, [3, 3], disturb=(77, 0, 0.3, dmax, 4), start_at=(ref.state[1], x["actions"], m))
    assert np.array_equal(bits(tail.end["state"]), bits(ref.end["state"])) and np.array_equal(bits(tail.end["thrust"]), bits(ref.end["thrust"]))
