"""T steps of the task-free env step, restated on the CPU from `oracle.substep` and `oracle.collide_sphere_boxes` (plain numpy + the
oracle, no GPU): what agx_dyn_rollout.h and the header comment of agx_env_rollout promise, written down once more.

`oracle_rollout` runs the dynamics; `with_boxes` adds the crash flags of a box scene to its result (boxes do not change the
dynamics, so the trajectory is computed once, before any box is placed); `scenes` places boxes RELATIVE to the recorded sub-step
positions with the helpers of tests/collision_cases.py.  Every array of a result is AoS ([N, C], as the oracle lays them out) and
read-only.
"""
import types

import numpy as np

import collision_cases as cc
import oracle as orc

RNG_DISTURB = 1 << 20  # the device generator's stream of the disturbance draws; + the sub-step index


def _ro(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.flags.writeable = False


def crash_flags(radius, traj, boxes):
    """([T, n] bool, first_crash [n] int32): the sphere/box predicate OR-ed over the k_t positions of each step alone (all clear
    for a step without sub-steps), and the first step whose flag is set, or -1"""
    T, n = len(traj), boxes.shape[0]
    flags = np.zeros((T, n), bool)
    for t, p in enumerate(traj):
        if p.shape[0]:
            flags[t] = cc.oracle_hits_per_substep(radius, p, boxes).any(0)
    first = np.where(flags.any(0), flags.argmax(0), -1).astype(np.int32)
    return flags, first


def oracle_rollout(pd, state, thrust, kT, tau_inc, tau_dec, gains, actions, ks, *, actions0, prev_actions0, derived0, sim_steps0,
                   boxes=None, disturb=None, wrench0=None):
    """`len(ks)` env steps; `actions` [N, A] (held) or [T, N, A]; `gains` = (Kp, Kv, KR, Kw), each [N, 3]; `disturb` = None or
    (seed, step0, prob, disturb_max [6], env_index_base): the device generator's draws, restated.  `wrench0`: what the wrench
    buffer held before (it is returned untouched when no step has a sub-step).

    Returns a namespace: the per-step record `state` [T, N, 13], `derived` [T, N, 16], `thrust` [T, N, M], `crash` [T, N] bool; the
    end buffers `end` (dict: state, derived, thrust, actions, prev_actions, wrench, crashes, truncations, sim_steps) and
    `first_crash` [N]; `traj`, a list of T arrays [k_t, N, 3] with every sub-step position; `applied`, the number of disturbance
    draws that applied."""
    P = orc.make_params(pd)
    ks = [int(k) for k in ks]
    T, n = len(ks), state.shape[0]
    actions = np.asarray(actions, np.float32)
    held = actions.ndim == 2
    assert held or actions.shape[0] == T
    st, th = np.array(state, np.float32), np.array(thrust, np.float32)
    derived = np.array(derived0, np.float32)
    cur, prev = np.array(actions0, np.float32), np.array(prev_actions0, np.float32)
    wrench = None if wrench0 is None else np.array(wrench0, np.float32)
    rec = dict(state=np.zeros((T, n, 13), np.float32), derived=np.zeros((T, n, 16), np.float32),
               thrust=np.zeros((T, n, th.shape[1]), np.float32))
    traj, applied = [], 0
    for t, k in enumerate(ks):
        a = np.ascontiguousarray(actions if held else actions[t])
        pos = np.zeros((k, n, 3), np.float32)
        for sub in range(k):
            kw = {}
            if disturb is not None:
                seed, step0, prob, dmax, base = disturb
                step = (int(step0) + t) & 0x7FFFFFFF
                u = orc.rng_fill(seed, np.full(base + n, step, np.int32), RNG_DISTURB + sub, 7)[base:]
                d = u.copy()
                d[:, 0] = (u[:, 0] < np.float32(prob)).astype(np.float32)
                applied += int(d[:, 0].sum())
                kw = dict(disturb=d, disturb_max=np.asarray(dmax, np.float32))
            o = orc.substep(P, st, a.copy(), th, kT, tau_inc, tau_dec, *gains, **kw)
            pos[sub] = st[:, 0:3]
            # (what the sub-step computed BEFORE it integrated: one sub-step stale)
            derived = np.concatenate([o.euler, o.qveh, o.vveh, o.vbody, o.wbody], axis=1)
            wrench = o.wrench_cmd.copy()
        traj.append(pos)
        if k >= 2:  # RobotManagerIGE.pre_physics_step runs every sub-step: prev <- cur, cur <- action
            prev, cur = a.copy(), a.copy()
        elif k == 1:
            prev, cur = cur, a.copy()
        rec["state"][t], rec["derived"][t], rec["thrust"][t] = st, derived, th
    out = types.SimpleNamespace(T=T, n=n, ks=ks, traj=traj, applied=applied, radius=pd["collision_radius"], **rec)
    out.end = dict(state=st, derived=derived, thrust=th, actions=cur, prev_actions=prev, wrench=wrench,
                   truncations=np.zeros(n, np.uint8), sim_steps=(np.asarray(sim_steps0, np.int64) + T).astype(np.int32))
    _ro(*rec.values(), *traj, *out.end.values())
    return with_boxes(out, boxes)


def with_boxes(ref, boxes):
    """the result `ref` with the crash flags of the scene `boxes` [N, K, 10] (None: no obstacles); the dynamics are shared"""
    out = types.SimpleNamespace(**vars(ref))
    if boxes is None:
        out.crash, out.first_crash = np.zeros((ref.T, ref.n), bool), np.full(ref.n, -1, np.int32)
    else:
        out.crash, out.first_crash = crash_flags(ref.radius, ref.traj, np.ascontiguousarray(boxes, np.float32))
    out.end = dict(ref.end, crashes=out.crash[-1].astype(np.uint8))
    _ro(out.crash, out.first_crash, out.end["crashes"])
    return out


def record_channel(ref, source, component):
    """[T, N] float32: the channel (AGX_REC_* source, component) of the record"""
    a = (ref.state, ref.derived, ref.thrust, ref.crash[..., None].astype(np.float32))[source]
    return a[:, :, component]


# ---------------------------------------------------------------------------------------------------------------------------
# box scenes on a recorded rollout
# ---------------------------------------------------------------------------------------------------------------------------
CLASSES = ("first", "last", "two", "stale", "then_zero", "near", "parked")
MARGIN = 0.15  # every decisive distance stays this far (in radii) from the radius, as in collision_cases.py


def class_pattern(name, ks, K):
    """(steps that are to carry a hit, sub-step the hit is pinned to or None) of a scene class under the sub-step script `ks`;
    None when the script has no step the class needs (the env then gets the class 'last', or 'parked' without any sub-step).
    * first: the first step (with a sub-step);  * last: the last such step only;
    * two: two separate steps (with one box per env: two adjacent ones, the box between them);
    * stale: the LAST sub-step of a step with k >= 2 whose successor has k = 1 and misses -- the LDS rows 1.. of the successor
      still hold the hit;  * then_zero: a step followed by a step without sub-steps."""
    run = [t for t, k in enumerate(ks) if k > 0]
    if not run:
        return None
    if name == "first":
        return [run[0]], None
    if name == "last":
        return [run[-1]], None
    if name == "two":
        if len(run) < 2:
            return None
        return ([run[0], run[1]] if K == 1 else [run[0], run[-1]]), None
    if name == "stale":
        for t in range(len(ks) - 1):
            if ks[t] >= 2 and ks[t + 1] == 1:
                return [t], ks[t] - 1
        return None
    if name == "then_zero":
        for t in range(len(ks) - 1):
            if ks[t] > 0 and ks[t + 1] == 0:
                return [t], None
        return None
    raise KeyError(name)


def _sample_hit(rng, pos, step_of, r, want_steps, anchor, pinned=None, tries=4000):
    """one small box at 0.3 .. 0.8 r from the point `anchor` (random orientation, a face, an edge or a corner towards it) that hits
    positions of exactly the steps `want_steps` (and, with `pinned`, the position of that index and no other), every distance at
    least MARGIN r from the radius"""
    for _ in range(tries):
        h = rng.uniform(0.02, 0.25, (1, 3)) * r
        axes_out = rng.random((1, 3)) < 0.5
        axes_out[0, rng.integers(0, 3)] = True
        local = cc._outside_point(rng, h, r * rng.uniform(0.3, 0.8, 1), axes_out)
        b = cc._box(anchor[None], cc._rand_quat(rng, 1), h, local)[0]
        d = cc.obb_distance64(pos, b[None])
        if (np.abs(d - r) < MARGIN * r).any():
            continue
        hit = d < r
        if pinned is not None and not (hit[pinned] and hit.sum() == 1):
            continue
        if sorted(set(step_of[hit].tolist())) == sorted(want_steps):
            return b
    raise AssertionError("box placement did not converge")


def _sample_near(rng, pos, step_of, r, steps, tries=400):
    """one near miss (collision_cases._near_misses) whose bounding sphere reaches the AABB of EVERY step's positions"""
    for _ in range(tries):
        b = cc._near_misses(rng, pos[:, None, :], r, 1)[0, 0]
        c, reach = b[0:3].astype(np.float64), np.linalg.norm(b[7:10].astype(np.float64)) + r - 1.0e-3
        ok = True
        for t in steps:
            p = pos[step_of == t].astype(np.float64)
            ok = ok and np.linalg.norm(np.maximum(np.maximum(p.min(0) - c, c - p.max(0)), 0.0)) < reach
        if ok:
            return b
    raise AssertionError("near-miss placement did not converge")


def scenes(traj, r, rng, plan):
    """boxes [n, K, 10] for the recorded sub-step positions `traj` (list of T arrays [k_t, n, 3]); plan = dict(K=boxes per env,
    cls=[n] class names of CLASSES).  Hits sit at box index i % K (for 'two' with K >= 2: also (i + 1) % K); the other boxes
    alternate between near misses of the whole trajectory and boxes parked at +-1e3 m; 'near' envs carry K near misses that pass
    the cull on every step, 'parked' envs K parked boxes.  Returns (boxes, meta): meta.want [T, n] the flags the scene was built
    for, meta.cls the classes actually built (a class the script cannot express falls back, see class_pattern), meta.flags64 the
    float64 flags, meta.ambiguous [n].  Asserts: no env is ambiguous, float64 flags == the oracle's == want."""
    K, cls = int(plan["K"]), list(plan["cls"])
    ks = [p.shape[0] for p in traj]
    T, n = len(traj), traj[0].shape[1]
    assert len(cls) == n
    allpos = np.concatenate(traj, axis=0)  # [S, n, 3]
    step_of = np.repeat(np.arange(T), ks)
    first_of = np.concatenate([[0], np.cumsum(ks)])
    run = [t for t in range(T) if ks[t] > 0]
    boxes = cc._parked(rng, n * K).reshape(n, K, 10)
    want = np.zeros((T, n), bool)
    built = []
    for i in range(n):
        name = cls[i]
        pos = allpos[:, i].astype(np.float64)
        pat = None if name in ("near", "parked") else class_pattern(name, ks, K)
        if name not in ("near", "parked") and pat is None:
            name, pat = ("last", class_pattern("last", ks, K)) if run else ("parked", None)
        if not run and name == "near":
            name = "parked"
        built.append(name)
        if name == "parked":
            continue
        if name == "near":
            for j in range(K):
                boxes[i, j] = _sample_near(rng, allpos[:, i], step_of, r, run)
            continue
        for j in range(K):  # the boxes around the hit: near misses of the whole trajectory and parked ones, alternating
            if (j - i) % 2 == 1:
                boxes[i, j] = cc._near_misses(rng, allpos[:, i:i + 1], r, 1)[0, 0]
        steps, pin = pat
        want[steps, i] = True
        if pin is not None:
            s = first_of[steps[0]] + pin
            boxes[i, i % K] = _sample_hit(rng, pos, step_of, r, steps, pos[s], pinned=s)
        elif len(steps) == 2 and K == 1:
            a, b = first_of[steps[0] + 1] - 1, first_of[steps[1]]  # last position of the one step, first of the other
            boxes[i, 0] = _sample_hit(rng, pos, step_of, r, steps, 0.5 * (pos[a] + pos[b]))
        else:
            for m, t in enumerate(steps):
                s = first_of[t] + int(rng.integers(0, ks[t]))
                boxes[i, (i + m) % K] = _sample_hit(rng, pos, step_of, r, [t], pos[s])
    boxes = np.ascontiguousarray(boxes, np.float32)
    d64 = cc.obb_distance64(allpos[:, :, None, :], boxes[None])  # [S, n, K]
    bound = cc.separation_error_bound(allpos[:, :, None, :], boxes[None], r)
    ambiguous = (np.abs(d64 - r) <= bound).any((0, 2))
    assert int(ambiguous.sum()) == 0, ("ambiguous envs", np.nonzero(ambiguous)[0].tolist())
    hit64 = (d64 < r).any(2)  # [S, n]
    flags64 = np.stack([hit64[step_of == t].any(0) if ks[t] else np.zeros(n, bool) for t in range(T)])
    flags, first = crash_flags(np.float32(r), traj, boxes)
    assert np.array_equal(flags64, flags), "the float64 flags are not the oracle's"
    assert np.array_equal(flags64, want), "a scene env does not carry the flags it was built for"
    # the cull of the kernels in float64, per step: which (step, env, box) the predicate runs on
    passes = np.zeros((T, n, K), bool)
    c = boxes[..., 0:3].astype(np.float64)
    reach = np.linalg.norm(boxes[..., 7:10].astype(np.float64), axis=-1) + r
    for t in run:
        p = traj[t].astype(np.float64)
        lo, hi = p.min(0)[:, None, :], p.max(0)[:, None, :]
        passes[t] = np.linalg.norm(np.maximum(np.maximum(lo - c, c - hi), 0.0), axis=-1) < reach
    meta = types.SimpleNamespace(K=K, cls=tuple(built), want=want, flags64=flags64, first_crash=first, ambiguous=ambiguous,
                                 passes_cull=passes, d64=d64)
    near = np.array([b == "near" for b in built])
    assert passes[run][:, near].all(), "a near miss is culled on some step"
    _ro(boxes, want, flags64, first, ambiguous, passes, d64)
    return boxes, meta


def plan_for(n, K, classes=CLASSES):
    """every class in turn: with n >= 2 len(classes) each is carried by at least two envs"""
    return dict(K=K, cls=[classes[i % len(classes)] for i in range(n)])


# ---------------------------------------------------------------------------------------------------------------------------
# inputs the CPU and the GPU tests share
# ---------------------------------------------------------------------------------------------------------------------------
FAST, SLOW = (1.3, 1.6), (0.25, 0.4)  # collision radii per sub-step: FAST keeps consecutive positions a hit/miss margin apart


def start(case, n, seed, slow=None):
    """(state, action, m) of collision_cases._base for the fixture `case`: n envs moving at FAST, the envs of the mask `slow` at
    SLOW (a near miss can reach every step's positions only when they stay together)"""
    v0 = None
    if slow is not None and np.any(slow):
        pd = cc.golden_params(cc.load_golden("step_" + case))
        rng = np.random.default_rng(seed + 500)
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        v = d * rng.uniform(SLOW[0], SLOW[1], (n, 1)) * float(np.float32(pd["collision_radius"])) / pd["dt"]
        v0 = np.where(np.asarray(slow, bool)[:, None], v, np.nan)
    return cc._base(case, n, 0, seed, speed=FAST, v0=v0)


def initial(n, A, M, seed):
    """what the buffers hold before the launch: distinct, non-zero actions / prev_actions / wrench, a derived tensor of its own,
    distinct per-env step counts"""
    rng = np.random.default_rng(seed + 900)
    return dict(actions0=rng.uniform(0.1, 0.9, (n, A)).astype(np.float32), prev_actions0=rng.uniform(-0.9, -0.1, (n, A)).astype(np.float32),
                wrench0=rng.uniform(1.0, 2.0, (n, 6)).astype(np.float32), derived0=rng.uniform(-3.0, 3.0, (n, 16)).astype(np.float32),
                sim_steps0=(5 + 3 * np.arange(n)).astype(np.int32))


def schedule(action, T, seed):
    """[T, N, A]: the held action with another small offset in every step, so that the rows differ"""
    rng = np.random.default_rng(seed + 700)
    return (action[None] + rng.uniform(-0.2, 0.2, (T,) + action.shape)).astype(np.float32)


def reference(case, n, seed, ks, held=True, slow=None, disturb=None, pd_update=None, uniform=False, start_at=None):
    """(inputs dict, oracle_rollout result without boxes) of one run; pd_update: entries laid over the fixture's parameters (drag,
    root-link mode); uniform: every env gets env 0's gains x 1.25 and motor time constants x 1.125 (the arm of the kernels that reads them from
    the parameter block); start_at: (state, action, m) to use instead of start()"""
    state, action, m = start_at if start_at is not None else start(case, n, seed, slow)
    pd = dict(m["pd"])
    pd.update(pd_update or {})
    M, A = pd["num_motors"], pd["num_actions"]
    gains, tau_inc, tau_dec = m["gains"], m["tau_inc"], m["tau_dec"]
    if uniform:
        gains = tuple(np.ascontiguousarray(np.broadcast_to(g[0:1] * np.float32(1.25), g.shape)) for g in gains)
        tau_inc, tau_dec = (np.full_like(t, t[0, 0] * np.float32(1.125)) for t in (tau_inc, tau_dec))
        pd.update(gains_uniform=[float(x) for g in gains for x in g[0]], tau_inc_uniform=float(tau_inc[0, 0]), tau_dec_uniform=float(tau_dec[0, 0]))
    init = initial(n, A, M, seed)
    actions = action if held else schedule(action, len(ks), seed)
    x = dict(pd=pd, n=n, state=state, thrust=m["thrust"], kT=m["kT"], tau_inc=tau_inc, tau_dec=tau_dec, gains=gains, actions=actions,
             ks=[int(k) for k in ks], disturb=disturb, uniform=uniform, r=float(np.float32(pd["collision_radius"])), **init)
    ref = oracle_rollout(pd, state, x["thrust"], x["kT"], tau_inc, tau_dec, gains, actions, ks, disturb=disturb, **init)
    _ro(*(v for v in x.values() if isinstance(v, np.ndarray)), *gains)
    return x, ref
