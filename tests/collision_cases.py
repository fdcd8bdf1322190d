"""Obstacle scenes that put the crash flag of the env-step kernels at its limits (plain numpy + the CPU oracle, no GPU).

The GPU state after k sub-steps equals the oracle's bit for bit (test_gpu_dynamics.py, gate 0), so the robot's k sub-step positions
are known on the CPU: `orc.substep` is run k times from a chosen start state and the boxes are placed RELATIVE to the recorded
positions.  The expected flag is `orc.collide_sphere_boxes` after every oracle sub-step, OR-accumulated (as test_gpu_nav_task.py
does it).  Robots, gains and motor constants are those of the tests/golden/step_<case>.npz fixtures.

Every family returns `(state [N,13], action [N,A], boxes [N,K,10], expected_flags [N] bool, meta)`; `meta` carries what a GPU run
needs besides (params, motor tensors, gains), the recorded trajectory, the oracle's final state and per-sub-step hits, and the
family's own bookkeeping.  The arrays are shared between tests (lru_cache) and read-only.

Independent geometry: `obb_distance64` is the sphere-centre / oriented-box distance written from the definition in float64 (a
rotation MATRIX of the normalised quaternion, clamp to the box, Euclidean norm) -- not the quaternion formula of the oracle and the
kernels.  `separation_error_bound` bounds how far their float32 evaluation can be from it; cases closer to the radius than that
are "ambiguous" and only the oracle defines their answer.
"""
import functools

import numpy as np
from conftest import golden_params, load_golden

import oracle as orc

PARKED = 1.0e3  # where the scene parks inactive obstacles [m]


# ---------------------------------------------------------------------------------------------------------------------------
# float64 geometry
# ---------------------------------------------------------------------------------------------------------------------------
def rotmat64(q):
    """rotation matrix [..., 3, 3] (box frame -> world) of the quaternion xyzw [..., 4], normalised in float64"""
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    x, y, z, w = np.moveaxis(q, -1, 0)
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    return R


def obb_distance64(p, boxes):
    """distance of the points p [..., 3] from the solid oriented boxes [..., 10] (centre, quaternion xyzw, half extents; the leading
    dimensions broadcast): 0 inside.  The point in the box frame is R^T (p - c); the closest point of the box is its clamp."""
    p, b = np.asarray(p, np.float64), np.asarray(boxes, np.float64)
    local = np.einsum("...ji,...j->...i", rotmat64(b[..., 3:7]), p - b[..., 0:3])
    outside = np.maximum(np.abs(local) - b[..., 7:10], 0.0)
    return np.sqrt((outside * outside).sum(-1))


def separation_error_bound(p, boxes, r):
    """Bound on |float32 separation - obb_distance64| for the predicate of the oracle and the kernels, u = 2^-24:

    * v = p - c: one rounding per component, <= u |v|;
    * the rotation v s - 2 w (q x v) + 2 q (q . v) (|s| <= 1, every term <= 2 |v|): about ten roundings of quantities <= 2 |v| per
      component, <= 20 u |v|; the stored quaternion is a ROUNDED unit quaternion (| |q|^2 - 1 | <= 4 u) and the formula does not
      normalise it: <= 4 u |v| more.  Per component <= 25 u |v| with the first item;
    * e = |l| - h: <= u max(|l|, h) <= u (|v| + max h);
    * the distance is 1-Lipschitz in (ex, ey, ez): <= sqrt(3) (26 u |v| + u max h) <= u (46 |v| + 2 max h);
    * squares and their sum: <= 3 u relative on d^2, 1.5 u d on d, with d ~ r at the threshold; r * r rounded: 0.5 u r.

    Sum: u (46 |v| + 2 max h + 2 r) <= 2^-23 (24 |v| + max h + r), which is what is returned (|v| = centre-to-point distance)."""
    p, b = np.asarray(p, np.float64), np.asarray(boxes, np.float64)
    v = np.linalg.norm(p - b[..., 0:3], axis=-1)
    return 2.0 ** -23 * (24.0 * v + b[..., 7:10].max(-1) + r)


def _rand_quat(rng, m):
    q = rng.normal(size=(m, 4))
    return (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(np.float32)


def _box(p, q, h, local):
    """the box (float32 row of 10) with orientation q and half extents h in whose frame the point p has the coordinates `local`"""
    q = np.asarray(q, np.float32)
    c = np.asarray(p, np.float64) - np.einsum("...ij,...j->...i", rotmat64(q), np.asarray(local, np.float64))
    return np.concatenate([c, q.astype(np.float64), np.asarray(h, np.float64)], axis=-1).astype(np.float32)


def _outside_point(rng, h, dist, axes_out):
    """box-frame coordinates of a point at distance `dist` from the box h [m, 3]: beyond the faces of the axes marked in
    axes_out [m, 3] bool (1 axis: a face, 2: an edge, 3: a corner), anywhere within the extents along the others; random octant"""
    m = h.shape[0]
    u = np.abs(rng.normal(size=(m, 3))) * axes_out
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    inside = rng.uniform(-1.0, 1.0, (m, 3)) * h
    sign = rng.choice([-1.0, 1.0], (m, 3))
    return np.where(axes_out, sign * (h + np.asarray(dist).reshape(m, 1) * u), inside)


def _parked(rng, m):
    c = rng.choice([-PARKED, PARKED], (m, 3)) + rng.uniform(-5.0, 5.0, (m, 3))
    return np.concatenate([c, _rand_quat(rng, m), rng.uniform(0.1, 0.5, (m, 3))], axis=-1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# the robot's k sub-step positions, from the oracle
# ---------------------------------------------------------------------------------------------------------------------------
def _yaw(q):
    x, y, z, w = (q[:, i].astype(np.float64) for i in range(4))
    return np.arctan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))


def _base(case, n, k, seed, speed=(0.25, 0.4), v0=None):
    """n envs of the fixture's robot at random positions within +-2 m, the fixture's attitudes / body rates / motor state, moving
    at `speed` (in collision radii per sub-step; 0.25 .. 0.4 r are 4.6 .. 7.4 m/s for the quadrotor) in a random direction, or at
    v0 [n, 3] where that is finite: consecutive sub-step positions are more than 0.2 r apart.  The velocity law is commanded to
    keep that velocity, the acceleration law a small acceleration; without a controller the fixture's motor commands."""
    g = load_golden("step_" + case)
    pd = golden_params(g)
    rng = np.random.default_rng(seed)
    idx = np.arange(n) % g["state"].shape[1]
    r = float(np.float32(pd["collision_radius"]))
    state = g["state"][0][idx].copy()
    state[:, 0:3] = rng.uniform(-2.0, 2.0, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    vel = d * rng.uniform(speed[0], speed[1], (n, 1)) * r / pd["dt"]
    if v0 is not None:
        vel = np.where(np.isfinite(v0), v0, vel)
    state[:, 7:10] = vel
    action = g["action"][0][idx].copy()
    if pd["controller"] == "velocity":  # the set-point is a vehicle-frame velocity (clipped to +-10 by the robot)
        yaw = _yaw(state[:, 3:7])
        vx, vy = state[:, 7].astype(np.float64), state[:, 8].astype(np.float64)
        action[:, 0], action[:, 1], action[:, 2] = np.cos(yaw) * vx + np.sin(yaw) * vy, -np.sin(yaw) * vx + np.cos(yaw) * vy, state[:, 9]
    elif pd["controller"] == "acceleration":
        action[:, 0:3] = rng.uniform(-1.0, 1.0, (n, 3))
    state, action = np.ascontiguousarray(state, np.float32), np.ascontiguousarray(action, np.float32)
    m = dict(case=case, pd=pd, k=k, r=r, thrust=g["thrust_in"][0][idx].copy(), kT=g["kT"][idx].copy(), tau_inc=g["tau_inc"][idx].copy(),
             tau_dec=g["tau_dec"][idx].copy(), gains=tuple(g[x][idx].copy() for x in ("Kp", "Kv", "KR", "Kw")))
    P = orc.make_params(pd)
    st, th = state.copy(), m["thrust"].copy()
    traj = np.zeros((k, n, 3), np.float32)
    for s in range(k):
        orc.substep(P, st, action.copy(), th, m["kT"], m["tau_inc"], m["tau_dec"], *m["gains"])
        traj[s] = st[:, 0:3]
    m.update(traj=traj, final_state=st, final_thrust=th)
    return state, action, m


def oracle_hits_per_substep(radius, traj, boxes):
    """[k, n] bool: orc.collide_sphere_boxes at each recorded sub-step position"""
    k, n = traj.shape[:2]
    out = np.zeros((k, n), bool)
    st = np.zeros((n, 13), np.float32)
    st[:, 6] = 1.0
    boxes = np.ascontiguousarray(boxes, np.float32)
    for s in range(k):
        st[:, 0:3] = traj[s]
        c = np.zeros(n, np.uint8)
        orc.collide_sphere_boxes(radius, st, boxes, c)
        out[s] = c > 0
    return out


def _finish(state, action, boxes, m, **family_meta):
    boxes = np.ascontiguousarray(boxes, np.float32)
    traj, r = m["traj"], m["r"]
    m["hits_per_substep"] = oracle_hits_per_substep(m["pd"]["collision_radius"], traj, boxes)
    expected = m["hits_per_substep"].any(0)
    d64 = obb_distance64(traj[:, :, None, :], boxes[None])  # [k, n, K]
    bound = separation_error_bound(traj[:, :, None, :], boxes[None], r)
    m["d64"], m["flags64"] = d64, (d64 < r).any((0, 2))
    m["ambiguous"] = (np.abs(d64 - r) <= bound).any((0, 2)) & ~(d64 < r - bound).any((0, 2))
    # the cull of the kernels in float64: the box's bounding sphere (+ r) reaches the AABB of the k positions
    lo, hi = traj.min(0).astype(np.float64)[:, None, :], traj.max(0).astype(np.float64)[:, None, :]
    c = boxes[..., 0:3].astype(np.float64)
    gap = np.linalg.norm(np.maximum(np.maximum(lo - c, c - hi), 0.0), axis=-1)
    m["passes_cull"] = gap < np.linalg.norm(boxes[..., 7:10].astype(np.float64), axis=-1) + r
    m.update(family_meta)
    for a in (state, action, boxes, expected, *(v for v in m.values() if isinstance(v, np.ndarray))):
        a.flags.writeable = False
    return state, action, boxes, expected, m


def _near_misses(rng, traj, r, K):
    """[n, K, 10] boxes (one long axis 0.3 .. 0.8 m, random orientation) that every one of the k positions misses by more than
    0.15 r while the bounding sphere reaches the trajectory's AABB: the cull lets them through and the predicate runs on them"""
    k, n = traj.shape[:2]
    out = np.zeros((n, K, 10), np.float32)
    todo = np.ones((n, K), bool)
    lo, hi = traj.min(0).astype(np.float64), traj.max(0).astype(np.float64)
    for _ in range(200):
        ei, bi = np.nonzero(todo)
        m = ei.size
        if m == 0:
            return out
        p = traj[rng.integers(0, k, m), ei]
        h = np.stack([rng.uniform(0.3, 0.8, m), rng.uniform(0.03, 0.1, m), rng.uniform(0.03, 0.1, m)], -1)
        axes_out = np.zeros((m, 3), bool)
        axes_out[:, 1] = True
        local = _outside_point(rng, h, r * rng.uniform(1.25, 1.6, m), axes_out)
        perm = np.argsort(rng.random((m, 3)), axis=-1)  # which axis is the long one
        h, local = np.take_along_axis(h, perm, -1), np.take_along_axis(local, perm, -1)
        b = _box(p, _rand_quat(rng, m), h, local)
        dmin = obb_distance64(traj[:, ei], b[None]).min(0)
        c = b[:, 0:3].astype(np.float64)
        gap = np.linalg.norm(np.maximum(np.maximum(lo[ei] - c, c - hi[ei]), 0.0), axis=-1)
        ok = (dmin > 1.15 * r) & (gap < np.linalg.norm(h, axis=-1) + r - 1.0e-3)
        out[ei[ok], bi[ok]] = b[ok]
        todo[ei[ok], bi[ok]] = False
    raise AssertionError("near-miss placement did not converge")


def _one_box(rng, traj_i, r, make, accept, tries=2000):
    """rejection sampling of one env's box: make(rng) -> row of 10, accept(distances of the k positions [k]) -> bool"""
    for _ in range(tries):
        b = make(rng)
        if accept(obb_distance64(traj_i, b[None])):
            return b
    raise AssertionError("box placement did not converge")


# ---------------------------------------------------------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------------------------------------------------------
def hit_index_classes(K):
    """name -> box index a hit is to be seen at: first and last box, first and last index of each residue mod 4 (the lane of the
    lane-quad kernel), first and last index of every batch trip K reaches (4 lanes x 16 boxes and 4 x 12)"""
    c = {"first": 0, "last": K - 1}
    for res in range(min(4, K)):
        c[f"lane{res}_first"], c[f"lane{res}_last"] = res, res + 4 * ((K - 1 - res) // 4)
    for per_lane in (16, 12):
        trip = 4 * per_lane
        for t in range((K + trip - 1) // trip):
            c[f"batch{per_lane}_trip{t}_first"], c[f"batch{per_lane}_trip{t}_last"] = t * trip, min((t + 1) * trip, K) - 1
    return c


@functools.lru_cache(maxsize=None)
def count_edges(K, case="quad_velocity", n=53, k=4, seed=1):
    """K boxes per env; env i with i % 3 != 1 is hit by exactly ONE of them (at 0.3 .. 0.85 r from a face, an edge or a corner, at one
    random sub-step), the index sweeping hit_index_classes(K); every other box is a near miss the cull lets through, except two
    parked at +-1e3 m when K >= 8.  The envs with i % 3 == 1 have no hit."""
    state, action, m = _base(case, n, k, seed)
    rng = np.random.default_rng(seed + 1000)
    traj, r = m["traj"], m["r"]
    boxes = _near_misses(rng, traj, r, K)
    idxs = sorted(set(hit_index_classes(K).values()))
    hit_env = np.nonzero(np.arange(n) % 3 != 1)[0]
    assert hit_env.size >= len(idxs), "too few envs for the hit-index sweep"
    hit_index = np.full(n, -1)
    hit_index[hit_env] = [idxs[j % len(idxs)] for j in range(hit_env.size)]
    parked = np.zeros((n, K), bool)
    if K >= 8:
        for i in range(n):
            free = np.setdiff1d(np.arange(K), [hit_index[i]])
            parked[i, rng.choice(free, 2, replace=False)] = True
        boxes[parked] = _parked(rng, int(parked.sum()))
    mh = hit_env.size
    hit_sub = rng.integers(0, k, mh)
    h = rng.uniform(0.05, 0.4, (mh, 3))
    axes_out = rng.random((mh, 3)) < 0.5
    axes_out[np.arange(mh), rng.integers(0, 3, mh)] = True
    local = _outside_point(rng, h, r * rng.uniform(0.3, 0.85, mh), axes_out)
    boxes[hit_env, hit_index[hit_env]] = _box(traj[hit_sub, hit_env], _rand_quat(rng, mh), h, local)
    return _finish(state, action, boxes, m, family="count_edges", hit_index=hit_index, parked=parked)


@functools.lru_cache(maxsize=None)
def all_misses(K, case="quad_velocity", n=53, k=4, seed=5):
    """K near misses per env that the cull lets through: a clean step"""
    state, action, m = _base(case, n, k, seed)
    boxes = _near_misses(np.random.default_rng(seed + 1000), m["traj"], m["r"], K)
    out = _finish(state, action, boxes, m, family="all_misses")
    assert not out[3].any()
    return out


@functools.lru_cache(maxsize=None)
def substep_only(k, s=None, case="quad_velocity", n=None, K=3, seed=2):
    """A tiny box (half extents 1e-3) 0.98 r to the side of the oracle position of sub-step s (env i: s = i % k when s is None;
    n = 2 k + 3 envs by default), at box index i % K among near misses: hit at sub-step s and at NO other, which the generator
    asserts with the oracle queried per sub-step.  (0.4 .. 0.55 r between consecutive positions: the neighbours of s are
    sqrt(0.98^2 + 0.4^2) r = 1.06 r away, less the box's 1.7e-3.)"""
    n = 2 * k + 3 if n is None else n
    state, action, m = _base(case, n, k, seed, speed=(0.4, 0.55))
    rng = np.random.default_rng(seed + 1000)
    traj, r = m["traj"], m["r"]
    boxes = _near_misses(rng, traj, r, K)
    s_env = np.arange(n) % k if s is None else np.full(n, s)
    env = np.arange(n)
    p = traj[s_env, env].astype(np.float64)
    chord = traj[np.minimum(s_env + 1, k - 1), env].astype(np.float64) - traj[np.maximum(s_env - 1, 0), env].astype(np.float64)
    chord /= np.linalg.norm(chord, axis=-1, keepdims=True)
    side = rng.normal(size=(n, 3))
    side -= (side * chord).sum(-1, keepdims=True) * chord
    side /= np.linalg.norm(side, axis=-1, keepdims=True)
    tiny = np.concatenate([p + 0.98 * r * side, _rand_quat(rng, n), np.full((n, 3), 1.0e-3)], axis=-1).astype(np.float32)
    boxes[env, env % K] = tiny
    out = _finish(state, action, boxes, m, family="substep_only", hit_substep=s_env)
    hps = m["hits_per_substep"]
    assert hps[s_env, env].all() and (hps.sum(0) == 1).all(), "a substep_only env is not hit at its sub-step alone"
    return out


ADVERSARY_PAIRS = ("beam_tip",) * 6 + ("slab_above", "slab_above", "slab_below", "slab_below", "robot_at_centre", "deep_inside",
                                        "fast_through", "fast_through")


@functools.lru_cache(maxsize=None)
def cull_adversaries(case="quad_velocity", k=4, K=5, seed=3):
    """Boxes whose CENTRE is far from the robot while a face is touched, and the other ways a cull goes wrong; env 2 j is the hit
    and env 2 j + 1 the near miss of pair j (0.9 r / 1.1 r from the touched feature at one sub-step, the last one in the even
    pairs; every other position of a near-miss env is more than 1.05 r away):
    * beam_tip: half extents (4, 0.03, 0.03), random rotation, touched at the end face;
    * slab_above / slab_below: (10, 10, 0.05), tilted by a few degrees, the robot anywhere over / under it;
    * robot_at_centre (small box) and deep_inside (3 m box): hits; their near miss is the same box 1.1 r off a face;
    * fast_through: 3.4 r per sub-step along a space diagonal; the hit touches one position, the near miss is a small box in the
      MIDDLE of the trajectory's AABB, between two positions.
    The other K - 1 boxes are parked at +-1e3 m; the adversary sits at index i % K."""
    n = 2 * len(ADVERSARY_PAIRS)
    g = load_golden("step_" + case)
    pd = golden_params(g)
    r = float(np.float32(pd["collision_radius"]))
    rng = np.random.default_rng(seed + 1000)
    v0 = np.full((n, 3), np.nan)
    for i in range(n):
        if ADVERSARY_PAIRS[i // 2] == "fast_through":
            d = rng.choice([-1.0, 1.0], 3) * np.array([1.0, 1.0, 0.6]) * rng.uniform(0.9, 1.1, 3)
            v0[i] = d / np.linalg.norm(d) * min(3.4 * r / pd["dt"], 0.95 * pd["max_linear_velocity"])
    state, action, m = _base(case, n, k, seed, v0=v0)
    traj = m["traj"]
    boxes = _parked(rng, n * K).reshape(n, K, 10)
    wants_hit, touch = np.arange(n) % 2 == 0, np.zeros(n, int)
    for i in range(n):
        j, kind, hit = i // 2, ADVERSARY_PAIRS[i // 2], bool(wants_hit[i])
        s = k - 1 if j % 2 == 0 else j % max(k - 1, 1)
        touch[i] = s
        ti = traj[:, i].astype(np.float64)
        sep = (0.9 if hit else 1.1) * r
        face = lambda rng, h, ax: _outside_point(rng, h[None], sep, (np.arange(3) == ax)[None])[0]  # noqa: E731
        if kind == "beam_tip":
            h = np.array([4.0, 0.03, 0.03])
            make = lambda rng: _box(ti[s], _rand_quat(rng, 1)[0], h, face(rng, h, 0))  # noqa: E731
        elif kind in ("slab_above", "slab_below"):
            h = np.array([10.0, 10.0, 0.05])
            def make(rng, h=h, up=kind == "slab_above"):
                tilt = rng.uniform(-0.05, 0.05, 3)
                q = np.array([tilt[0], tilt[1], tilt[2], 1.0])
                q = (q / np.linalg.norm(q)).astype(np.float32)
                local = rng.uniform(-0.9, 0.9, 3) * h
                local[2] = (h[2] + sep) * (1.0 if up else -1.0)
                height = ti @ rotmat64(q)[:, 2]  # the near miss is measured from the position closest to the slab
                at = ti[s] if hit else ti[np.argmin(height) if up else np.argmax(height)]
                return _box(at, q, h, local)
        elif kind in ("robot_at_centre", "deep_inside"):
            h = rng.uniform(0.1, 0.3, 3) if kind == "robot_at_centre" else np.full(3, 3.0)
            inside = np.zeros(3) if kind == "robot_at_centre" else rng.uniform(-1.0, 1.0, 3)
            make = lambda rng, h=h, inside=inside: _box(ti[s], _rand_quat(rng, 1)[0], h,  # noqa: E731
                                                          inside if hit else face(rng, h, int(rng.integers(0, 3))))
        else:  # fast_through
            h = np.full(3, 0.15 * r)
            at = ti[s] if hit else 0.5 * (ti.min(0) + ti.max(0))
            make = lambda rng, h=h, at=at: _box(at, _rand_quat(rng, 1)[0], h,  # noqa: E731
                                                 face(rng, h, int(rng.integers(0, 3))) if hit else np.zeros(3))
        accept = (lambda d: d[s] < 0.95 * r) if hit else (lambda d: d.min() > 1.05 * r)
        boxes[i, i % K] = _one_box(rng, ti, r, make, accept)
    out = _finish(state, action, boxes, m, family="cull_adversaries", wants_hit=wants_hit, pair_kind=ADVERSARY_PAIRS, touch_substep=touch)
    assert m["passes_cull"][np.arange(n), np.arange(n) % K][wants_hit].all(), "a touched box is culled in exact arithmetic"
    return out


@functools.lru_cache(maxsize=None)
def grazing(case="quad_velocity", k=4, K=4, seed=4, replicas=2):
    """One face or one corner of an axis-aligned or a rotated box at a separation of r (1 +- 2^-e), e = 16 .. 20, from the first or
    the last trajectory position (every other position more than 1.02 r away): 2 x 2 x 5 x 2 cases x `replicas`.  The centre is
    rounded to float32 (half an ulp of a 2 m coordinate is 1.2e-7 = r 2^-20.5): only the oracle defines the answer, and the
    generator asserts that each outcome occurs in at least a quarter of the cases.  The other boxes are near misses."""
    combos = [(feat, rot, e, sgn) for feat in ("face", "corner") for rot in (False, True) for e in range(16, 21) for sgn in (-1.0, 1.0)]
    n = len(combos) * replicas
    state, action, m = _base(case, n, k, seed)
    rng = np.random.default_rng(seed + 1000)
    traj, r = m["traj"], m["r"]
    boxes = _near_misses(rng, traj, r, K)
    for i in range(n):
        feat, rot, e, sgn = combos[i % len(combos)]
        s = (k - 1) if (i // len(combos) + i) % 2 == 0 else 0
        ti = traj[:, i].astype(np.float64)
        sep = r * (1.0 + sgn * 2.0 ** -e)

        def make(rng, feat=feat, rot=rot, s=s, ti=ti, sep=sep):
            h = rng.uniform(0.1, 0.5, 3)
            axes_out = np.ones(3, bool) if feat == "corner" else np.arange(3) == rng.integers(0, 3)
            q = _rand_quat(rng, 1)[0] if rot else np.array([0.0, 0.0, 0.0, 1.0], np.float32)
            return _box(ti[s], q, h, _outside_point(rng, h[None], sep, axes_out[None])[0])
        boxes[i, i % K] = _one_box(rng, ti, r, make, lambda d, s=s: np.delete(d, s).min(initial=np.inf) > 1.02 * r)
    out = _finish(state, action, boxes, m, family="grazing", combos=tuple(combos))
    share = out[3].mean()
    assert 0.25 <= share <= 0.75, f"grazing: {share:.2f} of the cases hit"
    return out


def cpu_families():
    """(name, family) of the shapes the CPU test checks: the ones the GPU tests run, without the 65 606-env instances"""
    fams = []
    for case in ("quad_velocity", "magpie_acceleration"):
        for K in (1, 2, 3, 4, 5, 63, 64, 65, 129):
            fams.append((f"count_edges[{case},K={K}]", count_edges(K, case)))
    for case in ("quad_velocity", "quad_no_control", "tinyprop_no_control"):
        for k in (1, 4):
            for K in (1, 2, 64, 65):
                fams.append((f"count_edges[{case},n=71,k={k},K={K}]", count_edges(K, case, 71, k)))
    for K in (3, 47, 48, 49, 97):
        fams.append((f"count_edges[octarotor_velocity,K={K}]", count_edges(K, "octarotor_velocity", 37)))
    for k in (2, 10, 32):
        fams.append((f"substep_only[k={k}]", substep_only(k)))
    fams.append(("cull_adversaries", cull_adversaries()))
    fams.append(("grazing", grazing()))
    fams.append(("cull_adversaries[quad_no_control]", cull_adversaries("quad_no_control")))
    fams.append(("grazing[quad_no_control]", grazing("quad_no_control")))
    fams.append(("all_misses", all_misses(5)))
    return fams
