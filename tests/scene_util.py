"""Test helper: synthetic box scenes in numpy (reference layout) for oracle and kernels."""
import numpy as np

BOX_VERTS = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]], np.float32) - 0.5
BOX_FACES = np.array([[1, 3, 0], [4, 1, 0], [0, 3, 2], [2, 4, 0], [1, 7, 3], [5, 1, 4], [5, 7, 1], [3, 7, 2], [6, 4, 2], [2, 7, 6],
                      [6, 5, 4], [7, 5, 6]])


def quat_from_euler(e):
    r, p, y = e[..., 0] * 0.5, e[..., 1] * 0.5, e[..., 2] * 0.5
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.stack([cy * sr * cp - sy * cr * sp, cy * cr * sp + sy * sr * cp, sy * cr * cp - cy * sr * sp,
                     cy * cr * cp + sy * sr * sp], axis=-1).astype(np.float32)


def random_box_scene(n, k_boxes, seed=0, bounds=((-2, -4, -3), (10, 4, 3)), walls=True):
    """Returns dict(tri_local [N,T,9], tri_asset [T], tri_seg [N,T], asset_state [N,K,13], half [N,K,3])."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(bounds[0], np.float32), np.array(bounds[1], np.float32)
    sizes = rng.uniform(0.1, 1.2, (n, k_boxes, 3)).astype(np.float32)
    pos = rng.uniform(lo, hi, (n, k_boxes, 3)).astype(np.float32)
    eul = np.zeros((n, k_boxes, 3), np.float32)
    eul[..., 2] = rng.uniform(-np.pi, np.pi, (n, k_boxes))
    if walls:
        wsz = np.array([[20, 0.2, 20], [20, 0.2, 20], [0.2, 20, 20], [0.2, 20, 20], [20, 20, 0.2], [20, 20, 0.2]], np.float32)
        mid = (lo + hi) / 2
        wpos = np.array([[mid[0], hi[1], mid[2]], [mid[0], lo[1], mid[2]], [lo[0], mid[1], mid[2]], [hi[0], mid[1], mid[2]],
                         [mid[0], mid[1], lo[2]], [mid[0], mid[1], hi[2]]], np.float32)
        sizes = np.concatenate([np.tile(wsz, (n, 1, 1)), sizes], axis=1)
        pos = np.concatenate([np.tile(wpos, (n, 1, 1)), pos], axis=1)
        eul = np.concatenate([np.zeros((n, 6, 3), np.float32), eul], axis=1)
    K = sizes.shape[1]
    tri = BOX_VERTS[BOX_FACES]  # [12,3,3]
    tri_local = (tri[None, None] * sizes[:, :, None, None, :]).reshape(n, 12 * K, 9).astype(np.float32)
    tri_asset = np.repeat(np.arange(K, dtype=np.int32), 12)
    seg = (100 + np.arange(n * K).reshape(n, K)).astype(np.int32)
    if walls:
        seg[:, :6] = np.array([11, 12, 10, 9, 13, 14], np.int32)
    state = np.zeros((n, K, 13), np.float32)
    state[..., 0:3] = pos
    state[..., 3:7] = quat_from_euler(eul)
    return dict(tri_local=np.ascontiguousarray(tri_local), tri_asset=tri_asset, tri_seg=np.ascontiguousarray(np.repeat(seg, 12, axis=1)),
                asset_state=state, half=np.ascontiguousarray(sizes * 0.5), bounds=(lo, hi))


def random_robot_states(n, seed, lo, hi, tilt=0.4):
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 13), np.float32)
    s[:, 0:3] = rng.uniform(lo + 0.5, hi - 0.5, (n, 3))
    e = rng.uniform(-1, 1, (n, 3)) * np.array([tilt, tilt, np.pi])
    s[:, 3:7] = quat_from_euler(e.astype(np.float32))
    return s


def golden_environment_assets(dest):
    """Writes the reference's obstacle URDFs kept in tests/golden/environment_assets.npz (oracle/gen_golden_environment_assets.py)
    back out as <dest>/{objects,panels,walls,trees,thin}/*.urdf and returns dest."""
    import os

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "environment_assets.npz"))
    for key in g.files:
        sub, name = key.split("__", 1)
        os.makedirs(os.path.join(dest, sub), exist_ok=True)
        with open(os.path.join(dest, sub, name), "w") as f:
            f.write(str(g[key]))
    return str(dest)


# ------------------------------------------------------------------------------------------------------------------------------
# Adversarial scenes for the LBVH builders and the box-face culling of the ray-cast (tests/test_gpu_bvh_limits.py,
# tests/test_oracle_raycast.py).  Everything is drawn from a seed: no fixture files.
PARKED = -1000.0  # where the curriculum parks an obstacle (asset_manager.py:71)
BOX_EPS = 1.0e-3  # kBoxEps: the builders grow every box by this much
CORNER_SIGNS = BOX_VERTS * 2.0  # corner i of trimesh's box in units of the half extents, i = 4 x + 2 y + z


def random_quats(rng, shape):
    """uniformly distributed unit quaternions (x, y, z, w) over all of SO(3) (Shoemake), float32, w >= 0"""
    u1, u2, u3 = (rng.random(shape) for _ in range(3))
    a, b = np.sqrt(1.0 - u1), np.sqrt(u1)
    q = np.stack([a * np.sin(2 * np.pi * u2), a * np.cos(2 * np.pi * u2), b * np.sin(2 * np.pi * u3), b * np.cos(2 * np.pi * u3)], axis=-1)
    q = np.where(q[..., 3:] < 0, -q, q)
    return (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(np.float32)


def quat_from_matrix(R):
    """unit quaternion (x, y, z, w), float32, of a rotation matrix (Shepperd: the largest of w, x, y, z first)"""
    R = np.asarray(R, np.float64)
    t = np.trace(R)
    cand = [t, R[0, 0], R[1, 1], R[2, 2]]
    i = int(np.argmax(cand))
    if i == 0:
        w = 0.5 * np.sqrt(1 + t)
        q = [(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w]
    else:
        a, b, c = i - 1, i % 3, (i + 1) % 3
        v = np.zeros(3)
        v[a] = 0.5 * np.sqrt(1 + R[a, a] - R[b, b] - R[c, c])
        v[b] = (R[b, a] + R[a, b]) / (4 * v[a])
        v[c] = (R[c, a] + R[a, c]) / (4 * v[a])
        q = [v[0], v[1], v[2], (R[c, b] - R[b, c]) / (4 * v[a])]
    q = np.array(q)
    return (q / np.linalg.norm(q)).astype(np.float32)


def quat_matrix(q):
    """rotation matrices (float64) of quaternions (x, y, z, w)"""
    q = np.asarray(q, np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def box_scene(centres, quats, extents, seg_base=100):
    """Boxes in trimesh face order from explicit per-env lists: centres [N,K,3], quats [N,K,4] (x, y, z, w), extents [N,K,3] (full
    edge lengths; 0 makes a zero-thickness slab).  Same dict as random_box_scene: local triangles (corners * extents) posed by
    asset_state, so the world-frame triangles come from the scene transform the product runs."""
    centres, quats, extents = (np.asarray(a, np.float32) for a in (centres, quats, extents))
    n, K = centres.shape[:2]
    tri = BOX_VERTS[BOX_FACES]
    tri_local = (tri[None, None] * extents[:, :, None, None, :]).reshape(n, 12 * K, 9).astype(np.float32)
    state = np.zeros((n, K, 13), np.float32)
    state[..., 0:3], state[..., 3:7] = centres, quats
    seg = (seg_base + np.arange(n * K).reshape(n, K)).astype(np.int32)
    lo, hi = centres.reshape(-1, 3).min(0), centres.reshape(-1, 3).max(0)
    return dict(tri_local=np.ascontiguousarray(tri_local), tri_asset=np.repeat(np.arange(K, dtype=np.int32), 12),
                tri_seg=np.ascontiguousarray(np.repeat(seg, 12, axis=1)), asset_state=state, half=np.ascontiguousarray(extents * 0.5),
                bounds=(lo, hi))


def random_rotated_boxes(rng, n, K, lo, hi, size_lo=0.1, size_hi=1.2):
    """(centres, quats, extents) of K boxes per env, uniform in [lo, hi], fully rotated, edges uniform in [size_lo, size_hi]"""
    c = rng.uniform(lo, hi, (n, K, 3)).astype(np.float32)
    return c, random_quats(rng, (n, K)), rng.uniform(size_lo, size_hi, (n, K, 3)).astype(np.float32)


def soup_scene(tris, seg_base=100):
    """[N,T,9] world-frame triangles as ONE asset at the identity pose (the transform then copies them bit for bit)"""
    tris = np.ascontiguousarray(tris, np.float32)
    n, T = tris.shape[:2]
    state = np.zeros((n, 1, 13), np.float32)
    state[..., 6] = 1.0
    seg = (seg_base + np.arange(n * T).reshape(n, T)).astype(np.int32)
    v = tris.reshape(-1, 3)
    return dict(tri_local=tris, tri_asset=np.zeros(T, np.int32), tri_seg=seg, asset_state=state, half=np.ones((n, 1, 3), np.float32),
                bounds=(v.min(0), v.max(0)))


def feature_point(kind, rng):
    """a point of trimesh's box in units of its half extents: 'corner' (one of the eight), 'edge' (on one of the twelve edges,
    away from its ends) or 'face' (on one of the six faces, away from its rim; 'centre' = the face's centre)"""
    p = CORNER_SIGNS[rng.integers(8)].astype(np.float64)
    if kind == "corner":
        return p
    if kind == "edge":
        p[rng.integers(3)] = rng.uniform(-0.9, 0.9)
        return p
    fixed = rng.integers(3)
    free = [a for a in range(3) if a != fixed]
    p[free] = 0.0 if kind == "centre" else rng.uniform(-0.9, 0.9, 2)
    return p


def ulp_shift(point, ulps, direction):
    """a displacement of `ulps` float32 ulps of the point's largest coordinate along the unit vector `direction` (float64; nominal:
    the float32 rounding of a box's centre and pose moves its features by a few ulps more)"""
    m = np.float32(np.abs(np.asarray(point, np.float64)).max())
    return ulps * float(np.spacing(m)) * np.asarray(direction, np.float64)


def aim_box(origin, direction, t, quat, extents, point, shift=(0.0, 0.0, 0.0)):
    """The centre that puts the box's local point `point` (units of the half extents, feature_point) at origin + t * direction
    (float64 arithmetic, rounded to float32 once), the box then moved by `shift` (world frame): the ray meets the box where
    `point` - R^T shift lies.  Pass ulp_shift(...) for a few float32 ulps, or (kBoxEps +- delta) * unit for the box tolerance."""
    o, d = np.asarray(origin, np.float64), np.asarray(direction, np.float64)
    target = o + t * d / np.linalg.norm(d)
    local = np.asarray(point, np.float64) * 0.5 * np.asarray(extents, np.float64)
    return (target - quat_matrix(quat) @ local + np.asarray(shift, np.float64)).astype(np.float32)


def box_corners_world(tri_world_e, K):
    """[K,8,3] world-frame corners (index 4 x + 2 y + z) of the K trimesh boxes of one env's transformed triangles"""
    t = np.asarray(tri_world_e).reshape(K, 12, 3, 3)
    out = np.zeros((K, 8, 3), t.dtype)
    for f, face in enumerate(BOX_FACES):
        for v, corner in enumerate(face):
            out[:, corner] = t[:, f, v]
    return out


def special_directions():
    """axis rays, rays with one component exactly 0 and rays with one component +-1e-30"""
    d = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0.6, 0.8, 0], [0, -0.6, 0.8], [-0.8, 0, -0.6],
         [0.6, 0.8, 1e-30], [0.6, -0.8, -1e-30], [1e-30, -0.6, 0.8], [-1e-30, 0.8, 0.6], [-0.8, 1e-30, -0.6], [0.8, -1e-30, 0.6],
         [1, 1e-30, 0], [1e-30, 0, -1], [0, -1, -1e-30], [0.6, 0, 0.8], [0, 0.8, -0.6]]
    return np.array(d, np.float32)


def ray_table(rng, first=None, h=8, w=40):
    """[h, w, 3] unit ray directions: `first` (aimed rays), the special directions, then uniform ones"""
    parts = ([np.asarray(first, np.float32)] if first is not None else []) + [special_directions()]
    n_fill = h * w - sum(len(p) for p in parts)
    assert n_fill >= 0
    g = rng.normal(size=(n_fill, 3))
    parts.append((g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32))
    rv = np.concatenate(parts)
    nrm = np.sqrt((rv.astype(np.float64) ** 2).sum(1, keepdims=True))
    return (rv / nrm).astype(np.float32).reshape(h, w, 3)


def chain_scene_centres(K, s=0.01):
    """centres on a geometric progression along each axis: centre j has ONE bit of the object-level build's 30-bit Morton code set
    (x bit j at code bit 3 j + 2, y at 3 j + 1, z at 3 j; j = 1..9 -- the three low bits are masked), so the sorted codes share ever
    longer prefixes: a chain of 27 levels, then the objects at the origin.  One object at (1023 s)^3 fixes the grid."""
    c = np.zeros((K, 3), np.float64)
    k = 0
    for j in range(9, 0, -1):
        for axis in range(3):
            c[k, axis] = (2 ** j + 0.5) * s  # the middle of cell 2^j of the 10-bit grid over [0, 1023 s]
            k += 1
    c[k] = 1023 * s
    return c.astype(np.float32)


def degenerate_scenes(rng, K):
    """one env per degeneracy of the Morton keys (names in order)"""
    names = ["all centres equal", "two clusters of equal centres", "geometric progression", "all parked", "all but one parked",
             "all but two parked", "wall slabs among small boxes", "deformed objects interleaved"]
    n = len(names)
    lo, hi = np.float32([-5, -5, -2.5]), np.float32([5, 5, 2.5])
    c, q, e = random_rotated_boxes(rng, n, K, lo, hi)
    c[0] = np.float32([1.3, -0.7, 0.4])
    e[0] = rng.uniform(0.1, 3.0, (K, 3))
    c[1, : K // 2], c[1, K // 2:] = np.float32([-1.5, 2.0, 0.5]), np.float32([2.5, -1.0, -0.5])
    c[2] = chain_scene_centres(K)
    e[2] = rng.uniform(0.2, 0.4, (K, 3))  # overlapping near the origin: packets that meet both children at every chain level
    c[3] = PARKED
    c[4, 1:] = PARKED
    c[5, 2:] = PARKED
    wall = np.float32([[20, 0.2, 20], [20, 0.2, 20], [0.2, 20, 20], [0.2, 20, 20], [20, 20, 0.2], [20, 20, 0.2]])
    c[6, :6] = np.float32([[0, 6, 0], [0, -6, 0], [-6, 0, 0], [6, 0, 0], [0, 0, -3], [0, 0, 3]])
    e[6, :6], q[6, :6] = wall, np.float32([0, 0, 0, 1])
    e[6, 6:] = rng.uniform(0.05, 0.5, (K - 6, 3))
    sc = box_scene(c, q, e)
    sc["tri_local"][7, 0:12 * K:24, 0:3] *= 1.3  # every other object: vertex 0 of its triangle 0 moved (not a box)
    deformed = np.zeros((n, K), bool)
    deformed[7, 0::2] = True
    return names, sc, deformed


AIM_ENVS = ["exact", "ulps", "box tolerance", "ulps at 1 km", "ulps at 5 km", "origin on a face", "origin on an edge",
            "origin inside a box", "origin 0.5 mm off a face", "origin in the plane of box faces", "origin 0.5 mm inside a face",
            "grazing edges at 1 km", "grazing edges at 5 km"]


def fibonacci_directions(m):
    i = np.arange(m) + 0.5
    z = 1 - 2 * i / m
    r, phi = np.sqrt(1 - z * z), np.pi * (1 + 5 ** 0.5) * i
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], -1)


def aimed_scene(K=245, seed=31):
    """K boxes per env, box k hit by LiDAR ray k at one of its corners, edge points, face points or face centres (float64 aim,
    tests/scene_util.py aim_box), moved off that point by float32 ulps or across the feature by kBoxEps +- delta (names: AIM_ENVS).
    The ulp offsets are nominal: they move the float64 centre, which is then rounded to float32 and posed by the float32 scene
    transform, a few ulps more either way.  The "origin ..." envs put the LiDAR on, in, 0.5 mm off or 0.5 mm inside an axis-aligned
    2 m box (box 0), where the axis rays of the table graze its faces; an origin inside a box within kBoxEps of a face behind it
    takes box_face_candidates' t_alt path with |t_enter| up to 2 eps."""
    rng = np.random.default_rng(seed)
    n = len(AIM_ENVS)
    rv = ray_table(rng, first=fibonacci_directions(K), h=9, w=32)
    dirs = rv.reshape(-1, 3)[:K].astype(np.float64)
    origin = np.zeros((n, 3), np.float64)
    origin[3], origin[4] = [600, -800, 0], [3000, -4000, 0]
    origin[5:] = [[1.25, 0.8, -0.325], [1.25, 1.5, -0.325], [0.5, 0.6, 0.1], [1.2505, 0.8, -0.325], [0.0, 1.5, 0.0], [1.2495, 0.8, -0.325],
                  [-300, 950, 0], [4000, 0, -3000]]
    flat_env, graze_envs = AIM_ENVS.index("origin in the plane of box faces"), (n - 2, n - 1)
    c = np.zeros((n, K, 3), np.float32)
    q = random_quats(rng, (n, K))
    e = np.zeros((n, K, 3), np.float32)
    aim = dict(t=np.zeros((n, K)), point=np.zeros((n, K, 3)), shift=np.zeros((n, K, 3)), ulps=np.zeros((n, K)))
    kinds = ["corner", "edge", "face", "centre"]
    for env in range(n):
        for k in range(K):
            t = float(np.exp(rng.uniform(np.log(1.0), np.log(25.0))))
            e[env, k] = rng.uniform(0.04, 0.12, 3) * t
            p = feature_point(kinds[k % 4], rng)
            u = np.cross(dirs[k], rng.normal(size=3))
            u /= np.linalg.norm(u)
            target = origin[env] + t * dirs[k]
            if env in (1, 3, 4):
                shift = ulp_shift(target, [-4, -2, -1, 1, 2, 4][k % 6], u)
            elif env == 2:
                shift = (BOX_EPS + [-1e-4, -1e-5, 1e-5, 1e-4][k % 4]) * u
            else:
                shift = np.zeros(3)
            c[env, k] = aim_box(origin[env], dirs[k], t, q[env, k], e[env, k], p, shift)
            aim["t"][env, k], aim["point"][env, k], aim["shift"][env, k] = t, p, shift
            aim["ulps"][env, k] = [-4, -2, -1, 1, 2, 4][k % 6] if env in (1, 3, 4) else 0
    box0 = [AIM_ENVS.index(name) for name in ("origin on a face", "origin on an edge", "origin inside a box", "origin 0.5 mm off a face",
                                              "origin 0.5 mm inside a face")]
    c[box0, 0], q[box0, 0], e[box0, 0] = [0.25, 0.5, -0.125], [0, 0, 0, 1], 2.0  # faces at x = 1.25, y = 1.5, z = 0.875 ...
    # the last env: axis-aligned boxes whose top (or bottom) face lies in the plane y = 1.5 of the origin, along the table's rays with
    # d_y = 0 or +-1e-30: those rays run IN the plane of the face and are accepted at its rim by the vertical face they cross
    flat = [i for i, d in enumerate(rv.reshape(-1, 3)[K:K + 20]) if abs(d[1]) <= 1e-30]
    k = 0
    for i in flat:
        d = rv.reshape(-1, 3)[K + i].astype(np.float64)
        for t, cy in ((2.0, 1.0), (4.0, 2.0), (6.5, 1.0)):  # y extent 1 m: faces at y = 1.5 exactly (0.5 + 1.0, 2.0 - 0.5)
            xz = origin[flat_env] + (t + 0.6) * d
            c[flat_env, k], q[flat_env, k], e[flat_env, k] = [xz[0], cy, xz[2]], [0, 0, 0, 1], [1.0, 1.0, 1.0]
            aim["t"][flat_env, k], aim["point"][flat_env, k], aim["shift"][flat_env, k] = t, 0.0, 0.0
            k += 1
    # the last two envs: ray k meets the edge between faces +x and +y of box k head-on to +x but at a small angle theta to +y
    # (sin theta 0.005 - 0.5), the box moved across the edge by -4 .. 4 float32 ulps.  Far from the world origin the object node's
    # record (frame, centre, half extents from rounded vertices) is off the triangles by ~ulp(1 km) = 6e-5 m (5 km: 5e-4 m): the face
    # the exact test accepts can then be crossed up to that / sin theta -- millimetres -- after the slab entry, which is what
    # box_face_candidates' window of 2 eps has to cover
    grng = np.random.default_rng(seed + 1)
    for env, size in zip(graze_envs, ((0.4, 1.0), (1.8, 3.0))):
        for k in range(K):
            d = dirs[k]
            e1 = np.cross(d, grng.normal(size=3))
            e1 /= np.linalg.norm(e1)
            sin = float(np.exp(grng.uniform(np.log(0.005), np.log(0.5))))
            cos = np.sqrt(1 - sin * sin)
            na, nb = -cos * d + sin * e1, -sin * d - cos * e1  # d . na = -cos, d . nb = -sin: the ray grazes face +y
            q[env, k] = quat_from_matrix(np.stack([na, nb, np.cross(na, nb)], axis=1))
            e[env, k] = grng.uniform(*size, 3)
            t = 6.0 * float(e[env, k].max())
            p = np.array([1.0, 1.0, grng.uniform(-0.8, 0.8)])
            ulps = [-4, -2, -1, 0, 1, 2, 4][k % 7]
            shift = ulp_shift(origin[env] + t * d, ulps, nb)
            c[env, k] = aim_box(origin[env], d, t, q[env, k], e[env, k], p, shift)
            aim["t"][env, k], aim["point"][env, k], aim["shift"][env, k], aim["ulps"][env, k] = t, p, shift, ulps
    return box_scene(c, q, e), rv, origin.astype(np.float32), aim


def closest_hit_f64(o, dirs, tris, far, chunk=64):
    """float64 Moller-Trumbore closest hit of rays (o [3], dirs [R,3]) against triangles [T,9].

    Returns t [R] (inf: a miss), face [R], clean [R], cos [R] and diam [R].  A ray is clean when its answer is unambiguous: no
    triangle edge lies within tol = 1e-5 (1 + t) of where the ray crosses that triangle's plane (for every triangle crossed in
    [-tol, far + tol]), the second-nearest hit is more than tol behind the first, and the first is not within tol of 0 or far.
    cos is |d . n| of the hit triangle (the cosine of incidence), diam its longest edge."""
    v = tris.reshape(-1, 3, 3).astype(np.float64)
    a, e1, e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    nrm = np.cross(e1, e2)
    area2 = np.linalg.norm(nrm, axis=1)
    edges = np.stack([v[:, 2] - v[:, 1], v[:, 0] - v[:, 2], v[:, 1] - v[:, 0]], 1)
    height = area2[:, None] / np.maximum(np.linalg.norm(edges, axis=2), 1e-300)  # distance of vertex i from the opposite edge
    o = np.asarray(o, np.float64)
    R = len(dirs)
    t_out, f_out, clean, cos_out, diam_out = np.full(R, np.inf), np.full(R, -1), np.ones(R, bool), np.zeros(R), np.zeros(R)
    diam = np.linalg.norm(edges, axis=2).max(1)
    for r0 in range(0, R, chunk):
        d = dirs[r0:r0 + chunk].astype(np.float64)
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        pvec = np.cross(d[:, None, :], e2[None])
        det = np.einsum("tk,rtk->rt", e1, pvec)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            s = o - a
            u = np.einsum("tk,rtk->rt", s, pvec) * inv
            qv = np.cross(s, e1)
            vv = np.einsum("rk,tk->rt", d, qv) * inv
            t = np.einsum("tk,tk->t", e2, qv)[None] * inv
            w = 1 - u - vv
        bary = np.stack([w, u, vv], -1)                       # weights of vertices 0, 1, 2
        dist = bary * height[None]                            # signed distance of the crossing from each edge (in the plane)
        tol = 1e-5 * (1 + np.abs(t))
        crossed = np.isfinite(t) & (t >= -tol) & (t <= far + tol)
        near_edge = crossed & (np.abs(dist) <= tol[..., None]).any(-1)
        degenerate = (area2[None] <= 1e-12) | ~np.isfinite(t)
        # a ray in (or within tol of) the plane of a triangle: |normal . (o - a)| small and the direction parallel
        in_plane = (np.abs((s * nrm).sum(1))[None] <= 1e-5 * area2[None]) & (np.abs(d @ nrm.T) <= 1e-5 * area2[None])
        hit = crossed & (dist >= 0).all(-1) & (t >= 0) & (t < far) & ~degenerate
        th = np.where(hit, t, np.inf)
        order = np.argsort(th, axis=1)[:, :2]
        t1 = np.take_along_axis(th, order[:, :1], 1)[:, 0]
        t2 = np.take_along_axis(th, order[:, 1:2], 1)[:, 0]
        tl = 1e-5 * (1 + np.where(np.isfinite(t1), t1, 0))
        ok = ~near_edge.any(1) & ~in_plane.any(1) & ~(np.isfinite(t1) & ((np.where(np.isfinite(t2), t2, 1e300) - t1 <= tl) | (t1 <= tl) | (far - t1 <= tl)))
        t_out[r0:r0 + chunk], f_out[r0:r0 + chunk] = t1, np.where(np.isfinite(t1), order[:, 0], -1)
        clean[r0:r0 + chunk] = ok
        f1 = order[:, 0]
        cos = np.abs((d * nrm[f1]).sum(1)) / np.maximum(area2[f1], 1e-300)
        cos_out[r0:r0 + chunk], diam_out[r0:r0 + chunk] = cos, diam[f1]
    return t_out, f_out, clean, cos_out, diam_out


# The float64 bound on t the aimed-ray tests assert, for a clean ray hit at an incidence cosine |d . n| >= T64_MIN_COS.  The
# watertight test forms A = v - o in float32 (relative error 2^-24 of |A| <= t + L, L the triangle's diameter), the sheared
# coordinates, the three 2 x 2 determinants with diff_product, T and det (three-term sums) and t = T / det: a handful of roundings,
# each <= 2^-24 (t + L) in the hit point's distance from the triangle's plane; 16 of them stay below 1e-6 (t + L).  Along the ray
# that distance is divided by |d . n| <= 1 / T64_MIN_COS = 2; the float32 direction (normalised twice) adds ~1 ulp, 1.2e-7 t.
#   |t - t64| <= 2e-6 (t + L) + 1.2e-7 t      (L <= 3 m in these scenes: of the order of 2e-6 t + 6e-6)
# Rays that graze their triangle (|d . n| < 0.5) stay in the hit / miss and segment checks only.
T64_MIN_COS = 0.5


def t64_bound(t, diam):
    return 2e-6 * (t + diam) + 1.2e-7 * t
