"""Ray casting at the limits of the two LDS-resident LBVH builders and on adversarial scenes.

Every scene is drawn from a seed here (tests/scene_util.py).  Each is built in every tree form that applies -- the object-level
tree (12 | AGX_BVH_BOX_OBJECTS | AGX_BVH_OBJECT_TREE), the triangle-level tree with object nodes (12 | AGX_BVH_BOX_OBJECTS), the
plain triangle-level tree (12) and the soup build (0) -- and every sensor output (camera depth / range / world points / normals +
face ids, stereo depth, LiDAR range and points through a ray table written here) must equal the oracle's brute force over all
triangles BIT FOR BIT.  The downloaded trees are walked (every triangle once, every child box holds its triangles, at most
kStackDepth = 64 internal levels: the traversal stack wraps silently beyond that), and the aimed-ray sets are pinned to a float64
Moller-Trumbore closest hit as well, so that the oracle is not the only judge."""
import numpy as np
import pytest
import torch
import scene_util as su
from scene_util import AIM_ENVS, aimed_scene, closest_hit_f64, degenerate_scenes, ray_table
from test_gpu_raycast import Scene, T, _walk_tree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

OBJ_TREE, OBJ_NODES, TRI_TREE, SOUP = 12 | 0x30000000, 12 | 0x20000000, 12, 0
BOX_FORMS = (OBJ_TREE, OBJ_NODES, TRI_TREE, SOUP)
STACK_DEPTH = 64  # kStackDepth of csrc/agx_raycast.hip
W, H, HFOV, BASELINE = 24, 16, 87.0, 0.3


class Brute:
    """the oracle's brute-force closest hit (use_bvh=False) behind the GPU Scene's sensor signatures"""

    def __init__(self, orc, tris, seg):
        self.orc, self.tris, self.seg = orc, tris, seg

    def camera(self, W, H, kinv, far, cx, cy, mode, pos, quat):
        return self.orc.raycast_camera(W, H, kinv, far, cx, cy, mode, pos, quat, self.tris, self.seg)

    def stereo(self, W, H, kinv, far, baseline, cx, cy, mode, pos, quat):
        return self.orc.raycast_stereo_camera(W, H, kinv, far, baseline, cx, cy, mode, pos, quat, self.tris, self.seg)

    def lidar(self, rv, far, mode, pos, quat):
        return self.orc.raycast_lidar(rv, far, mode, pos, quat, self.tris, self.seg)


def frames(R, orc, cam, lid, rv, far):
    """every sensor output of one launch: name -> (pixels, segmentation / face ids)"""
    kinv, cx, cy = orc.camera_kinv(W, H, HFOV)
    out = {}
    for name, mode in (("depth", 1), ("range", 0), ("pointcloud_world", 3), ("normal_world", 5)):
        out["camera " + name] = R.camera(W, H, kinv, far, cx, cy, mode, *cam)
    out["stereo depth"] = R.stereo(W, H, kinv, far, BASELINE, cx, cy, 1, *cam)
    out["stereo range, wide baseline"] = R.stereo(W, H, kinv, far, 2 * BASELINE, cx, cy, 0, *cam)
    for name, mode in (("range", 0), ("pointcloud", 2)):
        out["lidar " + name] = R.lidar(rv, far, mode, *lid)
    return out


def assert_frames_equal(got, ref, what):
    for k, (rp, rs) in ref.items():
        gp, gs = got[k]
        bad = (gp.view(np.uint32) != rp.view(np.uint32)).reshape(rs.shape + (-1,)).any(-1) | (gs != rs)
        if bad.any():
            e, s, y, x = np.argwhere(bad)[0]
            raise AssertionError(f"{what}, {k}: {int(bad.sum())} of {bad.size} pixels differ from the brute force; first: env {e} "
                                 f"pixel ({y}, {x}) got {gp[e, s, y, x]} / {gs[e, s, y, x]}, want {rp[e, s, y, x]} / {rs[e, s, y, x]}")


def look_at(orc, pos, target):
    """camera (pos, quat) [n,1,3] / [n,1,4] of a body at `pos` whose x axis points at `target`, x-forward camera frame"""
    pos, target = np.asarray(pos, np.float32), np.asarray(target, np.float32)
    d = (target - pos).astype(np.float64)
    e = np.stack([np.zeros(len(d)), -np.arctan2(d[:, 2], np.hypot(d[:, 0], d[:, 1])), np.arctan2(d[:, 1], d[:, 0])], -1)
    st = np.zeros((len(d), 13), np.float32)
    st[:, 0:3], st[:, 3:7] = pos, su.quat_from_euler(e.astype(np.float32))
    frame = orc.quat_from_euler(np.deg2rad(np.array([[-90.0, 0.0, -90.0]], np.float32)))[0]
    lq = np.tile(np.float32([0, 0, 0, 1]), (len(d), 1, 1))
    return orc.sensor_pose(st, np.zeros((len(d), 1, 3), np.float32), lq, frame)


def lidar_at(pos):
    pos = np.asarray(pos, np.float32).reshape(-1, 1, 3)
    return pos, np.tile(np.float32([0, 0, 0, 1]), (pos.shape[0], 1, 1))


def walk(S):
    """-> per env (object nodes, internal nodes visited, internal levels); every triangle reached exactly once"""
    nodes = S.nodes.cpu().numpy()
    NI = nodes.view(np.int32)
    tris = S.tri_world.cpu().numpy().reshape(S.n, -1, 3, 3)
    out = []
    for e in range(S.n):
        seen, objects, visited, depth = _walk_tree(nodes, NI, tris[e], e, S.nt)
        assert seen.min() == 1 and seen.max() == 1, (e, S.ppo)
        assert depth <= STACK_DEPTH, (e, S.ppo, depth)
        out.append((objects, visited, depth))
    return out


def check_scene(orc, sc, forms, cam, lid, rv, fars, what):
    """build in every form, walk the trees, every output of every far plane == brute force
    -> (world triangles, walks by form, brute-force frames by far plane, device frames by (form, far plane))"""
    tris = orc.scene_transform(sc["tri_local"], sc["tri_asset"], sc["asset_state"])
    B = Brute(orc, tris, sc["tri_seg"])
    ref = {far: frames(B, orc, cam, lid, rv, far) for far in fars}
    walks, got = {}, {}
    for form in forms:
        S = Scene(sc)
        S.ppo = form
        S.build()
        assert np.array_equal(S.tri_world.cpu().numpy().view(np.uint32), tris.view(np.uint32))
        walks[form] = walk(S)
        for far in fars:
            got[(form, far)] = frames(S, orc, cam, lid, rv, far)
            assert_frames_equal(got[(form, far)], ref[far], f"{what}, tree form {form:#x}, far plane {far}")
    return tris, walks, ref, got


# ---------------------------------------------------------------------------------------------------------------- object count
@pytest.mark.parametrize("K", [2, 3, 63, 64, 65, 127, 128, 129, 192, 245])
def test_object_count_across_the_four_waves(orc, K):
    """Phase 2 of the object-level build gives each object a lane of waves 0-3: K = 65 reaches wave 1, 129 wave 2, 192 / 245 wave 3
    (245 boxes = 2940 triangles, the largest box scene the ABI takes).  Envs: fully rotated boxes of 0.1-1.2 m, of 2 mm - 4 m, and
    the first scene again with the camera inside the cluster."""
    rng = np.random.default_rng(1000 + K)
    lo, hi = np.float32([-6, -6, -3]), np.float32([6, 6, 3])
    c, q, e = su.random_rotated_boxes(rng, 3, K, lo, hi)
    e[1] = np.exp(rng.uniform(np.log(0.002), np.log(4.0), (K, 3))).astype(np.float32)
    c[2], q[2], e[2] = c[0], q[0], e[0]
    sc = su.box_scene(c, q, e)
    pos = np.float32([[-9.0, 0.5, 0.8], [-9.0, -0.5, 1.5], [0.3, 0.2, 0.1]])
    cam = look_at(orc, pos, np.float32([[0, 0, 0], [0, 0, 0], [5, 1, -1]]))
    rv = ray_table(rng)
    _, walks, ref, _ = check_scene(orc, sc, BOX_FORMS, cam, lidar_at(pos), rv, (20.0,), f"K = {K}")
    objects, visited = (np.array([w[i] for w in walks[OBJ_TREE]]) for i in (0, 1))
    assert objects[0] == K and objects[2] == K  # every object is a recognised box: an object node
    assert 0.9 * K <= objects[1] <= K  # (a 2 mm x 4 m box is beyond the recognition's orthogonality tolerance: a five-node subtree)
    assert list(visited) == list((K - 1) + 5 * (K - objects))  # the tree over the objects: K - 1 internal nodes
    if K >= 63:  # the frames see the scene
        assert (ref[20.0]["camera depth"][1] >= 0).mean() > 0.1 and (ref[20.0]["lidar range"][1] >= 0).mean() > 0.03


def test_triangle_soup_at_the_limit(orc):
    """2944 triangles (kBvhMaxTris: the triangle-level build's 160 KiB of LDS) of a soup: slivers, zero-area and shared-vertex
    triangles, long ones across the scene; the soup build (prims_per_object = 0)."""
    rng = np.random.default_rng(2944)
    n, nt = 3, 2944
    v0 = rng.uniform(-6, 6, (n, nt, 3))
    tris = np.concatenate([v0, v0 + rng.normal(0, 0.4, (n, nt, 3)), v0 + rng.normal(0, 0.4, (n, nt, 3))], -1)
    tris[:, :200, 6:9] = tris[:, :200, 3:6]                                                 # zero area: two equal vertices
    tris[:, 200:400, 6:9] = 0.5 * (tris[:, 200:400, 0:3] + tris[:, 200:400, 3:6])           # zero area: collinear
    tris[:, 400:600, 3:6] = tris[:, 400:600, 0:3] + rng.normal(0, 1e-4, (n, 200, 3))         # slivers
    tris[:, 600:800, 0:3] = tris[:, 599:799, 3:6]                                           # shared vertices
    tris[:, 800:830, 3:6] = -tris[:, 800:830, 0:3]                                          # long ones across the scene
    sc = su.soup_scene(tris.astype(np.float32).reshape(n, nt, 9))
    pos = np.float32([[-9.0, 0.5, 0.8], [0.1, -0.2, 0.3], [8.0, 7.0, 2.0]])
    cam = look_at(orc, pos, np.zeros((n, 3), np.float32))
    _, walks, ref, _ = check_scene(orc, sc, (SOUP,), cam, lidar_at(pos), ray_table(rng), (20.0,), "2944-triangle soup")
    assert (ref[20.0]["camera depth"][1] >= 0).mean() > 0.3


# ------------------------------------------------------------------------------------------------------------ key degeneracies
# the longest root-to-leaf path of internal nodes the device builds on the geometric-progression env (measured, exact: the tree is
# a pure function of the keys); the chain alone is 27 levels
CHAIN_DEPTH = {129: {OBJ_TREE: 35, OBJ_NODES: 40, TRI_TREE: 40, SOUP: 28},
               245: {OBJ_TREE: 35, OBJ_NODES: 41, TRI_TREE: 41, SOUP: 29}}


@pytest.mark.parametrize("K", [129, 245])
def test_key_degeneracies(orc, K):
    rng = np.random.default_rng(77 + K)
    names, sc, deformed = degenerate_scenes(rng, K)
    n = len(names)
    pos = np.float32([[-8, 1, 1], [-8, 0, 1], [-2.5, -2.0, -1.5], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0.5, 0.3, 0.2], [-8, 0.5, 0.8]])
    tgt = np.float32([[1.3, -0.7, 0.4], [0, 0.5, 0], [1, 1, 1], [-1000] * 3, [-1000] * 3, [-1000] * 3, [5, 1, -1], [0, 0, 0]])
    tgt[4] = sc["asset_state"][4, 0, 0:3]
    tgt[5] = sc["asset_state"][5, 1, 0:3]
    cam = look_at(orc, pos, tgt)
    # the LiDAR also looks straight at the parked pile and at the boxes left in the env
    aim = (tgt - pos).astype(np.float64)
    aim[[0, 1, 2, 6, 7]] = rng.normal(size=(5, 3))
    rv = ray_table(rng, first=aim / np.linalg.norm(aim, axis=1, keepdims=True))
    _, walks, ref, _ = check_scene(orc, sc, BOX_FORMS, cam, lidar_at(pos), rv, (10.0, 3000.0), f"key degeneracies, K = {K}")
    parked = (sc["asset_state"][..., 0] == su.PARKED)
    boxes = (~parked & ~deformed).sum(1)
    objects, visited, depth = (np.array([w[i] for w in walks[OBJ_TREE]]) for i in range(3))
    assert list(objects) == list(boxes), names
    assert list(visited) == list((K - 1) + 5 * (K - boxes))  # K - 1 nodes over the objects, five under each that is not a box
    chain = {form: walks[form][names.index("geometric progression")][2] for form in BOX_FORMS}
    print("geometric progression: internal levels", chain, "all envs, object tree:", list(depth))
    assert chain[OBJ_TREE] >= 25
    assert chain == CHAIN_DEPTH[K]
    far = ref[3000.0]
    assert (far["lidar range"][1][3:6] >= 0).any(axis=(1, 2, 3)).all()  # the parked piles are hit within 3 km


# ------------------------------------------------------------------------------------------------------------------------ scale
def test_scale_sizes_slabs_translation_and_far_planes(orc):
    """Box edges from 2 mm to 40 m; slabs 1e-4 - 1e-2 m thick and of zero thickness; the first two scenes again, scene and sensors
    translated by 1 km and by 5 km (the stated range of the box-face culling is |coords| < 10 km); far planes of 10, 1 000 and
    3 000 m."""
    rng = np.random.default_rng(5000)
    K = 64
    lo, hi = np.float32([-10, -10, -10]), np.float32([10, 10, 10])
    c, q, e = su.random_rotated_boxes(rng, 6, K, lo, hi)
    e[0] = np.exp(rng.uniform(np.log(0.002), np.log(40.0), (K, 3)))
    e[1] = rng.uniform(0.5, 3.0, (K, 3))
    thin = rng.integers(3, size=K)
    e[1, np.arange(K), thin] = np.exp(rng.uniform(np.log(1e-4), np.log(1e-2), K))
    e[1, ::8, 2] = 0.0  # zero thickness
    shift = np.float32([[0, 0, 0], [0, 0, 0], [600, -800, 0], [600, -800, 0], [3000, 4000, 0], [-3000, 0, 4000]])
    for k in (2, 4):
        c[k], q[k], e[k] = c[0], q[0], e[0]
    for k in (3, 5):
        c[k], q[k], e[k] = c[1], q[1], e[1]
    c += shift[:, None, :]
    sc = su.box_scene(c, q, e)
    pos = np.float32([-14, 0.5, 0.8]) + shift
    cam = look_at(orc, pos, shift)
    check_scene(orc, sc, BOX_FORMS, cam, lidar_at(pos), ray_table(rng), (10.0, 1000.0, 3000.0), "scale")


# ------------------------------------------------------------------------------------------------------------------ aimed rays
def test_aimed_rays_at_corners_edges_and_faces(orc):
    """LiDAR rays aimed at the corners, edges and faces of fully rotated boxes (245 per env, 1-25 m away, edges 4-12 % of the
    distance), exactly and off by 1-4 float32 ulps or kBoxEps +- 1e-5 / 1e-4, at the origin and 1 / 5 km from it; origins on a face,
    on an edge, inside a box, 0.5 mm off and 0.5 mm inside a face and in the plane of faces, with axis rays and rays with a component
    of exactly 0 or +-1e-30; edges met at grazing angles 1 and 5 km from the origin.  Bit-exact against the brute force in every tree
    form, and every form's LiDAR frame pinned to the float64 closest hit on the rays whose answer is unambiguous:
        hit / miss and segment id equal;  |t - t64| <= 2e-6 (t + L) + 1.2e-7 t  (L the triangle's diameter)
    where the ray meets the triangle at an incidence cosine >= 0.5 (derivation at scene_util.t64_bound; grazing rays have the
    error divided by the cosine and stay in the hit / miss and segment checks)."""
    sc, rv, origin, _ = aimed_scene()
    n = len(AIM_ENVS)
    lid = lidar_at(origin)
    rng = np.random.default_rng(3)
    cam_pos = origin.copy()
    cam_tgt = origin + rng.normal(size=(n, 3)).astype(np.float32)
    near_box0 = [AIM_ENVS.index(name) for name in ("origin on a face", "origin on an edge", "origin inside a box", "origin 0.5 mm off a face")]
    cam_pos[near_box0] = np.float32([[2.0, 0.8, -0.3], [1.8, 1.2, 0.2], [2.3, 0.1, -0.6], [1.6, 0.5, 0.5]])  # 0.35 - 1 m from box 0
    cam_tgt[near_box0] = np.float32([0.25, 0.5, -0.125])
    cam = look_at(orc, cam_pos, cam_tgt)
    far = 100.0
    tris, walks, ref, got = check_scene(orc, sc, BOX_FORMS, cam, lid, rv, (far,), "aimed rays")
    K = sc["asset_state"].shape[1]
    assert [w[0] for w in walks[OBJ_TREE]][:3] == [K] * 3  # (at 1 and 5 km float32 no longer resolves many of them as boxes)
    # every form's device LiDAR frame against the float64 closest hit
    tw = tris.reshape(n, -1, 9)
    dirs = rv.reshape(-1, 3)
    checked = timed = 0
    for env in range(n):
        t64, f64, clean, cos, diam = closest_hit_f64(origin[env], dirs, tw[env], far)
        hit64 = np.isfinite(t64)
        want_seg = np.where(hit64, sc["tri_seg"][env][np.maximum(f64, 0)], -2)
        h = clean & hit64 & (cos >= su.T64_MIN_COS)
        for form in BOX_FORMS:
            dev_t, dev_seg = (a[env, 0].reshape(-1) for a in got[(form, far)]["lidar range"])
            assert np.array_equal((dev_seg >= 0)[clean], hit64[clean]), (AIM_ENVS[env], form)
            assert np.array_equal(dev_seg[clean], want_seg[clean]), (AIM_ENVS[env], form)
            err = np.abs(dev_t[h].astype(np.float64) - t64[h])
            assert (err <= 2e-6 * (t64[h] + diam[h]) + 1.2e-7 * t64[h]).all(), (AIM_ENVS[env], form, (err / su.t64_bound(t64[h], diam[h])).max())
        checked += int(clean.sum())
        timed += int(h.sum())
    assert checked > 0.4 * n * dirs.shape[0] and timed > 0.3 * checked


# ------------------------------------------------------------------------------------------------------------ refresh at the limit
def _refresh_case(n, density, seed):
    rng = np.random.default_rng(seed)
    K = 245
    lo, hi = np.float32([-6, -6, -3]), np.float32([6, 6, 3])
    c, q, e = su.random_rotated_boxes(rng, n, K, lo, hi)
    sc = su.box_scene(c, q, e)
    c2 = rng.uniform(lo, hi, (n, K, 3)).astype(np.float32)
    c2[:, ::7] = su.PARKED  # the new poses park some obstacles, too
    st2 = sc["asset_state"].copy()
    st2[..., 0:3], st2[..., 3:7] = c2, su.random_quats(rng, (n, K))
    mask = (rng.random(n) < density).astype(np.uint8)
    mask[0], mask[-1] = 1, 0
    return sc, st2, mask


@pytest.mark.parametrize("n,density,form", [(5, 0.3, OBJ_TREE), (5, 0.9, OBJ_TREE), (5, 0.5, OBJ_NODES), (2100, 0.05, OBJ_TREE),
                                            (2100, 0.8, OBJ_TREE)])
def test_scene_refresh_at_245_objects(orc, n, density, form):
    """agx_scene_refresh in one call == agx_scene_transform + agx_bvh_build (+ agx_boxes_from_assets) with the same mask, bit for bit
    for every env, at K = 245: n = 5 takes a workgroup per env, n = 2100 (> kDirectRefreshEnvs = 2048) the mask compaction and the
    persistent grid.  The frames of the refreshed envs (every env at n = 5, 16 of them at n = 2100, masked and clean) == brute force."""
    sc, st2, mask = _refresh_case(n, density, seed=n + int(100 * density))
    I = lambda t: t.view(torch.int32)  # noqa: E731
    out = []
    for one_call in (False, True):
        S = Scene(sc)
        S.ppo = form
        p, L = S.L.dptr, S.L
        bx = torch.full((S.na, 11, n), -7.0, device=DEV)
        S.build()
        L.check(S.lib.agx_boxes_from_assets(n, S.na, p(S.asset_state), p(S.half), None, p(bx), S.stream))
        S.asset_state.copy_(T(st2))
        mt = T(mask)
        if one_call:
            L.check(S.lib.agx_scene_refresh(n, S.nt, S.na, p(S.tri_local), p(S.tri_asset), p(S.asset_state), p(S.half), S.ppo, p(mt),
                                            p(S.tri_world), p(bx), p(S.nodes), p(S.work), S.stream))
        else:
            L.check(S.lib.agx_scene_transform(n, S.nt, S.na, p(S.tri_local), p(S.tri_asset), p(S.asset_state), p(mt), p(S.tri_world), S.stream))
            L.check(S.lib.agx_bvh_build(n, S.nt, S.ppo, p(S.tri_world), p(mt), p(S.nodes), p(S.work), S.stream))
            L.check(S.lib.agx_boxes_from_assets(n, S.na, p(S.asset_state), p(S.half), p(mt), p(bx), S.stream))
        torch.cuda.synchronize()
        out.append((I(S.tri_world).clone(), I(S.nodes).clone(), I(bx).clone()))
        if one_call:
            R = S
        del mt
    for a, b in zip(*out):
        for env in range(n):  # every env, bit for bit
            if a.shape[0] == n:
                assert torch.equal(a[env], b[env]), env
        if a.shape[0] != n:
            assert torch.equal(a, b)
    mixed = sc["asset_state"].copy()
    mixed[mask.astype(bool)] = st2[mask.astype(bool)]
    pick = np.arange(n) if n <= 16 else np.sort(np.concatenate([np.flatnonzero(mask)[:8], np.flatnonzero(~mask.astype(bool))[:8]]))
    assert mask[pick].any() and not mask[pick].all()
    tris = orc.scene_transform(sc["tri_local"][pick], sc["tri_asset"], mixed[pick])
    assert np.array_equal(out[1][0].cpu().numpy()[pick].view(np.float32), tris)
    pos = np.tile(np.float32([-9.0, 0.3, 0.5]), (n, 1))
    cam = look_at(orc, pos, np.zeros((n, 3), np.float32))
    kinv, cx, cy = orc.camera_kinv(W, H, HFOV)
    got = R.camera(W, H, kinv, 20.0, cx, cy, 1, *cam)
    want = orc.raycast_camera(W, H, kinv, 20.0, cx, cy, 1, cam[0][pick], cam[1][pick], tris, sc["tri_seg"][pick])
    assert np.array_equal(got[0][pick].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1][pick], want[1])
    rv = ray_table(np.random.default_rng(1))
    lid = lidar_at(pos)
    got = R.lidar(rv, 20.0, 0, *lid)
    want = orc.raycast_lidar(rv, 20.0, 0, lid[0][pick], lid[1][pick], tris, sc["tri_seg"][pick])
    assert np.array_equal(got[0][pick].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1][pick], want[1])
    assert (want[1] >= 0).mean() > 0.05
