"""The ray-cast launch mapping: every workgroups-per-image split, many tiles per wave.

k_raycast (csrc/agx_raycast.hip) cuts an (env, sensor) image into `split` workgroups of 4 waves; a wave walks its tiles with a stride
of split * 4.  At the sizes of the other bit-exact tests the launch policy clamps `split` to the image's tile count / 4, so a wave
owns at most one tile there; production batches run 2 - 4 tiles per wave.  agx_set_option("ray_split", n) forces the split: with
split = 1 on a handful of envs, four waves walk every tile of an image -- the production regime at a size the brute-force oracle
handles in milliseconds.

Every frame here is compared BIT FOR BIT (uint32 views of the pixels, equality of segmentation / face ids) with the oracle's brute
force over all triangles (use_bvh=False), for each of the five kernel instances (<camera | LiDAR> x <BASIC | NORMAL>, camera STEREO),
under every split, with partial tiles, several sensors per env and a short last group of 8 images.  The outputs are launched into
canary-filled buffers with a guard env on either side: a pixel nobody wrote, or a write outside the image block, fails the test.
The loop trips per wave and the launched grid (agx_raycast_kernel) are asserted, so the regime is really reached."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from scene_util import quat_matrix, random_box_scene, ray_table, soup_scene
from test_gpu_bvh_limits import Brute
from test_gpu_raycast import Scene, T, _poses

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CANARY_PX = 0x7FC5A5A5  # a quiet NaN with a payload: no frame holds it (the kernels store distances, points, normals, +-1, 1000)
CANARY_SEG = -12345     # segmentation ids are >= 0 or -2, face ids >= -1
WAVES = 4               # kRayThreads / 64
FAR = 4.0               # no walls and a far plane of 4 m: every frame has hits and misses
HFOV = 87.0
BASELINES = (0.095, 0.3)
LIMITS = (1.0, 3.0, 3.0, -1.0)  # min_range, max_range, far_oor, near_oor: both limits bite under the 4 m far plane
BASIC, NORMAL, STEREO = 0, 1, 2  # agx_raycast_kernel's `variant`

# (n, ns) -> (boxes, scene seed, camera pose seed, LiDAR pose seed): every env its own geometry, every (env, sensor) its own pose.
# 6 images: one short group of 8; 9: the second group holds one; 8: exactly one group; 17: two groups and one image.
# The seeds were chosen on the CPU with the oracle alone so that the shares asserted by _shares() hold (>= 5 % hits, >= 5 % misses,
# >= 2 % occluded stereo pixels at either baseline); a seed picked blindly gave 0.7 - 1.6 % occluded pixels at 0.095 m.
BATCHES = {(3, 2): (25, 41, 8, 18), (3, 3): (26, 41, 8, 18), (8, 1): (29, 41, 8, 18), (17, 1): (27, 43, 10, 20)}
BOUNDS = ((-2, -2, -1.5), (3, 2, 1.5))
# width, height, tiles, max_split (8 x 8 tile)
CAMERA_SHAPES = [(37, 21, 15, 4), (64, 48, 48, 12), (9, 65, 18, 5), (8, 8, 1, 1)]
# height, width, tiles, max_split (16 x 4 tile)
LIDAR_SHAPES = [(6, 50, 8, 2), (48, 120, 96, 24), (4, 16, 1, 1)]


# ------------------------------------------------------------------------------------------------- the launch, restated
def ray_split_policy(images, tiles, lidar):
    fill = -(-16384 // (images * WAVES))
    local = tiles // (WAVES * (2 if lidar else 4))
    return max(fill, local)


def launch_shape(images, W, H, lidar, forced):
    """-> tiles, max_split, split, threads of the launch (csrc/agx_raycast.hip ray_launch_shape)"""
    tw, th = (16, 4) if lidar else (8, 8)
    tiles = -(-W // tw) * -(-H // th)
    max_split = -(-tiles // WAVES)
    split = forced if forced else ray_split_policy(images, tiles, lidar)
    split = min(max(split, 1), max_split)
    return tiles, max_split, split, -(-images // 8) * 8 * split * 64 * WAVES


def splits_for(max_split):
    """0 = the policy, then the forced values; max_split + 5 and the option's upper bound must clamp"""
    out = []
    for s in (0, 1, 2, 3, max_split - 1, max_split, max_split + 5, 1 << 20):
        if (s == 0 or s >= 1) and s not in out:
            out.append(s)
    return out


def launched_threads(S, ns, W, H, lidar, variant):
    buf = C.create_string_buffer(128)
    S.L.check(S.lib.agx_raycast_kernel(S.n, ns, W, H, int(lidar), variant, buf, 128), "agx_raycast_kernel")
    name = buf.value.decode()
    assert name.startswith(f"k_raycast<{'true' if lidar else 'false'},{variant}>_"), name
    return int(name.rsplit("_", 1)[1])


def use_split(S, ns, W, H, lidar, variant, forced, tiles_want, max_split_want):
    """force the split; the test's arithmetic == the issue's table == what the library launches -> loop trips per wave"""
    S.L.set_option("ray_split", forced)
    images = S.n * ns
    tiles, max_split, split, threads = launch_shape(images, W, H, lidar, forced)
    assert (tiles, max_split) == (tiles_want, max_split_want)
    if forced:
        assert split == min(max(forced, 1), max_split)
        assert threads == -(-images // 8) * 8 * split * 256
    assert launched_threads(S, ns, W, H, lidar, variant) == threads, (forced, split)
    trips = -(-tiles // (split * WAVES))
    if forced == 1 and tiles > WAVES:
        assert trips >= 2  # the multi-tile regime: a wave runs the loop body more than once
    return trips


# ------------------------------------------------------------------------------------------------- the guarded launcher
class Guarded:
    """Scene.camera / stereo / lidar into canary-filled outputs of n + 2 envs, the pointer to env 1 handed to the library.
    -> (pixels as int32 bits, segmentation or None) of the n envs, still on the device; asserts that both guard envs are
    untouched and that no canary is left inside."""

    def __init__(self, S):
        self.S = S

    def _out(self, ns, H, W, vec, seg):
        n = self.S.n
        px = torch.full((n + 2, ns, H, W) + ((3,) if vec else ()), CANARY_PX, dtype=torch.int32, device=DEV)
        sg = torch.full((n + 2, ns, H, W), CANARY_SEG, dtype=torch.int32, device=DEV) if seg else None
        return px, sg

    def _checked(self, px, sg):
        torch.cuda.synchronize()
        n = self.S.n
        for name, t, canary in (("pixels", px, CANARY_PX), ("segmentation", sg, CANARY_SEG)):
            if t is None:
                continue
            assert bool((t[0] == canary).all()) and bool((t[n + 1] == canary).all()), f"{name}: written outside the image block"
            left = t[1:n + 1] == canary
            if bool(left.any()):
                where = torch.nonzero(left)[0].tolist()
                raise AssertionError(f"{name}: {int(left.sum())} of {left.numel()} elements never written, first at {where}")
        return px[1:n + 1], (sg[1:n + 1] if sg is not None else None)

    def _nodes(self):
        return self.S.L.dptr(self.S.nodes) if self.S.nodes is not None else None  # nt == 1: the entry points take NULL

    def camera(self, W, H, kinv, far, cx, cy, mode, pos, quat, seg=True, limits=None):
        S, L, p = self.S, self.S.L, self.S.L.dptr
        ns = pos.shape[1]
        px, sg = self._out(ns, H, W, mode >= 2, seg)
        kin = (C.c_float * 4)(*[float(x) for x in kinv])
        tp, tq = T(pos), T(quat)
        L.check(S.lib.agx_raycast_camera(S.n, ns, W, H, kin, float(far), cx, cy, mode, p(tp), p(tq), p(S.tri_world), p(S.tri_seg),
                                         self._nodes(), S.nt, p(px[1:]), p(sg[1:]) if seg else None, S._lim(limits), S.stream))
        return self._checked(px, sg)

    def stereo(self, W, H, kinv, far, baseline, cx, cy, mode, pos, quat, limits=None):
        S, L, p = self.S, self.S.L, self.S.L.dptr
        ns = pos.shape[1]
        px, sg = self._out(ns, H, W, mode >= 2, True)
        kin = (C.c_float * 4)(*[float(x) for x in kinv])
        tp, tq = T(pos), T(quat)
        L.check(S.lib.agx_raycast_stereo_camera(S.n, ns, W, H, kin, float(far), float(baseline), cx, cy, mode, p(tp), p(tq),
                                                p(S.tri_world), p(S.tri_seg), self._nodes(), S.nt, p(px[1:]), p(sg[1:]),
                                                S._lim(limits), S.stream))
        return self._checked(px, sg)

    def lidar(self, rv, far, mode, pos, quat, seg=True, limits=None):
        S, L, p = self.S, self.S.L, self.S.L.dptr
        ns, H, W = pos.shape[1], rv.shape[0], rv.shape[1]
        px, sg = self._out(ns, H, W, mode != 0, seg)
        trv, tp, tq = T(rv), T(pos), T(quat)
        L.check(S.lib.agx_raycast_lidar(S.n, ns, W, H, p(trv), float(far), mode, p(tp), p(tq), p(S.tri_world), p(S.tri_seg),
                                        self._nodes(), S.nt, p(px[1:]), p(sg[1:]) if seg else None, S._lim(limits), S.stream))
        return self._checked(px, sg)


class Case:
    """one frame: how to launch it, the kernel instance that renders it and the oracle's frame (computed once)"""

    def __init__(self, name, variant, launch, ref_px, ref_seg):
        self.name, self.variant, self.launch = name, variant, launch
        self.ref_px, self.ref_seg = ref_px, ref_seg
        self.dev = (T(np.ascontiguousarray(ref_px).view(np.int32)), T(ref_seg) if ref_seg is not None else None)

    def check(self, G, W, lidar, what):
        px, sg = self.launch(G)
        if torch.equal(px, self.dev[0]) and (sg is None or torch.equal(sg, self.dev[1])):
            return
        got, ref = px.cpu().numpy(), np.ascontiguousarray(self.ref_px).view(np.int32)
        bad = (got != ref).reshape(got.shape[:4] + (-1,)).any(-1)
        if sg is not None:
            bad |= sg.cpu().numpy() != self.ref_seg
        e, s, y, x = np.argwhere(bad)[0]
        tw, th = (16, 4) if lidar else (8, 8)
        tile, lane = (y // th) * -(-W // tw) + x // tw, (y % th) * tw + x % tw
        raise AssertionError(f"{what}, {self.name}: {int(bad.sum())} of {bad.size} pixels differ from the brute force; first: env {e} "
                             f"sensor {s} pixel ({y}, {x}) = tile {tile} lane {lane}: got {got.view(np.float32)[e, s, y, x]}"
                             f"{'' if sg is None else ' / ' + str(int(sg[e, s, y, x]))}, want {self.ref_px[e, s, y, x]}"
                             f"{'' if sg is None else ' / ' + str(int(self.ref_seg[e, s, y, x]))}")


def _shares(hit, miss, one_tile, what, occluded=None):
    """the input conditions: >= 5 % hits and >= 5 % misses in every reference frame (>= 2 % occluded pixels in every stereo one).
    A one-tile image (8 x 8, 4 x 16: 64 rays per image) is not required to meet a share, only to hold both kinds."""
    if one_tile:
        assert hit.any() and miss.any(), what
        assert occluded is None or occluded.any(), what
        return
    assert hit.mean() >= 0.05 and miss.mean() >= 0.05, (what, hit.mean(), miss.mean())
    assert occluded is None or occluded.mean() >= 0.02, (what, occluded.mean())


def _images_differ(seg, what):
    """a frame written to the wrong image index must differ: no two images of the reference are equal"""
    flat = seg.reshape(seg.shape[0] * seg.shape[1], -1)
    for i in range(len(flat)):
        for j in range(i):
            assert not np.array_equal(flat[i], flat[j]), (what, i, j)


@functools.lru_cache(maxsize=None)
def _batch(n, ns):
    """the scene of a batch shape in both tree forms, the oracle on its world-frame triangles, camera and LiDAR poses"""
    import oracle as orc

    boxes, seed, cam_seed, lidar_seed = BATCHES[(n, ns)]
    sc = random_box_scene(n, boxes, seed=seed, bounds=BOUNDS, walls=False)
    tris = orc.scene_transform(sc["tri_local"], sc["tri_asset"], sc["asset_state"])
    scenes = {}
    for form in ("object tree", "triangle tree"):
        S = Scene(sc)
        if form == "triangle tree":
            S.ppo = 12
        S.build()
        assert np.array_equal(S.tri_world.cpu().numpy().view(np.uint32), tris.view(np.uint32))
        scenes[form] = S
    cam = _poses(orc, n, sc, cam_seed, S=ns)[4:]
    lid = _poses(orc, n, sc, lidar_seed, lidar=True, S=ns)[4:]
    return scenes, Brute(orc, tris, sc["tri_seg"]), cam, lid


def _run(scenes, cases, ns, W, H, lidar, tiles, max_split, what):
    """every case under every split on every tree form; -> {variant: the splits it ran under}"""
    ran = {}
    for form, S in scenes.items():
        G = Guarded(S)
        for forced in splits_for(max_split):
            for variant in sorted({c.variant for c in cases}):
                trips = use_split(S, ns, W, H, lidar, variant, forced, tiles, max_split)
                ran.setdefault(variant, set()).add(forced)
            for c in cases:
                c.check(G, W, lidar, f"{what}, {form}, ray_split {forced} ({trips} trips per wave)")
    S.L.set_option("ray_split", 0)
    return ran


def _batch_id(b):
    return f"{b[0]}envs_x{b[1]}"


# ---------------------------------------------------------------------------------------------------------------- the camera
@pytest.mark.parametrize("shape", CAMERA_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("batch", list(BATCHES), ids=_batch_id)
def test_camera_every_split_equals_the_brute_force(orc, batch, shape):
    """k_raycast<false, BASIC> and <false, NORMAL>: all six modes, depth without a segmentation image and depth through the fused
    range limits on the (3, 2) batch; depth and world normals on the others."""
    (n, ns), (W, H, tiles, max_split) = batch, shape
    scenes, B, (pos, quat), _ = _batch(n, ns)
    kinv, cx, cy = orc.camera_kinv(W, H, HFOV)
    full = batch == (3, 2)
    what = f"camera {W} x {H}, {n} envs x {ns}"
    cases = []
    for mode in (("depth", "range", "pointcloud", "pointcloud_world", "normal", "normal_world") if full else ("depth", "normal_world")):
        m = orc.MODE[mode]
        rp, rs = B.camera(W, H, kinv, FAR, cx, cy, mode, pos, quat)
        _shares(rs >= 0, rs < 0, tiles == 1, (what, mode))
        _images_differ(rs, (what, mode))
        cases.append(Case(mode, NORMAL if m >= 4 else BASIC, lambda G, m=m: G.camera(W, H, kinv, FAR, cx, cy, m, pos, quat), rp, rs))
        if mode == "depth" and full:
            cases.append(Case("depth, seg = NULL", BASIC, lambda G: G.camera(W, H, kinv, FAR, cx, cy, 1, pos, quat, seg=False), rp, None))
            assert (rp[rs >= 0] > LIMITS[1]).any() and (rp < LIMITS[0]).any() and ((rp >= LIMITS[0]) & (rp <= LIMITS[1])).any()
            for normalize in (True, False):
                lim = LIMITS + (normalize,)
                cases.append(Case(f"depth, fused limits, normalize {normalize}", BASIC,
                                  lambda G, lim=lim: G.camera(W, H, kinv, FAR, cx, cy, 1, pos, quat, limits=lim),
                                  orc.sensor_postprocess(rp.copy(), *LIMITS, normalize), rs))
    ran = _run(scenes, cases, ns, W, H, False, tiles, max_split, what)
    assert ran[BASIC] == ran[NORMAL] == set(splits_for(max_split))


@pytest.mark.parametrize("shape", CAMERA_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("batch", list(BATCHES), ids=_batch_id)
def test_stereo_every_split_equals_the_brute_force(orc, batch, shape):
    """k_raycast<false, STEREO>: the second (any-hit) traversal starts inside the tile loop.  Four modes at baselines of 0.095 and
    0.3 m and depth through the fused range limits on the (3, 2) batch; depth at 0.095 m on the others."""
    (n, ns), (W, H, tiles, max_split) = batch, shape
    scenes, B, (pos, quat), _ = _batch(n, ns)
    kinv, cx, cy = orc.camera_kinv(W, H, HFOV)
    full = batch == (3, 2)
    what = f"stereo {W} x {H}, {n} envs x {ns}"
    cases = []
    for baseline in (BASELINES if full else BASELINES[:1]):
        occluded_points = None
        for mode in (("depth", "range", "pointcloud", "pointcloud_world") if full else ("depth",)):
            m = orc.MODE[mode]
            rp, rs = B.stereo(W, H, kinv, FAR, baseline, cx, cy, mode, pos, quat)
            # an occluded pixel: distance -1 (seg -2).  In the sensor-frame cloud that is a point BEHIND the camera (-1 x the unit
            # ray, z < 0); the world-frame cloud casts the very same rays: its occluded pixels are the sensor-frame cloud's
            if m <= 1:
                occluded = rp == -1.0
            elif mode == "pointcloud":
                occluded = occluded_points = rp[..., 2] < 0
            else:
                occluded = occluded_points
            _shares(rs >= 0, (rs < 0) & ~occluded, tiles == 1, (what, mode, baseline), occluded)
            assert not (occluded & (rs >= 0)).any()
            _images_differ(rs, (what, mode))
            cases.append(Case(f"{mode}, baseline {baseline}", STEREO,
                              lambda G, m=m, b=baseline: G.stereo(W, H, kinv, FAR, b, cx, cy, m, pos, quat), rp, rs))
            if mode == "depth" and full and baseline == BASELINES[0]:
                assert (rp > LIMITS[1]).any() and (rp < LIMITS[0]).any() and ((rp >= LIMITS[0]) & (rp <= LIMITS[1])).any()
                for normalize in (True, False):
                    lim = LIMITS + (normalize,)
                    cases.append(Case(f"depth, baseline {baseline}, fused limits, normalize {normalize}", STEREO,
                                      lambda G, lim=lim, b=baseline: G.stereo(W, H, kinv, FAR, b, cx, cy, 1, pos, quat, limits=lim),
                                      orc.sensor_postprocess(rp.copy(), *LIMITS, normalize), rs))
    ran = _run(scenes, cases, ns, W, H, False, tiles, max_split, what)
    assert ran[STEREO] == set(splits_for(max_split))


# ----------------------------------------------------------------------------------------------------------------- the LiDAR
def _lidar_table(orc, H, W):
    if (H, W) == (48, 120):
        return orc.lidar_ray_table(48, 120, -180, 180, -45, 45)  # the LiDAR task's dome
    return ray_table(np.random.default_rng(100 * H + W), h=H, w=W)


@pytest.mark.parametrize("shape", LIDAR_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("batch", list(BATCHES), ids=_batch_id)
def test_lidar_every_split_equals_the_brute_force(orc, batch, shape):
    """k_raycast<true, BASIC> and <true, NORMAL>: five modes, range without a segmentation image and range through the fused range
    limits on the (3, 2) batch; range and sensor-frame normals on the others."""
    (n, ns), (H, W, tiles, max_split) = batch, shape
    scenes, B, _, (pos, quat) = _batch(n, ns)
    rv = _lidar_table(orc, H, W)
    full = batch == (3, 2)
    what = f"LiDAR {H} x {W}, {n} envs x {ns}"
    cases = []
    for mode in (("range", "pointcloud", "pointcloud_world", "normal", "normal_world") if full else ("range", "normal")):
        m = orc.MODE[mode]
        rp, rs = B.lidar(rv, FAR, mode, pos, quat)
        _shares(rs >= 0, rs < 0, tiles == 1, (what, mode))
        _images_differ(rs, (what, mode))
        cases.append(Case(mode, NORMAL if m >= 4 else BASIC, lambda G, m=m: G.lidar(rv, FAR, m, pos, quat), rp, rs))
        if mode == "range" and full:
            cases.append(Case("range, seg = NULL", BASIC, lambda G: G.lidar(rv, FAR, 0, pos, quat, seg=False), rp, None))
            assert (rp > LIMITS[1]).any() and (rp < LIMITS[0]).any() and ((rp >= LIMITS[0]) & (rp <= LIMITS[1])).any()
            for normalize in (True, False):
                lim = LIMITS + (normalize,)
                cases.append(Case(f"range, fused limits, normalize {normalize}", BASIC,
                                  lambda G, lim=lim: G.lidar(rv, FAR, 0, pos, quat, limits=lim),
                                  orc.sensor_postprocess(rp.copy(), *LIMITS, normalize), rs))
    ran = _run(scenes, cases, ns, W, H, True, tiles, max_split, what)
    assert ran[BASIC] == ran[NORMAL] == set(splits_for(max_split))


# ------------------------------------------------------------------------------------------- one, two and three triangles
def _tiny_scene(orc, nt, lidar, seed):
    """n = 3 envs x 2 sensors in front of nt triangles of their own, laid out in the frame of each env's sensor 0 (axis a = the
    viewing direction: the camera's +z, the LiDAR's +x; u = the sensor's +x resp. +y -- the stereo partner sits at -u):
      triangle 0: the surface, 2 - 2.6 m away, circumradius 1.4 m, tilted;
      triangle 1: an occluder 1 m away, a little towards the partner: it shadows a strip of the surface for the partner;
      triangle 2: a larger one 3 m away, half of it behind the surface.
    -> soup scene, (pos, quat), the LiDAR's ray table (80 rays aimed into a 19-degree cone around +x, then ray_table's own)"""
    n, ns = 3, 2
    rng = np.random.default_rng(seed)
    box = dict(bounds=(np.float32([-2, -2, -1.5]), np.float32([3, 2, 1.5])))
    pos, quat = _poses(orc, n, box, seed, lidar=lidar, S=ns)[4:]
    R = quat_matrix(quat[:, 0])
    a, u = (R[:, :, 0], R[:, :, 1]) if lidar else (R[:, :, 2], R[:, :, 0])
    v = np.cross(a, u)
    tris = np.zeros((n, nt, 3, 3))
    layout = [(2.0, 0.0, 0.0, 1.4, 0.3), (1.0, -0.1, 0.05, 0.25, 0.05), (3.0, 0.8, 0.5, 1.5, 0.2)][:nt]
    for e in range(n):
        for k, (dist, du, dv, radius, tilt) in enumerate(layout):
            centre = pos[e, 0] + (dist + 0.3 * e * (k == 0)) * a[e] + du * u[e] + dv * v[e]
            th0 = rng.uniform(0, 2 * np.pi)
            for j in range(3):
                th = th0 + 2 * np.pi * j / 3
                tris[e, k, j] = centre + radius * (np.cos(th) * u[e] + np.sin(th) * v[e]) + rng.uniform(-tilt, tilt) * a[e]
    rv = None
    if lidar:
        off = rng.uniform(-0.35, 0.35, (80, 2))
        rv = ray_table(rng, first=np.concatenate([np.ones((80, 1)), off], axis=1), h=6, w=50)
    return soup_scene(tris.reshape(n, nt, 9)), (pos, quat), rv


def _build_tiny(sc):
    """nt = 1: the transform only and nodes = NULL (no tree); nt = 2, 3: the soup build (prims_per_object 0) into a node block
    with a guard env on either side"""
    S = Scene(sc)
    assert S.ppo == 0
    p, L = S.L.dptr, S.L
    L.check(S.lib.agx_scene_transform(S.n, S.nt, S.na, p(S.tri_local), p(S.tri_asset), p(S.asset_state), None, p(S.tri_world), S.stream))
    if S.nt == 1:
        S.nodes = None
    else:
        guarded = torch.full((S.n + 2, S.nt - 1, 16), CANARY_PX, dtype=torch.int32, device=DEV)
        S.nodes = guarded[1:S.n + 1].view(torch.float32)
        L.check(S.lib.agx_bvh_build(S.n, S.nt, 0, p(S.tri_world), None, p(S.nodes), p(S.work), S.stream))
        torch.cuda.synchronize()
        assert bool((guarded[0] == CANARY_PX).all()) and bool((guarded[S.n + 1] == CANARY_PX).all())
    torch.cuda.synchronize()
    assert np.array_equal(S.tri_world.cpu().numpy().view(np.uint32), sc["tri_local"].view(np.uint32))  # the identity pose copies
    return S


@pytest.mark.parametrize("nt", [1, 2, 3])
def test_scenes_of_one_two_and_three_triangles(orc, nt):
    """nt = 1: traverse() tests the one triangle without a node block (nodes == NULL); nt = 2, 3: the smallest trees of the LDS
    builder.  Camera depth / world points / normals, stereo depth (0.3 m; from nt = 2 on an occluder stands between the surface
    and the partner) at 37 x 21 and LiDAR range / world normals at 6 x 50, ray_split 0, 1 and max_split."""
    n, ns = 3, 2
    W, H, tiles, max_split = CAMERA_SHAPES[0]
    sc, (pos, quat), _ = _tiny_scene(orc, nt, False, 50 + nt)
    B = Brute(orc, sc["tri_local"], sc["tri_seg"])
    kinv, cx, cy = orc.camera_kinv(W, H, HFOV)
    far = 10.0
    cases = []
    for mode in ("depth", "pointcloud_world", "normal"):
        m = orc.MODE[mode]
        rp, rs = B.camera(W, H, kinv, far, cx, cy, mode, pos, quat)
        _shares(rs >= 0, rs < 0, False, ("camera", nt, mode))
        _images_differ(rs, ("camera", nt, mode))
        assert len(np.unique(rs[rs >= 0])) == (nt if m >= 4 else n * nt)  # every triangle of every env is in view (face / segment ids)
        cases.append(Case(f"camera {mode}", NORMAL if m >= 4 else BASIC, lambda G, m=m: G.camera(W, H, kinv, far, cx, cy, m, pos, quat), rp, rs))
    rp, rs = B.stereo(W, H, kinv, far, 0.3, cx, cy, "depth", pos, quat)
    occluded = rp == -1.0
    assert (rs >= 0).any() and ((rs < 0) & ~occluded).any()  # one triangle cannot hide itself: hits and misses only
    if nt >= 2:
        assert (occluded.reshape(n * ns, -1).sum(1) > 0).all()  # the occluder shadows the surface in every image
    cases.append(Case("stereo depth", STEREO, lambda G: G.stereo(W, H, kinv, far, 0.3, cx, cy, 1, pos, quat), rp, rs))
    S = _build_tiny(sc)
    what = f"{nt} triangle(s), camera {W} x {H}"
    for forced in (0, 1, max_split):
        for variant in (BASIC, NORMAL, STEREO):
            trips = use_split(S, ns, W, H, False, variant, forced, tiles, max_split)
        for c in cases:
            c.check(Guarded(S), W, False, f"{what}, ray_split {forced} ({trips} trips per wave)")

    H, W, tiles, max_split = LIDAR_SHAPES[0]
    sc, (pos, quat), rv = _tiny_scene(orc, nt, True, 60 + nt)
    B = Brute(orc, sc["tri_local"], sc["tri_seg"])
    cases = []
    for mode in ("range", "normal_world"):
        m = orc.MODE[mode]
        rp, rs = B.lidar(rv, far, mode, pos, quat)
        _shares(rs >= 0, rs < 0, False, ("LiDAR", nt, mode))  # the aimed rays: a random table alone gives 3 % hits
        _images_differ(rs, ("LiDAR", nt, mode))
        cases.append(Case(f"LiDAR {mode}", NORMAL if m >= 4 else BASIC, lambda G, m=m: G.lidar(rv, far, m, pos, quat), rp, rs))
    S = _build_tiny(sc)
    what = f"{nt} triangle(s), LiDAR {H} x {W}"
    for forced in (0, 1, max_split):
        for variant in (BASIC, NORMAL):
            trips = use_split(S, ns, W, H, True, variant, forced, tiles, max_split)
        for c in cases:
            c.check(Guarded(S), W, True, f"{what}, ray_split {forced} ({trips} trips per wave)")


# ------------------------------------------------------------------------------------------------------ the Python front end
def _frames_under_every_split(sensor, g, what):
    """the frozen state rendered through the sensor's own raycast call under ray_split 0, 1, 2 and 2^20, the images prefilled
    with canaries before every render: bit-identical frames, no canary left"""
    from aerial_gym_simulator_amd import _lib

    cfg = sensor.cfg
    tiles, _, split, _ = launch_shape(sensor.num_envs * sensor.num_sensors, cfg.width, cfg.height, sensor.is_lidar, 1)
    assert split == 1 and -(-tiles // WAVES) >= 2, what  # ray_split 1: several loop trips per wave
    px, seg = g["depth_range_pixels"], g["segmentation_pixels"] if sensor.segmentation_pixels is not None else None
    ref = None
    for forced in (0, 1, 2, 1 << 20):
        _lib.set_option("ray_split", forced)
        px.view(torch.int32).fill_(CANARY_PX)
        if seg is not None:
            seg.fill_(CANARY_SEG)
        sensor.raycast(fuse_limits=sensor.limits_fusable())
        torch.cuda.synchronize()
        assert not bool((px.view(torch.int32) == CANARY_PX).any()), (what, forced)
        assert seg is None or not bool((seg == CANARY_SEG).any()), (what, forced)
        img = (px.view(torch.int32).clone(), seg.clone() if seg is not None else None)
        if ref is None:
            ref = img
            assert len(torch.unique(img[0])) > 2, what  # a frame with content
        assert torch.equal(img[0], ref[0]) and (seg is None or torch.equal(img[1], ref[1])), (what, forced)
    _lib.set_option("ray_split", 0)


def test_front_end_frames_do_not_depend_on_ray_split():
    """navigation_task (depth camera, fused limits), lidar_navigation_task (48 x 120 world points) and the stereo and face-id /
    normal robots through SimBuilder: a few steps, then the same state rendered under every ray_split."""
    import random

    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.sim.sim_builder import SimBuilder
    from test_gpu_step_host_state import _task

    n = 8
    for name in ("navigation_task", "lidar_navigation_task"):
        with _task(name, n, args={"rng_seed": 99, "step_graph": False}) as task:
            task.reset()
            a = torch.rand(n, task.task_config.action_space_dim, device=DEV) * 2 - 1
            for _ in range(3):
                task.step(a)
            torch.cuda.synchronize()
            sensor = task.sim_env.robot_manager.warp_sensor
            assert sensor.is_lidar == (name == "lidar_navigation_task")
            if sensor.is_lidar:
                assert (sensor.cfg.height, sensor.cfg.width) == (48, 120) and sensor.cfg.pointcloud_in_world_frame
            else:
                assert sensor.limits_fusable()
            _frames_under_every_split(sensor, task.sim_env.global_tensor_dict, name)
    for robot in ("base_quadrotor_with_stereo_camera", "base_quadrotor_with_faceid_normal_camera"):
        random.seed(11)
        torch.manual_seed(11)
        env = SimBuilder().build_env("base_sim", "env_with_random_boxes", robot, "lee_velocity_control", DEV, num_envs=n,
                                     args={"rng_seed": 5})
        env.reset()
        a = torch.zeros(n, 4, device=DEV)
        for _ in range(3):
            env.step(actions=a)
            env.post_reward_calculation_step()
        g = env.get_obs()
        torch.cuda.synchronize()
        sensor = env.robot_manager.warp_sensor
        assert sensor.is_stereo == ("stereo" in robot) and sensor.is_normal == ("normal" in robot)
        _frames_under_every_split(sensor, g, robot)
