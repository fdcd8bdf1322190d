"""The global-memory LBVH build (agx_bvh_build_large, csrc/agx_scene_large.hip) for scenes above the LDS builders' 2944 triangles.

The tree is a pure accelerator, so the criterion is the usual one: every sensor output equals the oracle's brute force over all
triangles BIT FOR BIT.  Scenes are drawn from seeds; the trees are walked (every triangle once, every child box holds its
triangles, at most kStackDepth = 64 internal levels); sizes sit on both sides of every threshold of the build: the 4096-key sort
tile, the LDS builders' cap, the power-of-two padding, the slab count of the persistent grid, and the cap itself."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import scene_util as su
import test_gpu_bvh_limits as bl
from scene_util import ray_table
from test_gpu_bvh_limits import Brute, assert_frames_equal, check_scene, frames, lidar_at, look_at
from test_gpu_raycast import Scene, T, _walk_tree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures", "assets")
OBJ_NODES, TRI_TREE, SOUP = 12 | 0x20000000, 12, 0
STACK_DEPTH = 64
I32 = lambda t: t.view(torch.int32)  # noqa: E731  (child slots hold int bits: compare bit patterns)
npy = lambda t: np.ascontiguousarray(t.detach().cpu().numpy())  # noqa: E731


class LargeScene(Scene):
    """test_gpu_raycast.Scene whose build() goes through agx_bvh_build_large"""

    def __init__(self, sc):
        super().__init__(sc)
        if self.ppo:
            self.ppo = OBJ_NODES  # (Scene's default carries AGX_BVH_OBJECT_TREE, which the large build accepts and ignores)
        need = int(self.lib.agx_bvh_large_scratch_bytes(self.n, self.nt))
        assert need > 0
        self.scratch = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)  # the build may not rely on zeroed scratch

    def build(self, mask=None):
        p, L = self.L.dptr, self.L
        self._mask_t = T(mask) if mask is not None else None
        mk = p(self._mask_t) if mask is not None else None
        L.check(self.lib.agx_scene_transform(self.n, self.nt, self.na, p(self.tri_local), p(self.tri_asset), p(self.asset_state),
                                             mk, p(self.tri_world), self.stream))
        L.check(self.lib.agx_bvh_build_large(self.n, self.nt, self.ppo, p(self.tri_world), mk, p(self.nodes), p(self.work),
                                             p(self.scratch), self.scratch.numel(), self.stream))
        torch.cuda.synchronize()


@pytest.fixture
def large(monkeypatch):
    """check_scene / walk of test_gpu_bvh_limits, building through the large builder"""
    monkeypatch.setattr(bl, "Scene", LargeScene)


def walk_levels(nodes_e, tris_e, nt):
    """_walk_tree, a whole level at a time: -> (times each triangle is reached, object nodes, internal nodes visited, internal
    levels on the longest path); checks every child box on the way"""
    OBJ = 0x40000000
    NI = nodes_e.view(np.int32)
    tv = tris_e.reshape(nt, 3, 3)
    seen = np.zeros(nt, np.int64)
    frontier, visited, objects, depth = np.zeros(1, np.int64), 0, 0, 0
    while frontier.size:
        depth += 1
        visited += frontier.size
        assert visited <= nt - 1 and depth <= 4 * STACK_DEPTH, "a node is reached twice"
        nxt = []
        for cslot, sslot, lo, hi in ((3, 11, slice(0, 3), slice(4, 7)), (7, 15, slice(8, 11), slice(12, 15))):
            c, s2 = NI[frontier, cslot].astype(np.int64), NI[frontier, sslot].astype(np.int64)
            blo, bhi = nodes_e[frontier, lo], nodes_e[frontier, hi]
            leaf = c < 0
            for f, m in ((~c, leaf), (s2, leaf & (s2 >= 0))):
                np.add.at(seen, f[m], 1)
                assert (tv[f[m]] >= blo[m][:, None] - 1e-6).all() and (tv[f[m]] <= bhi[m][:, None] + 1e-6).all()
            obj = ~leaf & ((c & OBJ) != 0)
            if obj.any():
                f0 = NI[c[obj] & ~OBJ, 15].astype(np.int64)
                fs = f0[:, None] + np.arange(12)
                np.add.at(seen, fs.reshape(-1), 1)
                v = tv[fs].reshape(len(f0), 36, 3)
                assert (v >= blo[obj][:, None] - 1e-6).all() and (v <= bhi[obj][:, None] + 1e-6).all()
                objects += int(obj.sum())
            inner = c[~leaf & ~obj]
            assert ((inner >= 0) & (inner < nt - 1)).all()
            nxt.append(inner)
        frontier = np.concatenate(nxt)
    return seen, objects, visited, depth


def soup(rng, n, nt, spread=6.0, size=0.4):
    v0 = rng.uniform(-spread, spread, (n, nt, 3))
    tris = np.concatenate([v0, v0 + rng.normal(0, size, (n, nt, 3)), v0 + rng.normal(0, size, (n, nt, 3))], -1)
    return tris.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("nt", [2, 3, 511, 513, 2945, 4096, 4097, 8193])
def test_soup_sizes(orc, large, nt):
    """2 and 3: the smallest trees; 511 / 513: around the thread count; 2945: one past the LDS builders' cap; 4096 / 4097: one sort
    tile, and two (the merge stages through global memory; 4097 pads to 8192 keys); 8193: four tiles."""
    rng = np.random.default_rng(nt)
    n = 2
    tris = soup(rng, n, nt, size=0.4 if nt > 100 else 4.0)
    if nt >= 511:
        tris[:, :40, 6:9] = tris[:, :40, 3:6]          # zero area
        tris[:, 40:60, 3:6] = -tris[:, 40:60, 0:3]     # long ones across the scene
    sc = su.soup_scene(tris)
    pos = np.float32([[-9.0, 0.5, 0.8], [0.1, -0.2, 0.3]])
    cam = look_at(orc, pos, np.zeros((n, 3), np.float32))
    _, walks, ref, _ = check_scene(orc, sc, (SOUP,), cam, lidar_at(pos), ray_table(rng), (20.0,), f"{nt}-triangle soup")
    S = LargeScene(sc)
    S.build()
    nodes, tw = npy(S.nodes), npy(S.tri_world)
    for e in range(n):  # the level-by-level walk the cap test relies on agrees with the per-node walk
        seen, objects, visited, depth = walk_levels(nodes[e], tw[e], nt)
        assert seen.min() == 1 and seen.max() == 1 and (objects, visited, depth) == walks[SOUP][e]
    if nt >= 511:
        assert (ref[20.0]["camera depth"][1] >= 0).mean() > 0.1


@pytest.mark.parametrize("K", [246, 342])
def test_box_scene_sizes(orc, large, K):
    """246 boxes = 2952 triangles: the first box scene the LDS builders refuse; 342 = 4104: across the 4096-key sort tile.  Triangle
    subtrees (12) and object nodes (12 | AGX_BVH_BOX_OBJECTS): every object is a recognised box."""
    rng = np.random.default_rng(K)
    n = 2
    c, q, e = su.random_rotated_boxes(rng, n, K, np.float32([-6, -6, -3]), np.float32([6, 6, 3]), size_hi=0.8)
    c[1, ::9] = su.PARKED  # the curriculum's parked obstacles
    sc = su.box_scene(c, q, e)
    pos = np.float32([[-9.0, 0.5, 0.8], [0.3, 0.2, 0.1]])
    cam = look_at(orc, pos, np.float32([[0, 0, 0], [5, 1, -1]]))
    _, walks, ref, _ = check_scene(orc, sc, (TRI_TREE, OBJ_NODES), cam, lidar_at(pos), ray_table(rng), (20.0,), f"K = {K}")
    parked = len(range(0, K, 9))
    assert walks[OBJ_NODES][0][0] == K and K - parked <= walks[OBJ_NODES][1][0] <= K and [w[0] for w in walks[TRI_TREE]] == [0, 0]
    assert (ref[20.0]["camera depth"][1] >= 0).mean() > 0.1


# ----------------------------------------------------------------------------------------------------------------------- the cap
def _cap_case(orc):
    rng = np.random.default_rng(65536)
    sc = su.soup_scene(soup(rng, 1, 65536, spread=8.0, size=0.15))
    pos = np.float32([[-12.0, 0.5, 0.8]])
    return sc, look_at(orc, pos, np.zeros((1, 3), np.float32)), lidar_at(pos), ray_table(rng)


def test_the_cap_65536_triangles(orc):
    """kBvhLargeMaxTris: sixteen sort tiles, ten merge stages through global memory, 2 MB of slab.  One camera depth frame and one
    LiDAR range frame; the oracle's own frame sees the scene (> 10 % of the pixels hit)."""
    sc, cam, lid, rv = _cap_case(orc)
    nt = 65536
    tris = orc.scene_transform(sc["tri_local"], sc["tri_asset"], sc["asset_state"])
    kinv, cx, cy = orc.camera_kinv(bl.W, bl.H, bl.HFOV)
    B = Brute(orc, tris, sc["tri_seg"])
    ref = {"camera depth": B.camera(bl.W, bl.H, kinv, 30.0, cx, cy, 1, *cam), "lidar range": B.lidar(rv, 30.0, 0, *lid)}
    assert (ref["camera depth"][1] >= 0).mean() > 0.1 and (ref["lidar range"][1] >= 0).mean() > 0.1
    S = LargeScene(sc)
    S.build()
    assert np.array_equal(npy(S.tri_world).view(np.uint32), tris.view(np.uint32))
    seen, objects, visited, depth = walk_levels(npy(S.nodes)[0], npy(S.tri_world)[0], nt)
    assert seen.min() == 1 and seen.max() == 1 and objects == 0
    print("65536-triangle soup: internal nodes visited", visited, "levels", depth)
    assert depth <= 48 <= STACK_DEPTH  # 31 + 16 key bits (+ 1 with the parked marker): the bound stated next to the cap
    got = {"camera depth": S.camera(bl.W, bl.H, kinv, 30.0, cx, cy, 1, *cam), "lidar range": S.lidar(rv, 30.0, 0, *lid)}
    assert_frames_equal(got, ref, "65536-triangle soup")


# ------------------------------------------------------------------------------------------------------------- key degeneracies
def test_key_degeneracies_at_4097_triangles(orc, large):
    """Soup envs whose Morton keys degenerate: every centroid exactly equal (the codes are equal: only the index word splits);
    every triangle parked at -1000 m (no bounds at all, every code the parked marker); sizes on a geometric progression from
    0.1 mm to 10 m (the large-primitive flag on a part of them); zero-area and sliver triangles among ordinary ones."""
    rng = np.random.default_rng(4097)
    nt = 4097
    tris = soup(rng, 4, nt)
    a, b = rng.normal(0, 1.5, (nt, 3)).astype(np.float32), rng.normal(0, 1.5, (nt, 3)).astype(np.float32)
    tris[0] = np.concatenate([a, b, -(a + b)], -1)  # (v0 + v1) + v2 == 0 exactly in float32, the order the build adds them in
    assert ((tris[0, :, 0:3] + tris[0, :, 3:6]) + tris[0, :, 6:9] == 0).all()
    tris[1] = (su.PARKED + rng.uniform(-3, 3, (nt, 9))).astype(np.float32)
    scale = (1e-4 * (1e5) ** (np.arange(nt) / (nt - 1)))[:, None]
    v0 = rng.uniform(-5, 5, (nt, 3))
    tris[2] = np.concatenate([v0, v0 + rng.normal(size=(nt, 3)) * scale, v0 + rng.normal(size=(nt, 3)) * scale], -1).astype(np.float32)
    tris[3, :1500, 6:9] = tris[3, :1500, 3:6]                                                     # zero area: two equal vertices
    tris[3, 1500:3000, 6:9] = 0.5 * (tris[3, 1500:3000, 0:3] + tris[3, 1500:3000, 3:6])           # zero area: collinear
    tris[3, 3000:3500, 3:6] = tris[3, 3000:3500, 0:3] + rng.normal(0, 1e-4, (500, 3))             # slivers; 597 ordinary ones stay
    sc = su.soup_scene(tris)
    pos = np.float32([[-6, 1, 1], [0, 0, 0], [-8, 0.5, 0.8], [-9, 0.5, 0.8]])
    tgt = np.float32([[0, 0, 0], [su.PARKED] * 3, [0, 0, 0], [0, 0, 0]])
    aim = (tgt - pos).astype(np.float64)
    rv = ray_table(rng, first=aim / np.linalg.norm(aim, axis=1, keepdims=True))
    _, walks, ref, _ = check_scene(orc, sc, (SOUP,), look_at(orc, pos, tgt), lidar_at(pos), rv, (3000.0,), "key degeneracies, 4097 triangles")
    depth = [w[2] for w in walks[SOUP]]
    print("internal levels:", depth)
    assert depth[0] == depth[1] <= 13  # equal codes: the tree over the 13 index bits of 4097 keys, whatever the code is
    hit = [(ref[3000.0]["camera depth"][1][e] >= 0).mean() for e in range(4)]
    assert hit[0] > 0.1 and hit[2] > 0.1 and hit[3] > 0.1, hit
    assert (ref[3000.0]["lidar range"][1][1] >= 0).any()  # the parked pile, 1.7 km away, through the aimed ray


# --------------------------------------------------------------------------------------------------- masked rebuild, the work list
def test_masked_rebuild_at_2945_triangles(orc):
    """After the scene has moved, a rebuild of envs 0 and 2 only: their triangles and nodes equal an unmasked build of the moved
    scene bit for bit, the clean envs keep theirs."""
    rng = np.random.default_rng(29450)
    n, nt = 5, 2945
    sc = su.soup_scene(soup(rng, n, nt))
    mask = np.uint8([1, 0, 1, 0, 0])
    S = LargeScene(sc)
    S.build()
    before = (I32(S.tri_world).clone(), I32(S.nodes).clone())
    moved = sc["asset_state"].copy()
    moved[:, 0, 0:3] = rng.uniform(-2, 2, (n, 3))
    moved[:, 0, 3:7] = su.random_quats(rng, (n,))
    S.asset_state.copy_(T(moved))
    S.build(mask)
    F = LargeScene(dict(sc, asset_state=moved))
    F.build()
    for e in range(n):
        want = (I32(F.tri_world), I32(F.nodes)) if mask[e] else before
        assert torch.equal(I32(S.tri_world)[e], want[0][e]) and torch.equal(I32(S.nodes)[e], want[1][e]), e
    mixed = np.where(mask.astype(bool)[:, None, None], moved, sc["asset_state"])
    tris = orc.scene_transform(sc["tri_local"], sc["tri_asset"], mixed)
    pos = np.tile(np.float32([-9.0, 0.3, 0.5]), (n, 1))
    cam = look_at(orc, pos, np.zeros((n, 3), np.float32))
    kinv, cx, cy = orc.camera_kinv(bl.W, bl.H, bl.HFOV)
    want = orc.raycast_camera(bl.W, bl.H, kinv, 20.0, cx, cy, 1, *cam, tris, sc["tri_seg"])
    got = S.camera(bl.W, bl.H, kinv, 20.0, cx, cy, 1, *cam)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
    assert (want[1] >= 0).mean() > 0.1


def test_work_list_reuses_slabs():
    """More dirty envs than slabs: the scratch stops growing at some env count G (one slab per resident workgroup); with G + 3 envs,
    all dirty, workgroups pull several envs each from the work list and reuse their slab.  Two-box scenes, 24 triangles."""
    from aerial_gym_simulator_amd import _lib

    f = _lib.load().agx_bvh_large_scratch_bytes
    G = next(g for g in range(1, 4096) if f(g, 24) == f(g + 1, 24))
    assert f(G, 24) == f(1 << 16, 24) and G <= 1024
    n = G + 3
    rng = np.random.default_rng(24)
    c, q, e = su.random_rotated_boxes(rng, n, 2, np.float32([-3, -3, -2]), np.float32([3, 3, 2]))
    sc = su.box_scene(c, q, e)
    A, Bm = LargeScene(sc), LargeScene(sc)
    A.build()
    Bm.nodes.fill_(-7.0)
    Bm.build(np.ones(n, np.uint8))
    assert torch.equal(I32(A.nodes), I32(Bm.nodes))
    nodes, tw = npy(A.nodes), npy(A.tri_world)
    for env in (0, 1, G - 1, G, n - 1):
        seen, objects, _, _ = _walk_tree(nodes, nodes.view(np.int32), tw[env].reshape(-1, 3, 3), env, 24)
        assert seen.min() == 1 and seen.max() == 1 and objects == 2


# ------------------------------------------------------------------------------------------------------------------- determinism
def test_three_builds_give_the_same_bits():
    rng = np.random.default_rng(81930)
    S = LargeScene(su.soup_scene(soup(rng, 2, 8193)))
    out = []
    for k in range(3):
        S.nodes.fill_(float(k))
        S.scratch.fill_(17 * k)
        S.build()
        out.append(I32(S.nodes).clone())
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], out[2])


# --------------------------------------------------------------------------------------------------- A/B against the LDS builders
def test_same_frames_and_trees_as_the_lds_builders_at_1272_triangles(orc):
    """The config-3 scene (100 boxes + 6 walls): frames from the large build == frames from the LDS build == brute force, for the
    triangle tree, the tree with object nodes and the soup build; and the node blocks are the LDS build's bit for bit (the same
    keys in the same order make the same tree, and min / max are exact in any order)."""
    n = 3
    sc = su.random_box_scene(n, 100, seed=7)
    assert sc["tri_local"].shape[1] == 1272
    rng = np.random.default_rng(1272)
    st = su.random_robot_states(n, 11, *sc["bounds"])
    cam = look_at(orc, st[:, 0:3], st[:, 0:3] + rng.normal(size=(n, 3)).astype(np.float32))
    lid, rv = lidar_at(st[:, 0:3]), ray_table(rng)
    tris = orc.scene_transform(sc["tri_local"], sc["tri_asset"], sc["asset_state"])
    ref = frames(Brute(orc, tris, sc["tri_seg"]), orc, cam, lid, rv, 10.0)
    for form in (TRI_TREE, OBJ_NODES, SOUP):
        got = []
        for cls in (Scene, LargeScene):
            S = cls(sc)
            S.ppo = form
            S.build()
            got.append((frames(S, orc, cam, lid, rv, 10.0), I32(S.nodes).clone()))
            assert_frames_equal(got[-1][0], ref, f"{cls.__name__}, tree form {form:#x}")
        assert torch.equal(got[0][1], got[1][1]), f"node blocks differ, tree form {form:#x}"
    assert (ref["camera depth"][1] >= 0).mean() > 0.3


# -------------------------------------------------------------------------------------------------------------------- end to end
def _asset_env_cfg(folder, count, file=None):
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config import asset_config as A
    from aerial_gym_simulator_amd.config.env_config import ForestEnvCfg

    class trees(A.tree_asset_params):
        num_assets = count
        asset_folder = os.path.join(FIX, folder)

    if file:
        trees.file = file

    class Cfg(ForestEnvCfg):
        class env_config:
            include_asset_type = {"trees": True, "objects": True, "bottom_wall": True}
            asset_type_to_dict_map = {"trees": trees, "objects": A.object_asset_params, "bottom_wall": A.bottom_wall}

    return Cfg


@pytest.mark.parametrize("name,folder,file,per_asset,prims", [("forest_env_three_trees13", "trees13", None, 13 * 132, 13),
                                                              ("three_balls_on_posts", "meshes", "ball_on_post.urdf", 132 + 1284, 2)])
def test_scenes_above_the_lds_cap_end_to_end(orc, name, folder, file, per_asset, prims):
    """forest_env with THREE 13-link trees (5580 triangles per env; SceneManager raised ValueError at 2944 before the large build),
    and a scene of three URDF spheres on posts (4680): reset, step, a partial reset, step -- triangles, depth and segmentation
    equal the oracle's, and the crash flags follow collide_sphere_boxes."""
    from aerial_gym_simulator_amd.registry.env_registry import env_config_registry
    from aerial_gym_simulator_amd.sim.sim_builder import SimBuilder

    random.seed(4)
    torch.manual_seed(4)
    env_config_registry.register(name, _asset_env_cfg(folder, 3, file))
    n = 4
    env = SimBuilder().build_env("base_sim", name, "base_quadrotor_with_camera_64x48", "lee_velocity_control", DEV, num_envs=n)
    sc = env.scene
    assert sc.num_prims == 1 + 3 * prims + 35 and sc.num_tris == 12 + 3 * per_asset + 35 * 12 > sc.MAX_TRIS_PER_ENV
    assert sc.large_build and sc.bvh_scratch is not None
    scratch_ptr = sc.bvh_scratch.data_ptr()
    env.reset()
    g = env.get_obs()
    a = torch.zeros(n, 4, device=DEV)
    env.step(actions=a)
    env.post_reward_calculation_step()
    env.reset_idx(torch.tensor([1, 3], device=DEV))  # a partial reset: the masked rebuild through the work list
    env.step(actions=a)
    env.post_reward_calculation_step()
    assert sc.bvh_scratch.data_ptr() == scratch_ptr  # allocated once
    tris = orc.scene_transform(npy(sc.tri_local), npy(sc.tri_asset), npy(sc.prim_state))
    assert np.array_equal(npy(sc.tri_world), tris)
    sen = env.robot_manager.warp_sensor
    kinv, cx, cy = orc.camera_kinv(64, 48, sen.cfg.horizontal_fov_deg)
    ref, ref_seg = orc.raycast_camera(64, 48, kinv, sen.cfg.max_range, cx, cy, "depth", npy(sen.sensor_position), npy(sen.sensor_orientation),
                                      tris, npy(sc.tri_seg))
    ref = orc.sensor_postprocess(ref, sen.cfg.min_range, sen.cfg.max_range, sen.cfg.far_out_of_range_value, sen.cfg.near_out_of_range_value,
                                 sen.cfg.normalize_range)
    seg = npy(g["segmentation_pixels"])
    assert np.array_equal(seg, ref_seg) and np.array_equal(npy(g["depth_range_pixels"]), ref)
    nodes = npy(sc.bvh_nodes)
    seen, _, _, depth = walk_levels(nodes[0], tris[0], sc.num_tris)
    assert seen.min() == 1 and seen.max() == 1 and depth <= STACK_DEPTH
    # crash flags: every robot into the centre of the first primitive of the first tree / shape of its env
    prim = npy(sc.prim_state)
    state = g["robot_state_tensor"]
    state[:, 0:3] = torch.from_numpy(prim[:, 1, 0:3]).to(DEV)
    state[:, 7:13] = 0.0
    env.step(actions=a)
    boxes = np.concatenate([prim[..., :7], npy(sc.half_extents)], axis=-1)
    crash_ref = np.zeros(n, np.uint8)
    orc.collide_sphere_boxes(env.robot_manager.robot.params_dict["collision_radius"], npy(state), np.ascontiguousarray(boxes), crash_ref)
    assert crash_ref.all() and np.array_equal(npy(g["crashes"]).astype(np.uint8), crash_ref)


# ---------------------------------------------------------------------------------------------------- forced large build: A/B runs
def test_forced_large_build_leaves_the_navigation_task_unchanged():
    """navigation_task, 16 envs, 20 steps, same seeds, with and without args={"bvh_large_build": True}: observations, rewards and
    flags bit-identical (the forced run builds triangle-level trees through agx_scene_refresh_large behind agx_reset_assets)."""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config import task_config as tc
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    cfg = tc.navigation_task_config
    old = (cfg.episode_len_steps, cfg.args, cfg.device)
    n, tasks = 16, []
    try:
        for forced in (False, True):
            random.seed(5)
            torch.manual_seed(5)
            cfg.device, cfg.episode_len_steps = DEV, 7
            cfg.args = {"rng_seed": 77, "bvh_large_build": forced}
            t = task_registry.make_task("navigation_task", seed=3, num_envs=n, headless=True)
            t.reset()
            tasks.append(t)
        plain, forced = tasks
        assert forced.sim_env.scene.large_build and not plain.sim_env.scene.large_build and plain.sim_env.scene.bvh_scratch is None
        gen = torch.Generator(device=DEV).manual_seed(2)
        for step in range(20):
            a = torch.rand(n, 4, device=DEV, generator=gen) * 2 - 1
            (o0, r0, te0, tr0, _), (o1, r1, te1, tr1, _) = (t.step(a) for t in (plain, forced))
            torch.cuda.synchronize()
            assert torch.equal(I32(o0["observations"]), I32(o1["observations"])), step
            assert torch.equal(I32(r0), I32(r1)) and torch.equal(te0, te1) and torch.equal(tr0, tr1), step
            for key in ("robot_state_tensor", "depth_range_pixels", "env_asset_state_tensor", "scene_tri_world"):
                assert torch.equal(I32(plain.obs_dict[key]), I32(forced.obs_dict[key])), (step, key)
            assert torch.equal(plain.sim_env.scene.boxes_soa, forced.sim_env.scene.boxes_soa), step
        assert int(forced.sim_env.global_tensor_dict["episode_count"].sum()) >= 2 * n  # resets happened
    finally:
        cfg.episode_len_steps, cfg.args, cfg.device = old


def test_forced_large_build_leaves_dynamic_env_unchanged():
    """dynamic_env with moving obstacles, 5 steps: the every-env refresh of each step through agx_scene_refresh_large"""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.sim.sim_builder import SimBuilder

    n, envs = 4, []
    for forced in (False, True):
        random.seed(3)
        torch.manual_seed(3)
        env = SimBuilder().build_env("base_sim", "dynamic_env", "base_quadrotor_with_camera_64x48", "lee_velocity_control", DEV,
                                     args={"bvh_large_build": forced, "rng_seed": 9}, num_envs=n)
        env.reset()
        envs.append(env)
    plain, forced = envs
    assert forced.scene.large_build and not plain.scene.large_build
    K = plain.scene.num_assets
    a = torch.zeros(n, 4, device=DEV)
    twist = torch.zeros(n, K, 6, device=DEV)
    twist[:, :, 0], twist[:, :, 5] = -1.0, 0.5
    twist[:, ::3, 1] = 0.7
    for step in range(5):
        for env in envs:
            env.step(actions=a, env_actions=twist)
            env.post_reward_calculation_step()
        torch.cuda.synchronize()
        g0, g1 = plain.get_obs(), forced.get_obs()
        for key in ("robot_state_tensor", "depth_range_pixels", "segmentation_pixels", "env_asset_state_tensor", "scene_tri_world", "crashes",
                    "truncations"):
            x, y = g0[key], g1[key]
            assert torch.equal(I32(x) if x.is_floating_point() else x, I32(y) if y.is_floating_point() else y), (step, key)
        assert torch.equal(plain.scene.boxes_soa, forced.scene.boxes_soa), step
    assert not torch.equal(plain.get_obs()["env_asset_state_tensor"][..., 0:3], torch.zeros_like(plain.get_obs()["env_asset_state_tensor"][..., 0:3]))


def test_forest_example_runs():
    """examples/forest_example.py (three trees13 trees per env through the large build) runs to completion"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, AGX_EXAMPLE_STEPS="40", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("AERIAL_GYM_RESOURCES", None)
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "forest_example.py")], env=env, capture_output=True, text=True,
                         timeout=300, cwd=root)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    assert "5580 triangles per env" in out.stdout and "large build: True" in out.stdout
