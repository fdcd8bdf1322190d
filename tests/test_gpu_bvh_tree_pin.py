"""The node blocks of the three LBVH builders, pinned bit for bit.

Frames never see the tree (closest hit over all triangles, ties by index), and the LDS triangle-level build and the global-memory
build run the SAME key, radix-tree, box-marking and child-reference code (csrc/agx_bvh_parts.h), so comparing one with the other
no longer tells a shared mistake from a correct tree.  tests/golden/bvh_tree_pin.json therefore holds, per case, the SHA-256 of
the int32 view of the node block as the builders of an EARLIER commit wrote it (the fixture names the commit: the last one in
which each builder carried its own copy of that code).  Small sizes: the rules go wrong at the edges, not at volume.

World-frame triangles go straight into agx_bvh_build / agx_bvh_build_large.  They come from numpy's default_rng().random() and
elementwise float64 arithmetic only (no libm function beyond sqrt, no matrix product), rounded once to float32: the same input
bits on every machine.  The node buffer is preset to a pattern, so records a builder leaves alone hash the same everywhere.

    python tests/test_gpu_bvh_tree_pin.py --write --commit <id> [--out <file>]
writes the fixture (or <file>) with the library AGX_LIB_PATH names.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "bvh_tree_pin.json")
DEV = "cuda:0"
FULL_SORT, BOX_OBJECTS, OBJECT_TREE, OBJECT_REF = 0x40000000, 0x20000000, 0x10000000, 0x40000000
LDS_MAX_TRIS, OBJ_TREE_MAX = 2944, 256
PARKED = -1000.0
PRESET = 0x5A5A5A5A
BOX_CORNERS = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)])  # index 4 x + 2 y + z
BOX_FACES = np.array([[1, 3, 0], [4, 1, 0], [0, 3, 2], [2, 4, 0], [1, 7, 3], [5, 1, 4], [5, 7, 1], [3, 7, 2], [6, 4, 2], [2, 7, 6],
                      [6, 5, 4], [7, 5, 6]])  # trimesh.creation.box

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------------ inputs
def soup(T, seed):
    """[3][T][9]: env 0 plain; env 1 with every fourth triangle parked at -1000 m; env 2 with one triangle across the whole scene
    (the large-primitive flag)"""
    rng = np.random.default_rng(seed)
    v0 = rng.random((3, T, 3)) * 12.0 - 6.0
    e1, e2 = rng.random((3, T, 3)) - 0.5, rng.random((3, T, 3)) - 0.5
    tris = np.concatenate([v0, v0 + e1, v0 + e2], -1)
    tris[1, ::4] = PARKED + rng.random((len(range(0, T, 4)), 9))
    tris[2, 1] = [-20.0, -19.0, -18.0, 20.0, 19.0, 18.0, 1.0, 2.0, 30.0]
    return np.ascontiguousarray(tris, np.float32)


def box_triangles(centre, quat, extents, shear=0.0):
    """[..., 12, 9] world-frame triangles of boxes in trimesh's vertex and face order; shear: x += shear * y in the box frame"""
    x, y, z, w = (quat[..., k, None] for k in range(4))
    nrm = np.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x / nrm, y / nrm, z / nrm, w / nrm
    R = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    lx, ly, lz = (BOX_CORNERS[:, k] * extents[..., k, None] for k in range(3))  # [..., 8]
    lx = lx + shear * ly
    corners = np.stack([centre[..., k, None] + R[k][0] * lx + R[k][1] * ly + R[k][2] * lz for k in range(3)], -1)  # [..., 8, 3]
    return corners[..., BOX_FACES, :].reshape(corners.shape[:-2] + (12, 9))


IDENTITY = np.array([0.0, 0.0, 0.0, 1.0])


def boxes(K, seed, variant):
    """[3][12 K][9] fully rotated boxes.
    variant "a": env 0 with every third object parked at -1000 m; env 1 with EVERY object parked; env 2 with a wall slab longer
                 than 0.75 of the extent of the sort centres (its own subtree under the root).
    variant "b": env 0 with two identical objects (equal codes: the presorted path finds the tie and the full sort runs); env 1
                 with a sheared object, not a box, among boxes (no object node; the object-level build gives it its five-node
                 subtree); env 2 with a parked object, a slab and boxes."""
    rng = np.random.default_rng(seed)
    c = rng.random((3, K, 3)) * np.array([12.0, 12.0, 6.0]) - np.array([6.0, 6.0, 3.0])
    q = rng.random((3, K, 4)) * 2.0 - 1.0
    e = rng.random((3, K, 3)) * 1.1 + 0.1
    slab_c, slab_e = np.array([0.25, 6.5, 0.5]), np.array([14.0, 0.2, 7.0])
    shear = np.zeros((3, K, 1))
    if variant == "a":
        c[0, ::3] = PARKED
        c[1] = PARKED + rng.random((K, 3)) * 4.0
        c[2, 0], q[2, 0], e[2, 0] = slab_c, IDENTITY, slab_e
    else:
        c[0, 1], q[0, 1], e[0, 1] = c[0, 0], q[0, 0], e[0, 0]
        shear[1, K - 1] = 0.3
        c[2, 0] = PARKED
        c[2, 1], q[2, 1], e[2, 1] = slab_c, IDENTITY, slab_e
    return np.ascontiguousarray(box_triangles(c, q, e, shear).reshape(3, 12 * K, 9), np.float32)


def nines(T, seed):
    """[3][T][9] objects of nine triangles each, none a box; env 1 with the first object parked"""
    rng = np.random.default_rng(seed)
    K = T // 9
    c = np.repeat(rng.random((3, K, 1, 3)) * 8.0 - 4.0, 9, axis=2).reshape(3, T, 3)
    tris = np.concatenate([c + rng.random((3, T, 3)) - 0.5 for _ in range(3)], -1)
    tris[1, :9] += PARKED
    return np.ascontiguousarray(tris, np.float32)


BOX_FORMS = [12, 12 | BOX_OBJECTS, 12 | BOX_OBJECTS | OBJECT_TREE]


def cases():
    """-> [(name, tris, forms of the LDS builders, forms of the large builder)]; the large builder ignores AGX_BVH_FULL_SORT and
    AGX_BVH_OBJECT_TREE, so it runs the forms that differ for it"""
    out = []
    for T in (2, 3, 5, 64, 65, 257):
        out.append((f"soup T={T}", soup(T, 1000 + T), [0], [0]))
    for K in (2, 3, 64, 65, 106):
        for v in "ab":
            out.append((f"boxes K={K} {v}", boxes(K, 2000 + K, v), BOX_FORMS + [f | FULL_SORT for f in BOX_FORMS], BOX_FORMS[:2]))
    for T in (18, 27):
        out.append((f"nines T={T}", nines(T, 3000 + T), [9, 9 | FULL_SORT], [9]))
    for T in (4097, 8193):  # two and four 4096-key sort tiles
        out.append((f"soup T={T}", soup(T, 1000 + T), [], [0]))
    out.append(("boxes K=342 a", boxes(342, 2342, "a"), [], BOX_FORMS[:2]))
    return out


def object_level(form, T):
    """object_level_build() of agx_scene.hip: the launch builds the tree over the objects, with its own record layout"""
    return (form & OBJECT_TREE) and (form & BOX_OBJECTS) and not (form & FULL_SORT) and T >= 24 and T // 12 <= OBJ_TREE_MAX


# ---------------------------------------------------------------------------------------------------------------------- builders
def build_all():
    """-> ({key: sha256 of the node block}, {key: node block as int32 [3][T - 1][16]} for the cases the tests look into)"""
    import torch

    from aerial_gym_simulator_amd import _lib

    lib = _lib.load()
    stream = _lib.current_stream(DEV)
    hashes, kept = {}, {}
    for name, tris, lds_forms, large_forms in cases():
        n, T = tris.shape[:2]
        tw = torch.from_numpy(tris).to(DEV)
        scratch = torch.full((int(lib.agx_bvh_large_scratch_bytes(n, T)),), 0xA5, dtype=torch.uint8, device=DEV)
        for builder, forms in (("lds", lds_forms), ("large", large_forms)):
            for form in forms:
                nodes = torch.full((n, T - 1, 16), PRESET, dtype=torch.int32, device=DEV)
                if builder == "lds":
                    code = lib.agx_bvh_build(n, T, form, tw.data_ptr(), None, nodes.data_ptr(), None, stream)
                else:
                    code = lib.agx_bvh_build_large(n, T, form, tw.data_ptr(), None, nodes.data_ptr(), None, scratch.data_ptr(),
                                                   scratch.numel(), stream)
                _lib.check(code, f"{builder} build of {name}, form {form:#x}")
                torch.cuda.synchronize()
                block = np.ascontiguousarray(nodes.cpu().numpy())
                key = f"{name} | {builder} {form:#x}"
                hashes[key] = hashlib.sha256(block.tobytes()).hexdigest()
                if name == "boxes K=65 b" and form & BOX_OBJECTS:
                    kept[key] = block
    return hashes, kept


@pytest.fixture(scope="module")
def built():
    return build_all()


@pytest.fixture(scope="module")
def pinned():
    with open(FIXTURE) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------------------------------- tests
def test_every_node_block_is_the_pinned_commits(built, pinned):
    hashes = built[0]
    assert sorted(hashes) == sorted(pinned["sha256"]), "the cases of the fixture are not the cases of this module"
    differ = [k for k in sorted(hashes) if hashes[k] != pinned["sha256"][k]]
    assert not differ, f"{len(differ)} of {len(hashes)} node blocks differ from commit {pinned['commit']}: {differ}"


def test_large_build_writes_the_lds_triangle_level_builds_blocks(built):
    """every case both builders accept, whole blocks (at the pinned commit they were equal in every byte); with the flags the
    large builder ignores, the LDS builder's full sort gives the presorted order's tree too"""
    hashes = built[0]
    compared = 0
    for name, tris, lds_forms, large_forms in cases():
        T = tris.shape[1]
        for form in lds_forms:
            if object_level(form, T):
                continue
            base = form & ~(FULL_SORT | OBJECT_TREE)
            assert base in large_forms
            assert hashes[f"{name} | lds {form:#x}"] == hashes[f"{name} | large {base:#x}"], (name, hex(form))
            compared += 1
    assert compared == 6 + 10 * 5 + 4


def test_a_sheared_object_gets_no_object_node(built):
    """the inputs do what their names say: in env 1 of variant "b" the boxes become object nodes, the sheared last object none.
    The exact count K - 1 holds for the object-level build only: the triangle-level builds make an object node where a node of
    the radix tree spans exactly one object's keys, which two objects in one Morton cell prevent -- the hashes pin those blocks."""
    K = 65
    for key, block in built[1].items():
        rec, first, stack = block[1], set(), [0]
        while stack:  # from the root: child references in slots 3 and 7, leaves negative
            node = stack.pop()
            for c in (int(rec[node, 3]), int(rec[node, 7])):
                if c >= 0 and c & OBJECT_REF:
                    first.add(int(rec[c & ~OBJECT_REF, 15]))  # an object node's record ends with its first triangle
                elif c >= 0:
                    stack.append(c)
        assert first and first <= set(range(0, 12 * (K - 1), 12)), key
        if "lds" in key and object_level(int(key.split()[-1], 16), 12 * K):
            assert len(first) == K - 1, key  # the object-level build recognises every box, whatever the keys are


# ------------------------------------------------------------------------------------------------------------ writing the fixture
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    assert "--write" in sys.argv and "--commit" in sys.argv, __doc__
    commit = sys.argv[sys.argv.index("--commit") + 1]
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    hashes, _ = build_all()
    with open(out, "w") as f:
        json.dump({"commit": commit,
                   "what": "sha256 of the int32 view of the node block [3][T - 1][16] (preset to 0x5A5A5A5A) that the builders of "
                           "`commit` wrote for each case of tests/test_gpu_bvh_tree_pin.py; key: case | builder prims_per_object",
                   "sha256": hashes}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(hashes)} hashes -> {out}")
