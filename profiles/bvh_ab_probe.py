"""A/B of the BVH builders: another build of the library (say the previous commit's, built with _build.build_library(lib_path=...))
against this tree's, interleaved region by region in one process.  Regions of `reps` launches between device events, 9 regions per
library and case; per case the medians, and whether the new median exceeds the other's by more than the other's min-max spread.
Cases: the soups of large_scene_probe.py, and the 106-box / 1272-triangle scene (build and masked refresh, direct and work-list).
    python profiles/bvh_ab_probe.py OTHER_LIBRARY.so [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from aerial_gym_simulator_amd import _build, _lib  # noqa: E402
import scene_util as su  # noqa: E402

DEV = "cuda:0"
BOX, TREE = 0x20000000, 0x10000000


def load(path):
    lib = C.CDLL(path)
    for name, (res, args) in _lib._SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


libs = {"parent": load(sys.argv[1]), "new": load(_build.LIB_PATH)}
p = _lib.dptr
stream = _lib.current_stream(DEV)
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731


def ab(name, launch, reps, regions=9):
    """launch(lib) -> error code"""
    st, sp = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for lib in libs.values():
        for _ in range(3):
            assert launch(lib) == 0, name
    torch.cuda.synchronize()
    out = {k: [] for k in libs}
    for _ in range(regions):
        for k, lib in libs.items():
            st.record()
            for _ in range(reps):
                launch(lib)
            sp.record()
            torch.cuda.synchronize()
            out[k].append(st.elapsed_time(sp) / reps * 1e3)
    row = {"case": name}
    for k, v in out.items():
        row[k] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
    row["new_minus_parent_us"] = round(row["new"]["median_us"] - row["parent"]["median_us"], 2)
    row["parent_spread_us"] = round(row["parent"]["max_us"] - row["parent"]["min_us"], 2)
    row["within_bar"] = row["new_minus_parent_us"] <= row["parent_spread_us"]
    print(json.dumps(row), flush=True)
    return row


rows = []
# ---- soups: the LDS build at its cap, the global-memory build at the same size and above (profiles/large_scene_probe.py's shapes)
N = 64
for nt, large in ((2944, False), (2944, True), (8192, True), (32768, True), (65536, True)):
    rng = np.random.default_rng(nt)
    v0 = rng.uniform(-8, 8, (N, nt, 3))
    size = 0.4 * (2944.0 / nt) ** 0.5
    tris = T(np.concatenate([v0, v0 + rng.normal(0, size, (N, nt, 3)), v0 + rng.normal(0, size, (N, nt, 3))], -1).astype(np.float32))
    nodes = torch.zeros(N, nt - 1, 16, device=DEV)
    if large:
        scratch = torch.zeros(int(libs["new"].agx_bvh_large_scratch_bytes(N, nt)), dtype=torch.uint8, device=DEV)
        rows.append(ab(f"agx_bvh_build_large soup T={nt} n={N}",
                       lambda lib: lib.agx_bvh_build_large(N, nt, 0, p(tris), None, p(nodes), None, p(scratch), scratch.numel(), stream),
                       20 if nt <= 8192 else 5))
    else:
        rows.append(ab(f"agx_bvh_build soup T={nt} n={N}", lambda lib: lib.agx_bvh_build(N, nt, 0, p(tris), None, p(nodes), None, stream), 20))
    del tris, nodes

# ---- the 106-box / 1272-triangle scene (100 boxes + 6 walls), object nodes and the object-level tree
for n, frac in ((512, 1.0), (4096, 0.1)):  # direct mode (a workgroup per env), persistent mode (work list)
    sc = su.random_box_scene(n, 100, seed=7)
    nt, na = sc["tri_local"].shape[1], sc["asset_state"].shape[1]
    assert nt == 1272
    tl, ta, st_, he = T(sc["tri_local"]), T(sc["tri_asset"]), T(sc["asset_state"]), T(sc["half"])
    tw = torch.zeros(n, nt, 9, device=DEV)
    nodes = torch.zeros(n, nt - 1, 16, device=DEV)
    boxes = torch.zeros(na, 11, n, device=DEV)
    work = torch.zeros(n + 2, dtype=torch.int32, device=DEV)
    mask_np = (np.random.default_rng(5).random(n) < frac).astype(np.uint8)
    mask = T(mask_np)
    assert libs["new"].agx_scene_transform(n, nt, na, p(tl), p(ta), p(st_), None, p(tw), stream) == 0
    torch.cuda.synchronize()
    for form, tag in ((12 | BOX, "12|BOX_OBJECTS"), (12 | BOX | TREE, "12|BOX_OBJECTS|OBJECT_TREE")):
        if frac == 1.0:
            rows.append(ab(f"agx_bvh_build boxes {tag} n={n} every env",
                           lambda lib: lib.agx_bvh_build(n, nt, form, p(tw), None, p(nodes), p(work), stream), 20))
        else:
            rows.append(ab(f"agx_bvh_build boxes {tag} n={n} masked {int(mask_np.sum())} dirty",
                           lambda lib: lib.agx_bvh_build(n, nt, form, p(tw), p(mask), p(nodes), p(work), stream), 20))
        rows.append(ab(f"agx_scene_refresh boxes {tag} n={n} masked {int(mask_np.sum())} dirty",
                       lambda lib: lib.agx_scene_refresh(n, nt, na, p(tl), p(ta), p(st_), p(he), form, p(mask), p(tw), p(boxes), p(nodes),
                                                         p(work), stream), 20))
    del tl, ta, st_, he, tw, nodes, boxes, work, mask

if len(sys.argv) > 2:
    json.dump({"build_id": libs["new"].agx_build_id().decode(), "other_build_id": libs["parent"].agx_build_id().decode(),
               "device": torch.cuda.get_device_name(0), "rows": rows}, open(sys.argv[2], "w"), indent=1)
print("all within bar:", all(r["within_bar"] for r in rows))
