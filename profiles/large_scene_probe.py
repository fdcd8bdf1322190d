"""The global-memory LBVH build (csrc/agx_scene_large.hip) against the LDS-resident one, and what a tree of that size costs a
frame: at 64 envs of a seeded triangle soup, the full build (every env) and one 64 x 48 camera depth frame, for
    2944 triangles (LDS build), 2944 (large build), 8192, 32768, 65536.
Each figure is the median of 5 timed regions of `reps` launches between device events, after a warm-up of every shape.
    python profiles/large_scene_probe.py [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aerial_gym_simulator_amd import _lib  # noqa: E402

DEV, N, W, H, HFOV, FAR = "cuda:0", 64, 64, 48, 87.0, 30.0
assert torch.cuda.is_available(), "this probe measures on the GPU"
lib, p = _lib.load(), _lib.dptr
stream = _lib.current_stream(DEV)


def soup(nt, seed):
    rng = np.random.default_rng(seed)
    v0 = rng.uniform(-8, 8, (N, nt, 3))
    size = 0.4 * (2944.0 / nt) ** 0.5  # the same covered area at every size
    t = np.concatenate([v0, v0 + rng.normal(0, size, (N, nt, 3)), v0 + rng.normal(0, size, (N, nt, 3))], -1)
    return torch.from_numpy(t.astype(np.float32)).to(DEV)


def median_ms(launch, reps):
    st, sp = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(2):
        launch()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        st.record()
        for _ in range(reps):
            launch()
        sp.record()
        torch.cuda.synchronize()
        out.append(st.elapsed_time(sp) / reps)
    return statistics.median(out), min(out), max(out)


# camera 12 m from the centre of the soup, looking at it (x-forward body, the reference's camera frame)
focal = (W / 2) / np.tan(np.deg2rad(HFOV) / 2)  # K_inv of warp_cam.py:31-64: {1 / fx, -cx / fx, 1 / fy, -cy / fy}, fx = fy
kinv = (C.c_float * 4)(1 / focal, -(W / 2) / focal, 1 / focal, -(H / 2) / focal)
pos = torch.tensor([-12.0, 0.5, 0.8], device=DEV).repeat(N, 1, 1).contiguous()
quat = torch.tensor([0.5, -0.5, 0.5, -0.5], device=DEV).repeat(N, 1, 1).contiguous()
rows = []
for nt, large in ((2944, False), (2944, True), (8192, True), (32768, True), (65536, True)):
    tris = soup(nt, nt)
    seg = torch.arange(N * nt, dtype=torch.int32, device=DEV).reshape(N, nt)
    nodes = torch.zeros(N, nt - 1, 16, device=DEV)
    work = torch.zeros(N + 2, dtype=torch.int32, device=DEV)
    px = torch.zeros(N, 1, H, W, device=DEV)
    sg = torch.zeros(N, 1, H, W, dtype=torch.int32, device=DEV)
    if large:
        scratch = torch.zeros(int(lib.agx_bvh_large_scratch_bytes(N, nt)), dtype=torch.uint8, device=DEV)
        build = lambda: _lib.check(lib.agx_bvh_build_large(N, nt, 0, p(tris), None, p(nodes), p(work), p(scratch), scratch.numel(), stream))  # noqa: E731
    else:
        scratch = None
        build = lambda: _lib.check(lib.agx_bvh_build(N, nt, 0, p(tris), None, p(nodes), p(work), stream))  # noqa: E731
    frame = lambda: _lib.check(lib.agx_raycast_camera(N, 1, W, H, kinv, FAR, W // 2, H // 2, 1, p(pos), p(quat), p(tris), p(seg), p(nodes), nt,  # noqa: E731
                                                      p(px), p(sg), None, stream))
    b = median_ms(build, 20 if nt <= 8192 else 5)
    f = median_ms(frame, 20)
    torch.cuda.synchronize()
    rows.append({"num_envs": N, "num_tris": nt, "builder": "global memory" if large else "LDS", "build_all_envs_ms": round(b[0], 4),
                 "build_ms_min_max": [round(b[1], 4), round(b[2], 4)], "camera_64x48_frame_ms": round(f[0], 4),
                 "frame_ms_min_max": [round(f[1], 4), round(f[2], 4)], "hit_fraction": round(float((sg >= 0).float().mean()), 3),
                 "scratch_MiB": round(scratch.numel() / 2**20, 1) if large else 0.0})
    print(json.dumps(rows[-1]), flush=True)
    del tris, seg, nodes, scratch
if len(sys.argv) > 1:
    json.dump({"build_id": _lib.build_id(), "device": torch.cuda.get_device_name(0), "rows": rows}, open(sys.argv[1], "w"), indent=1)
