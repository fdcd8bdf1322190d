// Scene kernels for gfx950: vertex transform at reset, obstacle OBBs for the collision
// test, and an LBVH built per env entirely in LDS (one workgroup per env): a triangle-level builder and an object-level one.
// What they share with each other and with the global-memory builder (agx_scene_large.hip) -- keys, radix tree, box-object
// marking, child references, node records, the work-list loop, the host's argument rules -- is agx_bvh_parts.h.
//
// These replace WarpEnv.reset_idx's tf_apply over all vertices + per-env wp.Mesh.refit()
// (warp_env_manager.py:40-54) and the wp.Mesh BVH build (warp_env_manager.py:162-166).
// Warp only REFITS the boxes of its initial topology after obstacles were moved; here the
// tree is rebuilt from the new positions (Morton order), which keeps traversal tight.
//
// The BVH is a pure accelerator: the ray-cast result is defined over all triangles with
// a (t, face-index) tie-break (DESIGN.md "closest-hit semantics"), so any topology is valid as
// long as node boxes are conservative -- they are grown by kBoxEps like Warp's 1e-3.
#include "agx_common.h"
#include "agx_device_math.h"
#include "agx_nav_parts.h"
#include "agx_bvh_parts.h"

namespace agx {

constexpr int kBvhThreads = 512;
constexpr int kBvhMaxTris = 2944;  // 160 KiB of LDS: 8 B x 4096 padded keys + 44 B per triangle (bvh_lds_bytes); forest_env = 2148

// triangle f of env: local frame -> world frame through its asset's pose
AGX_DEV void transform_triangle(int env, int f, int nt, int na, const float *__restrict__ tri_local, const int32_t *__restrict__ tri_asset,
                                const float *__restrict__ asset_state, float *__restrict__ tri_world) {
  const float *as = asset_state + ((size_t)env * na + tri_asset[f]) * 13;
  const V3 t = V3{as[0], as[1], as[2]};
  const Q4 q = Q4{as[3], as[4], as[5], as[6]};
  const float *src = tri_local + ((size_t)env * nt + f) * 9;
  float *dst = tri_world + ((size_t)env * nt + f) * 9;
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    V3 w = tf_apply(q, t, V3{src[3 * v], src[3 * v + 1], src[3 * v + 2]});
    dst[3 * v] = w.x; dst[3 * v + 1] = w.y; dst[3 * v + 2] = w.z;
  }
}

__global__ void __launch_bounds__(256) k_scene_transform(int n, int nt, int na, const float *__restrict__ tri_local,
                                                          const int32_t *__restrict__ tri_asset,
                                                          const float *__restrict__ asset_state,
                                                          const uint8_t *__restrict__ mask, float *__restrict__ tri_world) {
  // env on grid.x (2^31 blocks), triangle chunk on grid.y: HIP caps grid.y at 65535, the env count has no such bound
  const int env = blockIdx.x;
  if (mask && !mask[env]) return;
  const int f = blockIdx.y * blockDim.x + threadIdx.x;
  if (f >= nt) return;
  transform_triangle(env, f, nt, na, tri_local, tri_asset, asset_state, tri_world);
}

AGX_DEV void box_from_asset(int env, int k, int n, int na, const float *__restrict__ asset_state, const float *__restrict__ half_extents,
                            float *__restrict__ boxes);

__global__ void __launch_bounds__(256) k_boxes_from_assets(int n, int na, const float *__restrict__ asset_state,
                                                            const float *__restrict__ half_extents,
                                                            const uint8_t *__restrict__ mask, float *__restrict__ boxes) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = blockIdx.y;
  if (env >= n) return;
  if (mask && !mask[env]) return;
  box_from_asset(env, k, n, na, asset_state, half_extents, boxes);
}

// collision box k of env (SoA rows [k][11][n]): pose, half extents, bounding-sphere radius
AGX_DEV void box_from_asset(int env, int k, int n, int na, const float *__restrict__ asset_state, const float *__restrict__ half_extents,
                            float *__restrict__ boxes) {
  const float *as = asset_state + ((size_t)env * na + k) * 13;
  const float *he = half_extents + ((size_t)env * na + k) * 3;
  float *bx = boxes + (size_t)k * 11 * n + env;
#pragma unroll
  for (int c = 0; c < 7; ++c) bx[(size_t)c * n] = as[c];
#pragma unroll
  for (int c = 0; c < 3; ++c) bx[(size_t)(7 + c) * n] = he[c];
  // bounding-sphere radius (for the conservative cull), rounded up
  bx[(size_t)10 * n] = sqrtf(he[0] * he[0] + he[1] * he[1] + he[2] * he[2]) * 1.000001f;
}

// ------------------------------------------------------------------------------------ LBVH
#ifdef AGX_SCENE_PHASE_CLOCK  // profiles/scene_phase_probe_r06.py: where a dirty env's refresh spends its time (100 MHz wall clock)
__device__ unsigned long long g_phase_clock[16];
#define AGX_PHASE(k) do { if (threadIdx.x == 0) g_phase_clock[k] = wall_clock64(); } while (0)
#define AGX_PHASE_LAST(k) do { if (threadIdx.x == kBvhThreads - 1) g_phase_clock[k] = wall_clock64(); } while (0)
#else
#define AGX_PHASE(k) do { } while (0)
#define AGX_PHASE_LAST(k) do { } while (0)
#endif

// Multi-primitive assets (URDFs with several links: the reference's `trees`): every primitive is its own rigid
// piece whose pose follows the asset's,  prim = asset (x) local.  prim_state [N][P][13] then plays the role of
// asset_state for agx_scene_transform / agx_boxes_from_assets.
__global__ void __launch_bounds__(256) k_prims_from_assets(int n, int np_, int na, const int32_t *__restrict__ prim_asset,
                                                            const float *__restrict__ asset_state,
                                                            const float *__restrict__ local_pos,
                                                            const float *__restrict__ local_quat,
                                                            const uint8_t *__restrict__ mask, float *__restrict__ prim_state) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * np_) return;
  const int env = idx / np_;
  if (mask && !mask[env]) return;
  const float *as = asset_state + ((size_t)env * na + prim_asset[idx]) * 13;  // per env: the free assets are shuffled
  const float *lp = local_pos + (size_t)idx * 3, *lq = local_quat + (size_t)idx * 4;
  const Q4 qa = Q4{as[3], as[4], as[5], as[6]};
  const V3 c = tf_apply(qa, V3{as[0], as[1], as[2]}, V3{lp[0], lp[1], lp[2]});
  const Q4 q = quat_mul(qa, Q4{lq[0], lq[1], lq[2], lq[3]});
  float *o = prim_state + (size_t)idx * 13;
  o[0] = c.x; o[1] = c.y; o[2] = c.z;
  o[3] = q.x; o[4] = q.y; o[5] = q.z; o[6] = q.w;
#pragma unroll
  for (int k = 7; k < 13; ++k) o[k] = as[k];
}

// Kinematic obstacles (EnvManager.step(actions, env_actions), obstacle_manager.py:40-44): the env action of an
// obstacle is its twist (world-frame linear and angular velocity), written into the root state every sub-step;
// the pose follows with the integrator's rule (p += v dt, exponential map for q) for k sub-steps.
__global__ void __launch_bounds__(256) k_assets_integrate(int count, float *__restrict__ asset_state, const float *__restrict__ twist,
                                                           float dt, int k) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= count) return;
  float *st = asset_state + (size_t)a * 13;
  const float *tw = twist + (size_t)a * 6;
  V3 p = V3{st[0], st[1], st[2]};
  Q4 q = Q4{st[3], st[4], st[5], st[6]};
  const V3 v = V3{tw[0], tw[1], tw[2]}, w = V3{tw[3], tw[4], tw[5]};
  const float wm2 = dot(w, w);
  float x1 = 0.0f, y1 = 0.0f, z1 = 0.0f, cs = 1.0f;
  if (wm2 != 0.0f) {
    float wm = sqrtf(wm2);
    float sn;
    sincos_bounded(fminf(dt * wm * 0.5f, 60.0f), sn, cs);
    float sc = sn / wm;
    x1 = w.x * sc; y1 = w.y * sc; z1 = w.z * sc;
  }
  for (int s = 0; s < k; ++s) {
    p = V3{p.x + v.x * dt, p.y + v.y * dt, p.z + v.z * dt};
    if (wm2 != 0.0f) {
      float rx = x1 * q.w + y1 * q.z - z1 * q.y;
      float ry = y1 * q.w + z1 * q.x - x1 * q.z;
      float rz = z1 * q.w + x1 * q.y - y1 * q.x;
      float rw = -(x1 * q.x) - y1 * q.y - z1 * q.z;
      rx += q.x * cs; ry += q.y * cs; rz += q.z * cs; rw += q.w * cs;
      float nn = sqrtf(rx * rx + ry * ry + rz * rz + rw * rw);
      q = Q4{rx / nn, ry / nn, rz / nn, rw / nn};
    }
  }
  st[0] = p.x; st[1] = p.y; st[2] = p.z;
  st[3] = q.x; st[4] = q.y; st[5] = q.z; st[6] = q.w;
#pragma unroll
  for (int c = 0; c < 6; ++c) st[7 + c] = tw[c];  // obstacle_linvel / obstacle_angvel
}

// floats of the LDS region that holds the internal nodes' boxes and, before them, the bounds reduction's scratch
AGX_DEV constexpr int bvh_box_floats_c(int nt, int threads) { return (nt - 1) * 6 > 6 * threads ? (nt - 1) * 6 : 6 * threads; }
// box of tree node c: internal nodes from LDS, leaves (c >= n_int) from their triangle, grown by kBoxEps
AGX_DEV void node_box(const float *box, const unsigned long long *keys, const float *__restrict__ tris, int n_int, int c, float (&o)[6]) {
  if (c >= n_int) {
    leaf_box(tris, key_index(keys[c - n_int]), o);
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = box[(size_t)c * 6 + k];
  }
}

// Bitonic sort of m (a power of two) 64-bit keys in LDS by the whole workgroup.
// A thread owns elements tid + q * kBvhThreads, so a WAVE owns whole 64-element blocks: the stages with j < 64 exchange
// inside a block, i.e. inside the wave (LDS operations of a wave execute in order), and need no workgroup barrier.
// Barriers remain where the next stage reads what other waves wrote: 21 of the 66 stages for 2048 keys.
AGX_DEV void bitonic_sort_lds(unsigned long long *keys, int m, int tid) {
  for (int k = 2; k <= m; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < m; i += kBvhThreads) {
        int ixj = i ^ j;
        if (ixj > i) {
          unsigned long long a = keys[i], b = keys[ixj];
          bool up = (i & k) == 0;
          if ((a > b) == up) { keys[i] = b; keys[ixj] = a; }
        }
      }
      const int next_j = j > 1 ? (j >> 1) : k;  // (the stage after j == 1 is (2k, k))
      if (j >= 64 || next_j >= 64) {
        __syncthreads();
      } else {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // compiler: keep the stages' LDS accesses in order
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// OBJECT-LEVEL BUILD (round 6).  With AGX_BVH_BOX_OBJECTS only 2K - 1 records of the triangle-level tree are ever reached on a box
// scene (K - 1 internal nodes over the objects, K object nodes) -- yet it Morton-sorted all 12 K triangles and built 12 K - 1 nodes
// through ~25 workgroup barriers (55-60 us for ONE env).  Here the tree is built over the K OBJECTS:
//   phase 1 (all waves)   per (object, face): the bounds of the face's two triangles -> LDS, and whether they are where
//                         trimesh.creation.box has them in the object's box (box_frame / box_triangle_ok, the same verdicts as the
//                         triangle-level build's three steps)
//   -- one workgroup barrier --
//   phase 2 (waves 0-3)   a lane per object: AABB, sort centre, Morton code (the triangle-level build's object key, bit for bit); rank
//                         sort of the K keys; Karras radix tree over them; boxes bottom-up; the K - 1 internal records with both child
//                         boxes inline.  Five workgroup barriers (one wave doing all of it needs none but runs every dependent LDS
//                         round trip of two objects in sequence: 15 us against 8, profiles/r06_scene_refresh_phases.txt).
//   phase 3 (waves 4-7)   per object, concurrently: its OBJECT NODE record (a recognised box), or -- parked beyond the curriculum level
//                         at -1000 m where float32 no longer resolves a box, or simply not a box -- a fixed five-node subtree over its
//                         six triangle pairs (two-triangle leaves), so that every triangle stays reachable.
// Record layout: internal node i of the object tree at index i (root 0); object o owns indices K - 1 + 5 o .. + 4: its object record
// at the first, or its subtree (root at the fifth).  2 <= K <= 256.  The tree is a pure accelerator (closest hit over ALL triangles,
// ties by index): frames are bit-identical whatever tree is built, which is what the test suites hold.
constexpr int kObjMax = 256;
__host__ __device__ constexpr int obj_lds_bytes_c(int nt) { return kObjMax * (8 + 8 + 24 + 24 + 8 + 8 + 4 + 8 + 4 + 1 + 6) + (nt / 2) * 24 + 64; }

AGX_DEV void box_union(const float (&a)[6], const float (&b)[6], float (&o)[6]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) { o[c] = fminf(a[c], b[c]); o[3 + c] = fmaxf(a[3 + c], b[3 + c]); }
}

AGX_DEV void bvh_build_objects_env(int env, int nt, const float *__restrict__ tri_world, float *__restrict__ nodes) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int K = nt / 12, tid = threadIdx.x, lane = tid & 63;
  unsigned long long *okey = reinterpret_cast<unsigned long long *>(smem);              // [kObjMax] code . object
  unsigned long long *skey = okey + kObjMax;                                            // [kObjMax] the same, sorted
  float *oaabb = reinterpret_cast<float *>(skey + kObjMax);                             // [kObjMax][6] object AABBs
  float *nbox = oaabb + kObjMax * 6;                                                    // [kObjMax][6] internal nodes' boxes
  int *parent = reinterpret_cast<int *>(nbox + kObjMax * 6);                            // [2 kObjMax] internal i at i, sorted leaf p at K - 1 + p
  int *child = parent + 2 * kObjMax;                                                    // [kObjMax][2] (a leaf child c is K - 1 + p)
  int *counter = child + 2 * kObjMax;                                                   // [kObjMax]
  int *boxoff = counter + kObjMax;                                                      // [kObjMax][2]
  float *red = reinterpret_cast<float *>(boxoff + 2 * kObjMax);                         // [4][6] the waves' bounds of the sort centres (+ pad)
  uint8_t *objok = reinterpret_cast<uint8_t *>(red + kObjMax);                          // [kObjMax] a recognised box
  uint8_t *fok = objok + kObjMax;                                                       // [6 kObjMax] this face's two triangles are where the box has them
  float *pb = reinterpret_cast<float *>(fok + 6 * kObjMax);                             // [6 K][6] bounds of the face pairs
  const float *tris = tri_world + (size_t)env * nt * 9;
  float *out = nodes + (size_t)env * (nt - 1) * 16;

  // ---- phase 1: a thread per (object, face): the two triangles trimesh.creation.box puts on that face
  for (int t = tid; t < 6 * K; t += kBvhThreads) {
    const int obj = t / 6, fc = t - obj * 6;
    const int qa = pair_a(fc), qb = pair_b(fc);
    const float *to = tris + (size_t)obj * 12 * 9;
    float a[9], b[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { a[k] = to[9 * qa + k]; b[k] = to[9 * qb + k]; }
    float la[3], ha[3], lb[3], hb[3];
    tri_bounds(a, la, ha);
    tri_bounds(b, lb, hb);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      pb[6 * t + c] = fminf(la[c], lb[c]);
      pb[6 * t + 3 + c] = fmaxf(ha[c], hb[c]);
    }
    bool ok = !tri_parked(to);
    if (ok) {
      BoxFrame F;
      uint32_t ids = 0u, ids2 = 0u;
      ok = box_frame(to, F) && box_triangle_ok(F, a, qa, ids) && box_triangle_ok(F, b, qb, ids2) && __popc(ids | ids2) == 4;
    }
    fok[t] = (ok ? 1 : 0) | (tri_parked(to) ? 2 : 0);  // (face 0 holds triangle 0, whose first vertex decides "parked")
  }
  __syncthreads();
  AGX_PHASE(4);

  constexpr int kTreeThreads = kObjMax;  // waves 0-3: one object / sorted position / tree node per lane; waves 4-7: phase 3
  if (tid >= kTreeThreads) {
    // ---- phase 3 (waves 4-7): the records the objects own
    for (int o = tid - kTreeThreads; o < K; o += kBvhThreads - kTreeThreads) {
      bool ok = true;
#pragma unroll
      for (int j = 0; j < 6; ++j) ok = ok && (fok[6 * o + j] & 1) != 0;
      const int base = K - 1 + 5 * o, g0 = 12 * o;
      float *rec = out + (size_t)base * 16;
      if (ok) {
        box_object_record(tris, o, rec);
        continue;
      }
      // six two-triangle leaves (the face pairs of trimesh's box; for anything else just six pairs), five nodes over them
      // (one pair of faces at a time: two boxes in, one node out, their union kept -- 36 live floats at once spilled)
      float un[3][6];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        float p0[6], p1[6];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          p0[c] = pb[6 * (6 * o + 2 * j) + c] - kBoxEps; p0[3 + c] = pb[6 * (6 * o + 2 * j) + 3 + c] + kBoxEps;
          p1[c] = pb[6 * (6 * o + 2 * j + 1) + c] - kBoxEps; p1[3 + c] = pb[6 * (6 * o + 2 * j + 1) + 3 + c] + kBoxEps;
        }
        store_node(rec + 16 * j, p0, p1, ~(g0 + pair_a(2 * j)), ~(g0 + pair_a(2 * j + 1)), g0 + pair_b(2 * j), g0 + pair_b(2 * j + 1));
        box_union(p0, p1, un[j]);
      }
      store_node(rec + 48, un[0], un[1], base + 0, base + 1, -1, -1);
      float d[6];
      box_union(un[0], un[1], d);
      store_node(rec + 64, d, un[2], base + 3, base + 2, -1, -1);
    }
    AGX_PHASE_LAST(8);
  }

  // ---- phase 2 (waves 0-3, lane = object, then sorted position, then node): the tree over the objects.  Every wave of the
  // workgroup takes part in the five barriers between its steps.
  const int o = tid;
  const bool has_obj = tid < K;
  float oc[4] = {0.0f, 0.0f, 0.0f, -1.0f};  // the object's sort-centre record (object_sort_centre), in registers
  {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (has_obj) {
      float alo[3] = {INFINITY, INFINITY, INFINITY}, ahi[3] = {-INFINITY, -INFINITY, -INFINITY};
      bool ok = true;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        ok = ok && (fok[6 * o + j] & 1) != 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          alo[c] = fminf(alo[c], pb[6 * (6 * o + j) + c]);
          ahi[c] = fmaxf(ahi[c], pb[6 * (6 * o + j) + 3 + c]);
        }
      }
      objok[o] = ok ? 1 : 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        oaabb[6 * o + c] = alo[c] - kBoxEps;      // (grown once, here: every box above is a union of these)
        oaabb[6 * o + 3 + c] = ahi[c] + kBoxEps;
      }
      object_sort_centre(alo, ahi, (fok[6 * o] & 2) != 0, oc, lo, hi);
    }
    if (tid < kTreeThreads) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float a = lo[c], b = hi[c];
        wave_min_max(a, b);
        if (lane == 0) { red[6 * (tid >> 6) + c] = a; red[6 * (tid >> 6) + 3 + c] = b; }
      }
    }
  }
  __syncthreads();
  AGX_PHASE(5);
  if (has_obj) {
    float blo[3], inv[3], max_ext = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float a = INFINITY, b = -INFINITY;
#pragma unroll
      for (int wv = 0; wv < kTreeThreads / 64; ++wv) { a = fminf(a, red[6 * wv + c]); b = fmaxf(b, red[6 * wv + 3 + c]); }
      blo[c] = a;
      const float ext = b - a;
      inv[c] = grid_scale(ext);
      max_ext = c == 0 ? ext : fmaxf(max_ext, ext);
    }
    const bool parked = oc[3] < 0.0f;
    const uint32_t code = sort_code(morton30(oc, blo, inv), oc[3], max_ext, parked);
    okey[o] = pack_key(parked ? code : class_code(code, 0u), o);
  }
  __syncthreads();
  if (has_obj) {  // rank sort: the keys are unique (the object index is the low word)
    const unsigned long long mine = okey[o];
    int rank = 0;
#pragma unroll 8
    for (int g = 0; g < K; ++g) rank += okey[g] < mine ? 1 : 0;  // (the same address in every lane: a broadcast read)
    skey[rank] = mine;
  }
  __syncthreads();
  AGX_PHASE(6);
  // Karras 2012 over the K sorted keys: children, parents, where the children's boxes lie
  const int n_int = K - 1;
  if (tid < n_int) {
    const int i = tid;
    int left, right, j;
    karras_node(skey, K, i, left, right, j);
    child[2 * i] = left;
    child[2 * i + 1] = right;
    parent[left] = i;
    parent[right] = i;
    counter[i] = 0;
    // float offsets from oaabb (nbox follows it): the bottom-up pass reads the boxes without going through the key table
    boxoff[2 * i] = left >= n_int ? 6 * key_index(skey[left - n_int]) : 6 * (kObjMax + left);
    boxoff[2 * i + 1] = right >= n_int ? 6 * key_index(skey[right - n_int]) : 6 * (kObjMax + right);
  }
  if (tid == 0) parent[0] = -1;
  __syncthreads();
  AGX_PHASE(9);
  // bottom-up: the second arriver at a node merges its children's boxes
  if (has_obj) {
    int node = parent[n_int + tid];
    while (node >= 0) {
      __threadfence_block();  // release: this thread's box is written before the arrival
      const int arrived = atomicAdd(&counter[node], 1);
      const int o0 = boxoff[2 * node], o1 = boxoff[2 * node + 1], up = parent[node];
      if (arrived == 0) break;
      __threadfence_block();  // acquire: the sibling's box is read after the arrival
      float a[6], b[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) { a[k] = oaabb[o0 + k]; b[k] = oaabb[o1 + k]; }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        nbox[6 * node + c] = fminf(a[c], b[c]);
        nbox[6 * node + 3 + c] = fmaxf(a[3 + c], b[3 + c]);
      }
      node = up;
    }
  }
  __syncthreads();
  AGX_PHASE(10);
  // emit the K - 1 internal records, both child boxes inline
  if (tid < n_int) {
    const int i = tid;
    float bx[2][6];
    int ref[2];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const int c = child[2 * i + side];
      if (c >= n_int) {
        const int ob = key_index(skey[c - n_int]);
#pragma unroll
        for (int k = 0; k < 6; ++k) bx[side][k] = oaabb[6 * ob + k];
        ref[side] = objok[ob] ? ((K - 1 + 5 * ob) | AGX_BVH_OBJECT_REF) : (K - 1 + 5 * ob + 4);
      } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) bx[side][k] = nbox[6 * c + k];
        ref[side] = c;
      }
    }
    store_node(out + (size_t)i * 16, bx[0], bx[1], ref[0], ref[1], -1, -1);
  }
  AGX_PHASE(7);
}

// The triangle-level build (node records: store_node, agx_bvh_parts.h).
// OBJ: the launch is known to take the object-level build (object_level_build() on the host: launch arguments only) -- each kernel
// instance carries ONE builder (both inlined in one kernel spilled loop-carried values to scratch)
template <bool OBJ>
AGX_DEV void bvh_build_env(int env, int nt, int npad, int ppo, const float *__restrict__ tri_world, float *__restrict__ nodes) {
  if (OBJ) {
    bvh_build_objects_env(env, nt, tri_world, nodes);
    return;
  }
  const bool force_full_sort = (ppo & AGX_BVH_FULL_SORT) != 0;
  const bool box_objects = (ppo & AGX_BVH_BOX_OBJECTS) != 0;
  ppo = bvh_ppo(ppo);
  extern __shared__ __align__(16) unsigned char smem[];
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(smem);         // [npad]
  // Only the INTERNAL nodes' boxes live in LDS: a leaf's box is three min / max over its triangle, recomputed where it is
  // needed (twice).  That, and the reduction scratch sharing the box region (it is dead before the first box is written),
  // takes the footprint from 115 KB to 72 KB for T = 1272: TWO workgroups per CU, i.e. 512 envs in flight instead of 256
  // (with 300-400 dirty envs per step at 8192 envs the rebuild was two rounds: 150 -> see profiles/r02_small_batch.txt).
  float *box = reinterpret_cast<float *>(keys + npad);                              // [nt-1][6] (>= the reduction scratch)
  int *parent = reinterpret_cast<int *>(box + bvh_box_floats_c(nt, kBvhThreads));                  // [2nt-1]
  int *child = parent + (2 * nt - 1);                                               // [nt-1][2]
  int *counter = child + 2 * (nt - 1);                                              // [nt-1]
  float *red = box;                                                                 // [6][kBvhThreads], first phase only
  const int tid = threadIdx.x;
  const float *tris = tri_world + (size_t)env * nt * 9;

  // --- Morton grid (centre_grid) over the sort centres.  With ppo > 0 the scene is a soup of K = nt / ppo objects of ppo
  // consecutive triangles each (boxes: 12) and the sort centre is the OBJECT's: the radix tree becomes a two-level hierarchy,
  // objects on top.  Measured on the config-3 scene: 105 -> see profiles/r01_raycast_variants.txt.
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  float *ocen = reinterpret_cast<float *>(counter);  // [K][8] object_sort_centre's record in the first four; counter is not live yet
  const int K = ppo > 0 ? nt / ppo : 0;
  // (every thread takes triangles -- nine independent loads each -- and leaves their bounds in LDS; the object's thread then
  //  reduces ppo LDS entries.  One thread per object walking its 3 ppo vertices was 36 memory latencies in sequence: the longest
  //  phase of the build.  The scratch is the box region, one entry longer than it: it runs into `parent`, not live yet.)
  float *tb = box;  // [nt][6]
  if (ppo > 0) {
    for (int f = tid; f < nt; f += kBvhThreads) {
      const float *t = tris + (size_t)f * 9;
      float v[9], tlo[3], thi[3];
#pragma unroll
      for (int k = 0; k < 9; ++k) v[k] = t[k];
      tri_bounds(v, tlo, thi);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        tb[6 * f + c] = tlo[c];
        tb[6 * f + 3 + c] = thi[c];
      }
    }
    __syncthreads();
  }
  for (int o = tid; o < K; o += kBvhThreads) {
    float alo[3] = {INFINITY, INFINITY, INFINITY}, ahi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int j = 0; j < ppo; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        alo[c] = fminf(alo[c], tb[6 * (o * ppo + j) + c]);
        ahi[c] = fmaxf(ahi[c], tb[6 * (o * ppo + j) + 3 + c]);
      }
    // (object_sort_centre's arithmetic, written out: through the call this kernel's code object built a 2944-triangle soup,
    //  which never enters this loop, in 150.0 us instead of 145.6)
    const bool parked = tri_parked(tris + (size_t)o * ppo * 9);
    float big = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float cen = 0.5f * (alo[c] + ahi[c]);
      ocen[8 * o + c] = cen;
      big = fmaxf(big, ahi[c] - alo[c]);
      if (!parked) { lo[c] = fminf(lo[c], cen); hi[c] = fmaxf(hi[c], cen); }
    }
    ocen[8 * o + 3] = parked ? -1.0f : big;
  }
  for (int f = tid; f < nt && ppo <= 0; f += kBvhThreads) soup_sort_centre(tris + (size_t)f * 9, lo, hi);
  if (ppo > 0) __syncthreads();  // the reduction scratch below shares the region the triangle bounds were read from
  float blo[3], inv[3], max_ext;
  centre_grid<kBvhThreads>(lo, hi, red, blo, inv, max_ext);
  // --- keys (agx_bvh_parts.h).  Objects of ppo triangles each (boxes: 12): the order of the keys is the order of the OBJECTS'
  // codes, and inside an object (face class, index).  So sort the K object keys (128 instead of 2048: the full sort was 35 of the
  // build's 67 us) and RANK every triangle inside its object against the ppo - 1 others.  This is the full sort's order exactly
  // unless two objects that are in the env share all 27 upper Morton bits -- their triangles would interleave by face class --,
  // which is looked for, and then the full sort runs.  (Parked objects all carry kParkedCode: index order, which the object
  // keys' low word gives.)
  bool presorted = false;
  if (ppo >= 2 && K >= 2 && K * ppo == nt && !force_full_sort) {
    __syncthreads();  // (the reduction's result is in registers everywhere: its scratch is reused)
    int Kpad = 1;
    while (Kpad < K) Kpad <<= 1;
    unsigned long long *okey = reinterpret_cast<unsigned long long *>(box);  // [Kpad] code . object
    uint32_t *ocode = reinterpret_cast<uint32_t *>(okey + Kpad);             // [K]    the object's code (Morton | large flag, or parked)
    int *orank = reinterpret_cast<int *>(ocode + K);                         // [K]    position of the object in the order
    int *tie = orank + K;                                                     // [1]
    uint8_t *cls = reinterpret_cast<uint8_t *>(tie + 1);                      // [nt]   face class of the triangle (0 when parked)
    if (tid == 0) *tie = 0;
    for (int o = tid; o < Kpad; o += kBvhThreads) {
      unsigned long long k64 = ~0ull;
      if (o < K) {
        const float *oc = ocen + 8 * o;
        const bool parked = oc[3] < 0.0f;
        const uint32_t code = sort_code(morton30(oc, blo, inv), oc[3], max_ext, parked);
        ocode[o] = code;
        k64 = pack_key(parked ? code : class_code(code, 0u), o);
      }
      okey[o] = k64;
    }
    for (int f = tid; f < nt; f += kBvhThreads)
      cls[f] = (uint8_t)(ocen[8 * (f / ppo) + 3] < 0.0f ? 0u : face_class(tris + (size_t)f * 9));
    __syncthreads();
    bitonic_sort_lds(okey, Kpad, tid);
    __syncthreads();
    for (int p = tid; p < K; p += kBvhThreads) {
      const unsigned long long a = okey[p];
      orank[key_index(a)] = p;
      if (p + 1 < K) {
        const uint32_t c0 = (uint32_t)(a >> 32), c1 = (uint32_t)(okey[p + 1] >> 32);
        if (c0 == c1 && c0 != kParkedCode) *tie = 1;  // (every writer stores the same value)
      }
    }
    __syncthreads();
    presorted = *tie == 0;  // the same for the whole workgroup
    if (presorted) {
      for (int f = tid; f < npad; f += kBvhThreads) {
        if (f < nt) {
          const int o = f / ppo, g0 = o * ppo;
          const uint32_t oc = ocode[o];
          const uint32_t cf = cls[f];
          int r = 0;
          for (int g = g0; g < g0 + ppo; ++g) {
            const uint32_t cg = cls[g];
            r += (cg < cf || (cg == cf && g < f)) ? 1 : 0;
          }
          keys[orank[o] * ppo + r] = pack_key(oc == kParkedCode ? oc : class_code(oc, cf), f);
        } else {
          keys[f] = ~0ull;
        }
      }
    }
    __syncthreads();
  }
  for (int f = tid; f < npad && !presorted; f += kBvhThreads)
    keys[f] = f < nt ? triangle_key(tris + (size_t)f * 9, f, ppo, ocen, blo, inv, max_ext) : ~0ull;
  __syncthreads();
  // --- sort
  if (!presorted) bitonic_sort_lds(keys, npad, tid);
  __syncthreads();
  // --- radix tree
  const int n_int = nt - 1;
  for (int i = tid; i < n_int; i += kBvhThreads) {
    int left, right, j;
    karras_node(keys, nt, i, left, right, j);
    child[2 * i] = left;
    child[2 * i + 1] = right;
    parent[left] = i;
    parent[right] = i;
    counter[i] = j << 2;  // arrival count in the two low bits; the other end of the node's key range above them (emit stage)
  }
  if (tid == 0) parent[0] = -1;
  __syncthreads();
  // --- bottom-up box propagation: the second arriver at a node merges its children
  for (int i = tid; i < nt; i += kBvhThreads) {
    int node = parent[n_int + i];
    while (node >= 0) {
      __threadfence_block();  // release: this thread's box is written before the arrival
      if ((atomicAdd(&counter[node], 1) & 3) == 0) break;
      __threadfence_block();  // acquire: the sibling's box is read after the arrival
      float a[6], b[6];
      node_box(box, keys, tris, n_int, child[2 * node], a);
      node_box(box, keys, tris, n_int, child[2 * node + 1], b);
      float *o = box + (size_t)node * 6;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        o[c] = fminf(a[c], b[c]);
        o[3 + c] = fmaxf(a[3 + c], b[3 + c]);
      }
      node = parent[node];
    }
  }
  __syncthreads();
  mark_box_objects<kBvhThreads>(box_objects, nt, tris, keys, counter, parent);  // (objroot[] in parent[], dead since the propagation)
  // --- emit nodes with both child boxes inline
  float *out = nodes + (size_t)env * (nt - 1) * 16;
  for (int i = tid; i < n_int; i += kBvhThreads) {
    int ref[2], second[2];
    float bx[2][6];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const int c = child[2 * i + side];
      node_box(box, keys, tris, n_int, c, bx[side]);
      ref[side] = child_ref(keys, child, counter, n_int, c, second[side]);
    }
    float *o = out + (size_t)i * 16;
    int obj;
    if (object_node(keys, counter, i, obj)) {  // the box's frame is its record
      box_object_record(tris, obj, o);
      continue;
    }
    // (store_node's sixteen stores, written out: through the call the box scene's build took 69.5 us instead of 68.0)
    const float *a = bx[0], *b = bx[1];
    o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = __int_as_float(ref[0]);
    o[4] = a[3]; o[5] = a[4]; o[6] = a[5]; o[7] = __int_as_float(ref[1]);
    o[8] = b[0]; o[9] = b[1]; o[10] = b[2]; o[11] = __int_as_float(second[0]);
    o[12] = b[3]; o[13] = b[4]; o[14] = b[5]; o[15] = __int_as_float(second[1]);
  }
}

// The 100+ KB LDS footprint lets one workgroup live on a CU, so a grid of one workgroup per env costs
// ~5 us of scheduling per env even when the env has nothing to rebuild (167 us per step at 8192 envs
// with 2 % dirty envs).  Instead: one small workgroup compacts the dirty env ids into a work list and a
// CU-sized persistent grid pulls envs from it through an atomic cursor (perfect balance, no idle slots).
//   work[0] = number of dirty envs, work[1] = cursor, work[2 ...] = env ids
// flag != nullptr: the step's reset flag word -- 0 means no env resets whatever the mask holds (what k_reset_assets and the
// one-launch refresh read), and the list stays empty
__global__ void __launch_bounds__(1024) k_compact_mask(int n, const uint8_t *__restrict__ mask, int32_t *__restrict__ work,
                                                        const int32_t *__restrict__ flag) {
  __shared__ int count;
  if (threadIdx.x == 0) count = 0;
  __syncthreads();
  const bool any = !flag || *flag != 0;
  for (int env = threadIdx.x; any && env < n; env += blockDim.x)
    if (mask[env]) work[2 + atomicAdd(&count, 1)] = env;
  __syncthreads();
  if (threadIdx.x == 0) {
    work[0] = count;
    work[1] = 0;
  }
}

template <bool OBJ>
__global__ void __launch_bounds__(kBvhThreads, 4) k_bvh_build(int n, int nt, int npad, int ppo, const float *__restrict__ tri_world,
                                                            int32_t *__restrict__ work, float *__restrict__ nodes) {
  if (!work) {  // every env
    for (int env = blockIdx.x; env < n; env += gridDim.x) {
      bvh_build_env<OBJ>(env, nt, npad, ppo, tri_world, nodes);
      __syncthreads();  // LDS is reused by the next env
    }
    return;
  }
  for_each_listed_env(work, [&](int env) { bvh_build_env<OBJ>(env, nt, npad, ppo, tri_world, nodes); });
}

// The masked refresh of a navigation step in ONE persistent launch: the workgroup that pulls a dirty env from the work list
// writes that env's world-frame triangles and collision boxes itself, then builds its tree.  As three launches the two small
// ones cost a dispatch over ALL envs each (40 960 and 3 392 workgroups at 8192 envs x 106 obstacles that look at the mask and
// leave: 22 + 9 us per step for a few dozen dirty envs).  Same device functions, same arithmetic.
// the asset reset of a dirty env in the refresh launch itself (agx_scene_reset_refresh; device generator only)
struct SceneResetArgs {
  int enabled, num_obstacles, num_keep;
  AgxEnvBuffers B;
  AgxResetArgs R;
  const float *min_ratio, *max_ratio;
};

template <bool OBJ>
AGX_DEV void scene_refresh_env(int env, int n, int nt, int npad, int ppo, int na, const float *__restrict__ tri_local,
                               const int32_t *__restrict__ tri_asset, float *asset_state, const float *__restrict__ half_extents,
                               float *tri_world, float *__restrict__ boxes, float *__restrict__ nodes, const SceneResetArgs &S) {
  AGX_PHASE(0);
  if (S.enabled) {  // AssetManager.reset_idx for this env first: the poses the triangles are about to be moved to
    for (int a = threadIdx.x; a < na; a += kBvhThreads)
      reset_asset_one(S.B, S.R, env, a, na, nullptr, nullptr, nullptr, S.min_ratio, S.max_ratio, S.num_obstacles, S.num_keep, asset_state);
    __syncthreads();  // (workgroup scope: the poses are read back by this workgroup only)
  }
  AGX_PHASE(1);
  for (int f = threadIdx.x; f < nt; f += kBvhThreads) transform_triangle(env, f, nt, na, tri_local, tri_asset, asset_state, tri_world);
  AGX_PHASE(2);
  if (boxes)
    for (int k = threadIdx.x; k < na; k += kBvhThreads) box_from_asset(env, k, n, na, asset_state, half_extents, boxes);
  __syncthreads();  // the env's triangles are in memory (workgroup scope) before the build reads them
  AGX_PHASE(3);
  bvh_build_env<OBJ>(env, nt, npad, ppo, tri_world, nodes);
}

template <bool OBJ>
__global__ void __launch_bounds__(kBvhThreads, 4) k_scene_refresh(int n, int nt, int npad, int ppo, int na, const float *__restrict__ tri_local,
                                                                const int32_t *__restrict__ tri_asset,
                                                                float *asset_state,
                                                                const float *__restrict__ half_extents, float *tri_world,
                                                                float *__restrict__ boxes, int32_t *__restrict__ work,
                                                                float *__restrict__ nodes, const uint8_t *__restrict__ mask, SceneResetArgs S) {
  if (mask) {
    // DIRECT mode (small batches: one workgroup per env, no work list): a clean env's workgroup leaves at once -- the launch that
    // compacted the mask (and the one that reset the assets, S.enabled) are gone from the step, and a step without a dirty env
    // costs one dispatch
    const int env = blockIdx.x;
    if (S.enabled && S.B.reset_flag[S.B.flag_parity] == 0) return;
    if (!mask[env]) return;
    scene_refresh_env<OBJ>(env, n, nt, npad, ppo, na, tri_local, tri_asset, asset_state, half_extents, tri_world, boxes, nodes, S);
    return;
  }
  for_each_listed_env(work, [&](int env) {
    scene_refresh_env<OBJ>(env, n, nt, npad, ppo, na, tri_local, tri_asset, asset_state, half_extents, tri_world, boxes, nodes, S);
  });
}

int compact_mask_launch(int n, const uint8_t *mask, int32_t *work, void *stream, const int32_t *flag) {
  hipLaunchKernelGGL(k_compact_mask, dim3(1), dim3(1024), 0, (hipStream_t)stream, n, mask, work, flag);
  return check_launch("k_compact_mask");
}
// the persistent grid of the LDS builders: two resident workgroups per CU (LDS bound: 72 KB each for T = 1272 triangle-level, 41 KB
// object-level)
static int bvh_persistent_grid(int n) { return n < 512 ? n : 512; }

static size_t bvh_lds_bytes(int nt, int npad) {
  const size_t box_floats = (size_t)(nt - 1) * 6 > (size_t)6 * kBvhThreads ? (size_t)(nt - 1) * 6 : (size_t)6 * kBvhThreads;
  const size_t tri_level = (size_t)npad * 8 + box_floats * 4 + (size_t)(2 * nt - 1) * 4 + (size_t)(nt - 1) * 8 + (size_t)(nt - 1) * 4 + 64;
  const size_t obj_level = (size_t)obj_lds_bytes_c(nt);
  return tri_level > obj_level ? tri_level : obj_level;
}
// what a launch that is KNOWN to take the object-level build needs (the triangle-level build's 72 KB for 1272 triangles allow two
// workgroups per CU; 41 KB allow three)
static bool object_level_build(int nt, int prims_per_object) {
  return (prims_per_object & AGX_BVH_OBJECT_TREE) && (prims_per_object & AGX_BVH_BOX_OBJECTS) && !(prims_per_object & AGX_BVH_FULL_SORT) &&
         bvh_ppo(prims_per_object) == 12 &&
         nt >= 24 && nt / 12 <= kObjMax;
}
static size_t bvh_lds_bytes_for(int nt, int npad, int prims_per_object) {
  return object_level_build(nt, prims_per_object) ? (size_t)obj_lds_bytes_c(nt) : bvh_lds_bytes(nt, npad);
}

}  // namespace agx

using namespace agx;

extern "C" int agx_scene_transform(int n, int nt, int na, const float *tri_local, const int32_t *tri_asset,
                                   const float *asset_state, const uint8_t *mask, float *tri_world, void *stream) {
  AGX_REQUIRE(n > 0 && nt > 0 && na > 0, "bad sizes n=%d nt=%d na=%d", n, nt, na);
  AGX_REQUIRE(tri_local && tri_asset && asset_state && tri_world, "null buffer");
  AGX_REQUIRE(blocks_for(nt, 256) <= 65535, "num_tris %d: more than 65535 chunks of 256 triangles per env (grid.y)", nt);
  dim3 grid(n, blocks_for(nt, 256));
  hipLaunchKernelGGL(k_scene_transform, grid, dim3(256), 0, (hipStream_t)stream, n, nt, na, tri_local, tri_asset, asset_state,
                     mask, tri_world);
  return check_launch("agx_scene_transform");
}

extern "C" int agx_boxes_from_assets(int n, int na, const float *asset_state, const float *half_extents, const uint8_t *mask,
                                     float *boxes, void *stream) {
  AGX_REQUIRE(n > 0 && na > 0, "bad sizes");
  AGX_REQUIRE(asset_state && half_extents && boxes, "null buffer");
  AGX_REQUIRE(na <= 65535, "num_assets %d: more than 65535 boxes per env (grid.y is the box index)", na);
  dim3 grid(blocks_for(n, 256), na);
  hipLaunchKernelGGL(k_boxes_from_assets, grid, dim3(256), 0, (hipStream_t)stream, n, na, asset_state, half_extents, mask, boxes);
  return check_launch("agx_boxes_from_assets");
}

extern "C" size_t agx_bvh_nodes_bytes(int n, int nt) { return nt > 1 ? (size_t)n * (nt - 1) * 16 * sizeof(float) : 0; }

#ifdef AGX_SCENE_PHASE_CLOCK
extern "C" int agx_debug_phase_clock(unsigned long long *out16) {
  return (int)hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_phase_clock), sizeof(unsigned long long) * 16);
}
#endif

extern "C" int agx_prims_from_assets(int n, int num_prims, int num_assets, const int32_t *prim_asset, const float *asset_state,
                                     const float *local_pos, const float *local_quat, const uint8_t *mask, float *prim_state,
                                     void *stream) {
  AGX_REQUIRE(n > 0 && num_prims > 0 && num_assets > 0, "bad sizes");
  AGX_REQUIRE(prim_asset && asset_state && local_pos && local_quat && prim_state, "null buffer");
  hipLaunchKernelGGL(k_prims_from_assets, dim3(blocks_for(n * num_prims, 256)), dim3(256), 0, (hipStream_t)stream, n, num_prims,
                     num_assets, prim_asset, asset_state, local_pos, local_quat, mask, prim_state);
  return check_launch("agx_prims_from_assets");
}

extern "C" int agx_assets_integrate(int n, int num_assets, float *asset_state, const float *twist, float dt, int k, void *stream) {
  AGX_REQUIRE(n > 0 && num_assets > 0 && k >= 0 && k <= AGX_MAX_SUBSTEPS && dt > 0.0f, "bad arguments");
  AGX_REQUIRE(asset_state && twist, "null buffer");
  const int count = n * num_assets;
  hipLaunchKernelGGL(k_assets_integrate, dim3(blocks_for(count, 256)), dim3(256), 0, (hipStream_t)stream, count, asset_state, twist,
                     dt, k);
  return check_launch("agx_assets_integrate");
}

// argument checks and launch shape shared by the two LBVH builders; `kernel`'s dynamic LDS limit is raised once (*attr_set)
static int bvh_launch_shape(int nt, int prims_per_object, int *npad_out, size_t *lds_out, const void *kernel, bool *attr_set) {
  AGX_REQUIRE(nt >= 2 && nt <= kBvhMaxTris, "num_tris %d outside [2, %d] (LDS-resident LBVH build)", nt, kBvhMaxTris);
  if (int e = bvh_check_objects(nt, prims_per_object, true)) return e;
  const int npad = bvh_npad(nt);
  const size_t lds = bvh_lds_bytes_for(nt, npad, prims_per_object);
  if (!*attr_set) {
    // the kernel also owns 4 bytes of static LDS: the dynamic maximum must leave room for them
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
    AGX_REQUIRE(e == hipSuccess, "hipFuncSetAttribute(LBVH build): %s", hipGetErrorString(e));
    *attr_set = true;
  }
  AGX_REQUIRE(lds <= 160 * 1024 - 256, "LBVH build needs %zu bytes of LDS (> 160 KiB)", lds);
  *npad_out = npad;
  *lds_out = lds;
  return AGX_OK;
}

// AssetManager's geometry refresh behind a reset (asset_manager.py:51-71 -> warp mesh refit, warp_env ...): world-frame
// triangles, collision boxes and the tree of the envs flagged in `mask`; mask == nullptr: every env (the three stand-alone
// launches).  One C call; with a mask, two launches (compaction + the persistent k_scene_refresh).
extern "C" int agx_reset_assets(const AgxEnvBuffers *B, int n, int K, const AgxResetArgs *R, const float *u1, const float *u2,
                                const float *u_sel, const float *min_ratio, const float *max_ratio, int num_obstacles,
                                int num_keep, float *asset_state, void *stream);

constexpr int kDirectRefreshEnvs = 2048;  // up to here a workgroup per env (clean ones leave at once) beats compaction + a persistent grid

// the masked refresh: direct (one workgroup per env, optionally with the asset reset in it) or compaction + persistent grid
static int scene_refresh_launch(int n, int nt, int na, const float *tri_local, const int32_t *tri_asset, float *asset_state,
                                const float *half_extents, int prims_per_object, const uint8_t *mask, float *tri_world, float *boxes,
                                float *nodes, int32_t *work, const SceneResetArgs *reset, const int32_t *flag, void *stream) {
  static bool attr_set[2] = {false, false};
  const bool obj = object_level_build(nt, prims_per_object);
  auto kernel = obj ? k_scene_refresh<true> : k_scene_refresh<false>;
  int npad = 0;
  size_t lds = 0;
  if (int e = bvh_launch_shape(nt, prims_per_object, &npad, &lds, reinterpret_cast<const void *>(kernel), &attr_set[obj])) return e;
  SceneResetArgs S{};
  if (reset) S = *reset;
  if (n <= kDirectRefreshEnvs) {
    hipLaunchKernelGGL(kernel, dim3(n), dim3(kBvhThreads), lds, (hipStream_t)stream, n, nt, npad, prims_per_object, na, tri_local,
                       tri_asset, asset_state, half_extents, tri_world, boxes, work, nodes, mask, S);
    return check_launch("agx_scene_refresh");
  }
  if (int e = compact_mask_launch(n, mask, work, stream, flag)) return e;
  hipLaunchKernelGGL(kernel, dim3(bvh_persistent_grid(n)), dim3(kBvhThreads), lds, (hipStream_t)stream, n, nt, npad, prims_per_object, na, tri_local,
                     tri_asset, asset_state, half_extents, tri_world, boxes, work, nodes, (const uint8_t *)nullptr, S);
  return check_launch("agx_scene_refresh");
}

extern "C" int agx_scene_refresh(int n, int nt, int na, const float *tri_local, const int32_t *tri_asset, const float *asset_state,
                                 const float *half_extents, int prims_per_object, const uint8_t *mask, float *tri_world,
                                 float *boxes, float *nodes, int32_t *work, void *stream) {
  AGX_REQUIRE(n > 0 && nt > 0 && na > 0, "bad sizes n=%d nt=%d na=%d", n, nt, na);
  AGX_REQUIRE(tri_local && tri_asset && asset_state && tri_world && nodes, "null buffer");
  AGX_REQUIRE(!boxes || half_extents, "collision boxes need the half extents");
  if (!mask) {
    if (int e = agx_scene_transform(n, nt, na, tri_local, tri_asset, asset_state, nullptr, tri_world, stream)) return e;
    if (int e = agx_bvh_build(n, nt, prims_per_object, tri_world, nullptr, nodes, work, stream)) return e;
    return boxes ? agx_boxes_from_assets(n, na, asset_state, half_extents, nullptr, boxes, stream) : AGX_OK;
  }
  AGX_REQUIRE(work, "a masked refresh needs the work buffer (int32[num_envs + 2])");
  return scene_refresh_launch(n, nt, na, tri_local, tri_asset, const_cast<float *>(asset_state), half_extents, prims_per_object, mask, tri_world, boxes,
                              nodes, work, nullptr, nullptr, stream);
}

// AssetManager.reset_idx + the geometry refresh behind it (agx_reset_assets + agx_scene_refresh) for the envs of buf->reset_mask, device
// generator only.  Up to kDirectRefreshEnvs envs: ONE launch (a workgroup per env; a clean env's leaves at once); above: the three
// launches (asset reset, mask compaction, persistent refresh).  Same device functions either way: the same poses, triangles and trees.
extern "C" int agx_scene_reset_refresh(const AgxEnvBuffers *B, int n, int nt, int na, const AgxResetArgs *R, const float *min_ratio,
                                       const float *max_ratio, int num_obstacles, int num_keep, float *asset_state, const float *tri_local,
                                       const int32_t *tri_asset, const float *half_extents, int prims_per_object, float *tri_world,
                                       float *boxes, float *nodes, int32_t *work, void *stream) {
  AGX_REQUIRE(B && R && n > 0 && nt > 0 && na > 0, "bad arguments");
  AGX_REQUIRE(min_ratio && max_ratio && asset_state && tri_local && tri_asset && tri_world && nodes && work, "null buffer");
  AGX_REQUIRE(B->reset_flag && B->reset_mask && B->episode_count, "the device generator needs reset_flag, reset_mask and episode_count");
  AGX_REQUIRE(!R->u_state, "agx_scene_reset_refresh draws from the device generator (strict draws: agx_reset_assets + agx_scene_refresh)");
  AGX_REQUIRE(!boxes || half_extents, "collision boxes need the half extents");
  SceneResetArgs S{1, num_obstacles, num_keep, *B, *R, min_ratio, max_ratio};
  if (n > kDirectRefreshEnvs) {
    if (int e = agx_reset_assets(B, n, na, R, nullptr, nullptr, nullptr, min_ratio, max_ratio, num_obstacles, num_keep, asset_state, stream)) return e;
    return scene_refresh_launch(n, nt, na, tri_local, tri_asset, asset_state, half_extents, prims_per_object, B->reset_mask, tri_world, boxes, nodes,
                                work, nullptr, B->reset_flag + B->flag_parity, stream);
  }
  return scene_refresh_launch(n, nt, na, tri_local, tri_asset, asset_state, half_extents, prims_per_object, B->reset_mask, tri_world, boxes, nodes, work,
                              &S, nullptr, stream);
}

extern "C" int agx_bvh_build(int n, int nt, int prims_per_object, const float *tri_world, const uint8_t *mask, float *nodes,
                             int32_t *work, void *stream) {
  AGX_REQUIRE(n > 0, "bad num_envs");
  AGX_REQUIRE(tri_world && nodes, "null buffer");
  AGX_REQUIRE(!mask || work, "a masked rebuild needs the work buffer (int32[num_envs + 2])");
  static bool attr_set[2] = {false, false};
  const bool obj = object_level_build(nt, prims_per_object);
  auto kernel = obj ? k_bvh_build<true> : k_bvh_build<false>;
  int npad = 0;
  size_t lds = 0;
  if (int e = bvh_launch_shape(nt, prims_per_object, &npad, &lds, reinterpret_cast<const void *>(kernel), &attr_set[obj])) return e;
  if (mask)
    if (int e = compact_mask_launch(n, mask, work, stream)) return e;
  hipLaunchKernelGGL(kernel, dim3(bvh_persistent_grid(n)), dim3(kBvhThreads), lds, (hipStream_t)stream, n, nt, npad,
                     prims_per_object, tri_world, mask ? work : nullptr, nodes);  // (with the AGX_BVH_FULL_SORT bit, if set)
  return check_launch("agx_bvh_build");
}
