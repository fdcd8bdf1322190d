// The LBVH builders' shared parts: everything the LDS-resident builds (agx_scene.hip) and the global-memory build of scenes above
// their cap (agx_scene_large.hip) agree on BY CONSTRUCTION -- the sort keys, the Karras radix tree, the recognition of box objects,
// the child references and the record of an emitted node, the work-list loop -- plus the host's argument rules.  The rules are
// DEFINED here.  The builders keep what differs: where the boxes live, the sorts, the memory layout, the wave split.
// Three places write a part out instead of calling it, each for a measured reason stated there: the global-memory build its
// Morton grid and key stages (agx_scene_large.hip), the LDS triangle-level build object_sort_centre's lines and store_node's stores.
// A change to one of those parts goes to these copies too; tests/test_gpu_bvh_tree_pin.py fails when it does not.
// Every device part is AGX_DEV (forced inline): a caller's arrays keep their own address space, LDS or global.  The parts that
// take `keys`, `child`, `counter`, `parent` or node records take PLAIN pointers: the global-memory build re-reads what its own
// workgroup has just written, and a `const __restrict__` there would allow a scalar-cache load of stale data.
#pragma once
#include "agx_common.h"
#include "agx_device_math.h"

namespace agx {

constexpr float kBoxEps = 1.0e-3f;

// ------------------------------------------------------------------------------------------------------------------- host rules
// prims_per_object without its flag bits (AGX_BVH_*: include/aerial_gym_hip.h)
__host__ __device__ constexpr int bvh_ppo(int prims_per_object) {
  return prims_per_object & ~(AGX_BVH_FULL_SORT | AGX_BVH_BOX_OBJECTS | AGX_BVH_OBJECT_TREE);
}
// keys of the bitonic sorts: num_tris rounded up to a power of two
inline int bvh_npad(int nt) {
  int npad = 1;
  while (npad < nt) npad <<= 1;
  return npad;
}
// What the builders ask of prims_per_object, in the order and the words each of them always used.  lds: an LDS builder's launch --
// it also refuses AGX_BVH_OBJECT_TREE without AGX_BVH_BOX_OBJECTS, which the global-memory build accepts and ignores.
inline int bvh_check_objects(int nt, int prims_per_object, bool lds) {
  const int ppo = bvh_ppo(prims_per_object);
  AGX_REQUIRE(!(prims_per_object & AGX_BVH_BOX_OBJECTS) || ppo == 12, "AGX_BVH_BOX_OBJECTS goes with objects of 12 triangles");
  AGX_REQUIRE(!lds || !(prims_per_object & AGX_BVH_OBJECT_TREE) || (prims_per_object & AGX_BVH_BOX_OBJECTS),
              "AGX_BVH_OBJECT_TREE goes with AGX_BVH_BOX_OBJECTS");
  AGX_REQUIRE(ppo == 0 || (ppo >= 9 && nt % ppo == 0), "prims_per_object must be 0 or >= 9%s and divide num_tris",
              lds ? " (8 floats of LDS scratch per object)" : "");
  return AGX_OK;
}
// mask -> work list (work[0] = count, work[1] = cursor, work[2 ...] = dirty env ids): k_compact_mask of agx_scene.hip
int compact_mask_launch(int n, const uint8_t *mask, int32_t *work, void *stream, const int32_t *flag = nullptr);

// ------------------------------------------------------------------------------------------------------------------------- keys
// A key is [code] . [primitive index], 32 bits each.  The code, from the top:
//   bit 31      only in kParkedCode: an obstacle parked outside the env.  The parked primitives make one subtree at the end of the
//               order (in index order), culled at its root.
//   bit 30      the large flag: a primitive longer than kBvhLargeFraction of the Morton grid (the room's wall slabs) gets its own
//               subtree under the root -- its huge box no longer inflates every level of the obstacle tree.
//   bits 29..0  the Morton code of the sort centre on a 10-bit grid over the bounds of the sort centres of everything that is IN
//               the env: a triangle's centroid, or with prims_per_object > 0 the centre of its OBJECT's bounds, so that the
//               triangles of an object stay together (their keys differ in the three lowest bits and the index only).
//   bits 2..0   with prims_per_object > 0 the three finest Morton bits (sub-centimetre cells) are replaced by the triangle's FACE
//               CLASS (zero in an object's own key): inside an object the two triangles of a box face then share the whole upper
//               word and become sibling leaves, which the emit stage folds into one two-triangle leaf -- half the in-object
//               nodes.  A collision of classes only shapes the tree; hits never depend on it.
// The index stays alone in the low word: hipcc dropped an `& 0xFFFFFF` on the LDS read when the class lived there.  It makes the
// keys unique.
constexpr float kBvhLargeFraction = 0.75f;
constexpr uint32_t kParkedCode = 0xFFFFFFFEu;

AGX_DEV unsigned long long pack_key(uint32_t code, int index) { return ((unsigned long long)code << 32) | (unsigned long long)(uint32_t)index; }
AGX_DEV int key_index(unsigned long long key) { return (int)(uint32_t)(key & 0xFFFFFFFFull); }

// obstacle parked outside the env by the curriculum (asset_manager.py:71 puts it at -1000 m)
AGX_DEV bool tri_parked(const float *t) { return t[0] < -900.0f && t[1] < -900.0f && t[2] < -900.0f; }

// bounds of the triangle at t (9 floats)
AGX_DEV void tri_bounds(const float *t, float (&lo)[3], float (&hi)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = fminf(fminf(t[k], t[3 + k]), t[6 + k]);
    hi[k] = fmaxf(fmaxf(t[k], t[3 + k]), t[6 + k]);
  }
}
// box of triangle f, grown by kBoxEps (a leaf's box)
AGX_DEV void leaf_box(const float *__restrict__ tris, int f, float (&o)[6]) {
  float lo[3], hi[3];
  tri_bounds(tris + (size_t)f * 9, lo, hi);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o[k] = lo[k] - kBoxEps;
    o[3 + k] = hi[k] + kBoxEps;
  }
}

AGX_DEV uint32_t expand_bits10(uint32_t v) {
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}
// cells per metre of the Morton grid along an axis of extent ext (-inf - inf = NaN when every primitive is parked)
AGX_DEV float grid_scale(float ext) { return (ext > 0.0f && ext < INFINITY) ? 1023.0f / ext : 0.0f; }
// 30-bit Morton code of a sort centre (3 floats at cen) on the grid (blo, inv)
AGX_DEV uint32_t morton30(const float *cen, const float (&blo)[3], const float (&inv)[3]) {
  uint32_t code = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float qv = fminf(fmaxf((cen[c] - blo[c]) * inv[c], 0.0f), 1023.0f);
    code |= expand_bits10((uint32_t)qv) << (2 - c);
  }
  return code;
}
// the code of a primitive of largest extent `big` whose sort centre has the Morton code `morton`
AGX_DEV uint32_t sort_code(uint32_t morton, float big, float max_ext, bool parked) {
  uint32_t code = morton;
  if (big > kBvhLargeFraction * max_ext) code |= 1u << 30;
  if (parked) code = kParkedCode;
  return code;
}
// face class of a triangle: dominant axis and sign of its normal
AGX_DEV uint32_t face_class(const float *t) {
  const V3 e1 = V3{t[3] - t[0], t[4] - t[1], t[5] - t[2]}, e2 = V3{t[6] - t[0], t[7] - t[1], t[8] - t[2]};
  const V3 nrm = cross_plain(e1, e2);
  const float ax = fabsf(nrm.x), ay = fabsf(nrm.y), az = fabsf(nrm.z);
  const int d = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
  const float comp = d == 0 ? nrm.x : (d == 1 ? nrm.y : nrm.z);
  return (uint32_t)(2 * d + (comp < 0.0f ? 1 : 0));
}
// an object's code with the face class fc in its three lowest bits (0: the object's own key)
AGX_DEV uint32_t class_code(uint32_t code, uint32_t fc) { return (code & ~7u) | fc; }

// The sort-centre record rec[0..3] of an object with the bounds (alo, ahi): centre, largest extent (-1: parked).  The centre joins
// the bounds (lo, hi) of the sort centres unless the object is parked: letting the obstacles the curriculum parks at -1000 m in
// would stretch the 10-bit grid over a kilometre.  The object-level build calls this; the two triangle-level builds write the same
// lines out in their object loops (the call cost the LDS build 3 % on soups: see bvh_build_env; the global-memory build: see there).
AGX_DEV void object_sort_centre(const float (&alo)[3], const float (&ahi)[3], bool parked, float *rec, float (&lo)[3], float (&hi)[3]) {
  float big = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float cen = 0.5f * (alo[c] + ahi[c]);
    rec[c] = cen;
    big = fmaxf(big, ahi[c] - alo[c]);
    if (!parked) { lo[c] = fminf(lo[c], cen); hi[c] = fmaxf(hi[c], cen); }
  }
  rec[3] = parked ? -1.0f : big;
}
// a soup triangle's centroid joins the bounds (lo, hi) of the sort centres unless it is parked
AGX_DEV void soup_sort_centre(const float *t, float (&lo)[3], float (&hi)[3]) {
  if (tri_parked(t)) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float cen = (t[c] + t[3 + c] + t[6 + c]) * (1.0f / 3.0f);
    lo[c] = fminf(lo[c], cen);
    hi[c] = fmaxf(hi[c], cen);
  }
}

// The full-sort key of triangle f (9 floats at t).  ppo > 0: the sort centre is its object's (ocen[8 o ...], object_sort_centre);
// ppo <= 0: its own centroid.
AGX_DEV unsigned long long triangle_key(const float *t, int f, int ppo, const float *ocen, const float (&blo)[3], const float (&inv)[3],
                                        float max_ext) {
  uint32_t morton;
  float big = 0.0f;
  bool parked;
  if (ppo > 0) {
    const float *oc = ocen + 8 * (f / ppo);
    morton = morton30(oc, blo, inv);
    big = oc[3];
    parked = big < 0.0f;
  } else {
    float cen[3], tlo[3], thi[3];
    tri_bounds(t, tlo, thi);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      cen[c] = (t[c] + t[3 + c] + t[6 + c]) * (1.0f / 3.0f);
      big = fmaxf(big, thi[c] - tlo[c]);
    }
    morton = morton30(cen, blo, inv);
    parked = tri_parked(t);
  }
  uint32_t code = sort_code(morton, big, max_ext, parked);
  if (ppo > 0 && !parked) code = class_code(code, face_class(t));
  return pack_key(code, f);
}

AGX_DEV void wave_min_max(float &a, float &b) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a = fminf(a, __shfl_xor(a, off));
    b = fmaxf(b, __shfl_xor(b, off));
  }
}
// Morton grid from the threads' bounds (lo, hi) of the sort centres, over a workgroup of THREADS threads: inside a wave by shuffles
// (min / max are exact: any order gives the same bits), then the waves' results through red[6 THREADS / 64] in LDS -- two
// barriers, the one in here and the caller's before red[] is reused (the pairwise tree over 512 LDS entries took ten).
template <int THREADS>
AGX_DEV void centre_grid(const float (&lo)[3], const float (&hi)[3], float *red, float (&blo)[3], float (&inv)[3], float &max_ext) {
  constexpr int kWaves = THREADS / 64;
  const int tid = threadIdx.x;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float a = lo[c], b = hi[c];
    wave_min_max(a, b);
    if ((tid & 63) == 0) {
      red[c * kWaves + (tid >> 6)] = a;
      red[(3 + c) * kWaves + (tid >> 6)] = b;
    }
  }
  __syncthreads();
  float bhi[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float a = INFINITY, b = -INFINITY;
#pragma unroll
    for (int wv = 0; wv < kWaves; ++wv) {
      a = fminf(a, red[c * kWaves + wv]);
      b = fmaxf(b, red[(3 + c) * kWaves + wv]);
    }
    blo[c] = a;
    bhi[c] = b;
    inv[c] = grid_scale(b - a);
  }
  max_ext = fmaxf(fmaxf(bhi[0] - blo[0], bhi[1] - blo[1]), bhi[2] - blo[2]);
}

// ------------------------------------------------------------------------------------------------------------------- radix tree
AGX_DEV int delta_keys(const unsigned long long *keys, int n, int i, int j) {
  if (j < 0 || j >= n) return -1;
  return __clzll(keys[i] ^ keys[j]);  // keys are unique (the index is in the low word)
}
// Karras 2012: internal node i of the radix tree over n sorted keys (internal nodes 0 .. n - 2, the leaf at sorted position p is
// n - 1 + p) -> its children and j, the other end of its key range
AGX_DEV void karras_node(const unsigned long long *keys, int n, int i, int &left, int &right, int &j) {
  const int n_int = n - 1;
  const int d = (delta_keys(keys, n, i, i + 1) - delta_keys(keys, n, i, i - 1)) >= 0 ? 1 : -1;
  const int dmin = delta_keys(keys, n, i, i - d);
  int lmax = 2;
  while (delta_keys(keys, n, i, i + lmax * d) > dmin) lmax <<= 1;
  int l = 0;
  for (int t = lmax >> 1; t >= 1; t >>= 1)
    if (delta_keys(keys, n, i, i + (l + t) * d) > dmin) l += t;
  j = i + l * d;
  const int dnode = delta_keys(keys, n, i, j);
  int s = 0, t = l;
  do {
    t = (t + 1) >> 1;
    if (delta_keys(keys, n, i, i + (s + t) * d) > dnode) s += t;
  } while (t > 1);
  const int gamma = i + s * d + min(d, 0);
  left = (min(i, j) == gamma) ? (n_int + gamma) : gamma;
  right = (max(i, j) == gamma + 1) ? (n_int + gamma + 1) : (gamma + 1);
}

// ------------------------------------------------------------------------------------------------------------------ box objects
// AGX_BVH_BOX_OBJECTS.  An internal node whose leaves are exactly ONE object's 12 triangles becomes an OBJECT NODE if those triangles
// make an orthogonal box of trimesh.creation.box's topology -- decided from the world-frame triangles alone, every vertex checked.
// Faces of trimesh's box (corners ({0,1}^3 - 0.5) * extents, index 4 x + 2 y + z) by triangle:
//   0 = (1, 3, 0), 1 = (4, 1, 0), 2 = (0, 3, 2), 11 = (7, 5, 6);  -x (0, 2)  +x (10, 11)  -y (1, 5)  +y (7, 9)  -z (3, 8)  +z (4, 6).
AGX_DEV constexpr int pair_a(int fc) { return (int)((0x4371A0u >> (4 * fc)) & 15u); }  // nibble fc of 0x4371A0 / 0x6895B2 (the ray-cast kernel's face table)
AGX_DEV constexpr int pair_b(int fc) { return (int)((0x6895B2u >> (4 * fc)) & 15u); }
// the second triangle of the face whose first triangle is q (pair_a(fc) -> pair_b(fc)); -1: q is a second triangle itself
AGX_DEV int face_mate(int q) { return q == 0 ? 2 : (q == 10 ? 11 : (q == 1 ? 5 : (q == 7 ? 9 : (q == 3 ? 8 : (q == 4 ? 6 : -1))))); }

struct BoxFrame {
  V3 nx, ny, nz, cen;
  float hx, hy, hz, tol;
};

// the box four corners of an object's first triangles span (corners 0, 1, 2, 4; the opposite corner 7 must close it)
AGX_DEV bool box_frame(const float *__restrict__ t, BoxFrame &F) {
  const V3 v1 = V3{t[0], t[1], t[2]}, v0 = V3{t[6], t[7], t[8]};          // triangle 0 = (1, 3, 0)
  const V3 v4 = V3{t[9], t[10], t[11]};                                     // triangle 1 = (4, 1, 0)
  const V3 v2 = V3{t[18 + 6], t[18 + 7], t[18 + 8]};                        // triangle 2 = (0, 3, 2)
  const V3 v7 = V3{t[99], t[100], t[101]};                                  // triangle 11 = (7, 5, 6)
  const V3 ex = v4 - v0, ey = v2 - v0, ez = v1 - v0;
  const float lx = sqrtf(dot(ex, ex)), ly = sqrtf(dot(ey, ey)), lz = sqrtf(dot(ez, ez));
  if (!(lx > 1.0e-5f && ly > 1.0e-5f && lz > 1.0e-5f) || !(lx < 1.0e4f && ly < 1.0e4f && lz < 1.0e4f)) return false;
  F.nx = ex * (1.0f / lx); F.ny = ey * (1.0f / ly); F.nz = ez * (1.0f / lz);
  if (fabsf(dot(F.nx, F.ny)) > 1.0e-4f || fabsf(dot(F.ny, F.nz)) > 1.0e-4f || fabsf(dot(F.nz, F.nx)) > 1.0e-4f) return false;
  const V3 far = v0 + ex + ey + ez - v7;  // the opposite corner is where a box has it
  if (!(sqrtf(dot(far, far)) <= 1.0e-4f * (lx + ly + lz))) return false;
  F.cen = v0 + (ex + ey + ez) * 0.5f;
  F.hx = 0.5f * lx; F.hy = 0.5f * ly; F.hz = 0.5f * lz;
  F.tol = 1.0e-4f * (lx + ly + lz) + 1.0e-5f;
  return true;
}

// triangle q of the object (9 floats at t): three distinct corners of the box, all in the plane of face `kFaceOf[q]`; -> the corners' ids
AGX_DEV bool box_triangle_ok(const BoxFrame &F, const float *__restrict__ t, int q, uint32_t &ids) {
  const int face = (int)((0x113435254020ull >> (4 * q)) & 15ull);  // {0, 2, 0, 4, 5, 2, 5, 3, 4, 3, 1, 1}[q] = 2 * axis + (plus side)
  const int axis = face >> 1;
  const float want = (face & 1) ? 1.0f : -1.0f;
  ids = 0u;
  bool ok = true;
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    const V3 p = V3{t[3 * v] - F.cen.x, t[3 * v + 1] - F.cen.y, t[3 * v + 2] - F.cen.z};
    const float l0 = dot(F.nx, p), l1 = dot(F.ny, p), l2 = dot(F.nz, p);
    ok = ok && !(fabsf(fabsf(l0) - F.hx) > F.tol || fabsf(fabsf(l1) - F.hy) > F.tol || fabsf(fabsf(l2) - F.hz) > F.tol);
    const float la = axis == 0 ? l0 : (axis == 1 ? l1 : l2);
    ok = ok && (la * want > 0.0f);
    ids |= 1u << ((l0 > 0.0f ? 4 : 0) | (l1 > 0.0f ? 2 : 0) | (l2 > 0.0f ? 1 : 0));
  }
  return ok && __popc(ids) == 3;
}

// the object node's record (include/aerial_gym_hip.h): the frame of object `obj`
AGX_DEV void box_object_record(const float *__restrict__ tris, int obj, float *rec) {
  BoxFrame F;
  box_frame(tris + (size_t)obj * 12 * 9, F);  // (validated before)
  rec[0] = F.nx.x; rec[1] = F.nx.y; rec[2] = F.nx.z; rec[3] = F.hx;
  rec[4] = F.ny.x; rec[5] = F.ny.y; rec[6] = F.ny.z; rec[7] = F.hy;
  rec[8] = F.nz.x; rec[9] = F.nz.y; rec[10] = F.nz.z; rec[11] = F.hz;
  rec[12] = F.cen.x; rec[13] = F.cen.y; rec[14] = F.cen.z; rec[15] = __int_as_float(obj * 12);
}

// Which internal nodes of the triangle-level tree are the root of ONE box object?  After the boxes' propagation, by the whole
// workgroup of THREADS threads, in three parallel steps (a thread that validated an object alone was a chain of ~120 dependent
// loads: +20 us on a 60 us build):
//   1. per internal node: is its key range one object's twelve keys?                                       -> objroot[object] = node
//   2. per triangle: are its three vertices corners of its object's box, in the plane of the face the ray-cast's table expects it
//      in; per face pair: do the two triangles have four distinct corners between them (they tile the rectangle)?  -> objroot[o] = -1
//   3. per object: the verdict into bit 0 of counter[node] (read by the node itself and by its parent in the emit stage).
// counter[i] comes in as (other end of node i's key range) << 2 | arrivals and leaves with the arrivals cleared: the range stays
// above bit 1, bit 0 is the verdict (always 0 without box_objects).  objroot[nt / 12] is scratch.  Ends behind a barrier.
template <int THREADS>
AGX_DEV void mark_box_objects(bool box_objects, int nt, const float *__restrict__ tris, const unsigned long long *keys, int *counter,
                              int *objroot) {
  const int tid = threadIdx.x, n_int = nt - 1, n_obj = nt / 12;
  if (box_objects) {
    for (int o = tid; o < n_obj; o += THREADS) objroot[o] = -1;
    __syncthreads();
    for (int i = tid + 1; i < n_int; i += THREADS) {  // (never the root: it has no parent to carry the reference)
      const int j = counter[i] >> 2;
      const int first = min(i, j), last = max(i, j);
      if (last - first != 11) continue;
      const int obj = key_index(keys[first]) / 12;
      bool same = true;
      for (int r = 1; r < 12; ++r) same = same && (key_index(keys[first + r]) / 12 == obj);
      if (same) objroot[obj] = i;  // (one node at most has exactly this range)
    }
    __syncthreads();
    for (int f = tid; f < n_obj * 12; f += THREADS) {
      const int obj = f / 12, q = f - obj * 12;
      if (objroot[obj] < 0) continue;
      const float *t = tris + (size_t)obj * 12 * 9;
      BoxFrame F;
      uint32_t ids = 0u, ids2 = 0u;
      bool ok = box_frame(t, F) && box_triangle_ok(F, t + 9 * q, q, ids);
      // the first triangle of each face also looks at its partner: four distinct corners between them
      const int mate = face_mate(q);
      if (ok && mate >= 0) ok = box_triangle_ok(F, t + 9 * mate, mate, ids2) && __popc(ids | ids2) == 4;
      if (!ok) objroot[obj] = -1;  // (every writer stores the same value)
    }
    __syncthreads();
  }
  for (int i = tid; i < n_int; i += THREADS) counter[i] &= ~3;
  __syncthreads();
  if (box_objects) {
    for (int o = tid; o < n_obj; o += THREADS)
      if (objroot[o] >= 0) counter[objroot[o]] |= 1;
    __syncthreads();
  }
}
// the object of node i of a marked tree, if the node IS an object node (the verdict its parent reads, too)
AGX_DEV bool object_node(const unsigned long long *keys, const int *counter, int i, int &obj) {
  if (!(counter[i] & 1)) return false;
  const int j = counter[i] >> 2;
  obj = key_index(keys[min(i, j)]) / 12;
  return true;
}

// ------------------------------------------------------------------------------------------------------------------------- emit
// Node record written to HBM (16 floats):
//   [0..2] lo_left  [3] child_left (int bits)   [4..6] hi_left  [7] child_right (int bits)
//   [8..10] lo_right [11] second_left (int)     [12..14] hi_right [15] second_right (int)
// child >= 0: internal node index (with AGX_BVH_OBJECT_REF: an object node, the tree ends at the box), child < 0: leaf holding
// triangle ~child and, if second >= 0, that triangle too.
AGX_DEV void store_node(float *o, const float (&a)[6], const float (&b)[6], int rl, int rr, int sl, int sr) {
  o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = __int_as_float(rl);
  o[4] = a[3]; o[5] = a[4]; o[6] = a[5]; o[7] = __int_as_float(rr);
  o[8] = b[0]; o[9] = b[1]; o[10] = b[2]; o[11] = __int_as_float(sl);
  o[12] = b[3]; o[13] = b[4]; o[14] = b[5]; o[15] = __int_as_float(sr);
}
// The reference to child c of a node of the triangle-level tree (n_int internal nodes; counter[] marked by mark_box_objects).  A
// child whose own two children are both leaves is folded into a two-triangle leaf (first triangle in the child slot, `second` in
// the pad slot); the folded node is never visited.
AGX_DEV int child_ref(const unsigned long long *keys, const int *child, const int *counter, int n_int, int c, int &second) {
  second = -1;
  if (c >= n_int) return ~key_index(keys[c - n_int]);
  if (counter[c] & 1) return c | AGX_BVH_OBJECT_REF;
  if (child[2 * c] >= n_int && child[2 * c + 1] >= n_int) {
    second = key_index(keys[child[2 * c + 1] - n_int]);
    return ~key_index(keys[child[2 * c] - n_int]);
  }
  return c;
}

// ------------------------------------------------------------------------------------------------------------------- work list
// The persistent grids' loop: the workgroup pulls envs from the work list (work[0] = count, work[1] = cursor, work[2 ...] = env
// ids) until it is empty.  The second barrier: everybody has read `next` before thread 0 overwrites it -- it also fences the
// reuse of LDS (and of the large build's slab) by the next env.
template <class F>
AGX_DEV void for_each_listed_env(int32_t *work, F body) {
  __shared__ int next;
  const int count = work[0];
  while (true) {
    if (threadIdx.x == 0) next = atomicAdd(&work[1], 1);
    __syncthreads();
    const int idx = next;
    __syncthreads();
    if (idx >= count) break;
    body(work[2 + idx]);
  }
}

}  // namespace agx
