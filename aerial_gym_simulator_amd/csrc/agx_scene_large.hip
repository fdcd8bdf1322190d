// LBVH build for scenes above the LDS-resident builder's cap (agx_scene.hip, kBvhMaxTris): the same tree as bvh_build_env<false>
// -- the radix tree, the box-object marking, the child references and the leaf boxes are the functions of agx_bvh_parts.h that the
// LDS build calls, too; the Morton grid and the keys are the same rules written out here (bvh_build_large_env says why) -- with
// the working arrays in a caller-provided slab of GLOBAL memory.  What is this file's own: the slab, the tiled sort, and boxes
// that travel up the tree in the parents' records.
// It serves the reference's Warp mesh build / refit behind asset_manager.py:51-71 for whatever mesh a user brings.
//
// ONE workgroup builds ONE env, and each resident workgroup owns one slab (slab = blockIdx.x): nothing is handed from one
// workgroup to another inside the launch, and there is no grid-wide synchronisation.  Everything the kernel re-reads from memory
// was written by the SAME workgroup, and a workgroup sits on one CU: its waves share that CU's vector L1, so the workgroup-scope
// discipline of the LDS build -- __syncthreads() between phases, __threadfence_block() around the arrival atomic -- carries over to
// global memory unchanged.  It would NOT hold between workgroups (another CU's L1 is never refreshed by this CU's stores).
// For the same reason the slab and the node block are read through ordinary vector loads only: their pointers carry no
// `const __restrict__`, so the compiler cannot turn a wave-uniform read of freshly written data into a scalar-cache load (the
// shared parts take them as plain pointers for this build's sake).
//
// Slab of an env of T triangles (npad = T rounded up to a power of two), 40 B per triangle at the most, each array 16-byte aligned:
//     keys    [npad]   u64  [code] . [triangle index] (agx_bvh_parts.h), sorted in place
//     parent  [2T - 1] i32  internal i at i, sorted leaf p at T - 1 + p      (after the propagation: objroot[T / 12])
//     child   [T - 1][2]
//     counter [T - 1]  i32  arrivals in the two low bits, the other end of the node's key range above them
//     ocen    [T / ppo][8]  objects' sort centres (prims_per_object > 0)
// The internal nodes' BOXES have no array: the box of node c is written straight into the record of c's parent (where the
// ray-cast reads it), by the thread that carries it up the tree.
//
// Sort: bitonic over npad keys.  Tiles of 4096 keys are sorted in LDS (32 KiB); of the later merge steps the stages whose
// partner distance is 4096 or more go through global memory (ten stages at 65536 keys), the others run on tiles in LDS again.
#include "agx_bvh_parts.h"

namespace agx {

constexpr int kLargeThreads = 512;
constexpr int kLargeTile = 4096;  // keys of a sort tile in LDS
// DEPTH.  The keys are unique.  Their upper word is [flag | 30-bit Morton], 31 significant bits -- or kParkedCode, which sets
// bit 31 too: 32 --, and the index below this cap has 16: two keys differ in one of at most 48 bit
// positions.  A radix tree node splits on one bit and every level below it on a later one, so a root-to-leaf path has at most
// 48 internal nodes (47 while nothing is parked) -- below the ray-cast's packet stack of kStackDepth = 64 entries, which WRAPS
// SILENTLY.  Raising the cap adds one level per doubling: redo this count before you do.
constexpr int kBvhLargeMaxTris = 65536;
constexpr int kLargeMaxGrid = 256;  // one workgroup per CU; 256 slabs of 2.1 MB at the cap: 0.53 GiB of scratch

__host__ __device__ constexpr size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
struct LargeSlab {
  size_t parent, child, counter, ocen, bytes;  // byte offsets (keys at 0)
};
__host__ __device__ inline LargeSlab large_slab(int nt, int npad) {
  LargeSlab s;
  s.parent = align16((size_t)npad * 8);
  s.child = s.parent + align16((size_t)(2 * nt - 1) * 4);
  s.counter = s.child + align16((size_t)(nt - 1) * 8);
  s.ocen = s.counter + align16((size_t)(nt - 1) * 4);
  s.bytes = s.ocen + align16((size_t)(nt / 9 + 1) * 32);  // objects hold 9 triangles or more
  return s;
}

// stages j = j0, j0 / 2, ... 1 of merge step k of the bitonic network on a tile of m keys in LDS that starts at key `base` of the
// whole sequence.  As in bitonic_sort_lds a thread owns elements tid + q * kLargeThreads, so a wave owns whole 64-element
// blocks: stages with j < 64 exchange inside the wave and need no workgroup barrier.
AGX_DEV void bitonic_tile_stages(unsigned long long *s, int m, int base, int k, int j0, int tid) {
  for (int j = j0; j > 0; j >>= 1) {
    for (int i = tid; i < m; i += kLargeThreads) {
      const int ixj = i ^ j;
      if (ixj > i) {
        const unsigned long long a = s[i], b = s[ixj];
        const bool up = ((base + i) & k) == 0;
        if ((a > b) == up) { s[i] = b; s[ixj] = a; }
      }
    }
    if (j >= 64) {  // this stage wrote, or the next one reads, across waves
      __syncthreads();
    } else {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // compiler: keep the stages' LDS accesses in order
      __builtin_amdgcn_wave_barrier();
    }
  }
  __syncthreads();
}

// ascending sort of keys[0 .. npad) (global memory, this workgroup's slab) by the whole workgroup
AGX_DEV void bitonic_sort_large(unsigned long long *keys, int npad, unsigned long long *tile, int tid) {
  const int m = npad < kLargeTile ? npad : kLargeTile;
  for (int base = 0; base < npad; base += m) {
    for (int i = tid; i < m; i += kLargeThreads) tile[i] = keys[base + i];
    __syncthreads();
    for (int k = 2; k <= m; k <<= 1) bitonic_tile_stages(tile, m, base, k, k >> 1, tid);
    for (int i = tid; i < m; i += kLargeThreads) keys[base + i] = tile[i];
    __syncthreads();
  }
  for (int k = 2 * m; k <= npad; k <<= 1) {
    for (int j = k >> 1; j >= m; j >>= 1) {  // partners in different tiles: through memory, one pair per thread and pass
      for (int p = tid; p < (npad >> 1); p += kLargeThreads) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), ixj = i | j;
        const unsigned long long a = keys[i], b = keys[ixj];
        const bool up = (i & k) == 0;
        if ((a > b) == up) { keys[i] = b; keys[ixj] = a; }
      }
      __syncthreads();  // (workgroup scope: stores drained, and visible to the waves of this CU)
    }
    for (int base = 0; base < npad; base += m) {
      for (int i = tid; i < m; i += kLargeThreads) tile[i] = keys[base + i];
      __syncthreads();
      bitonic_tile_stages(tile, m, base, k, m >> 1, tid);
      for (int i = tid; i < m; i += kLargeThreads) keys[base + i] = tile[i];
      __syncthreads();
    }
  }
}

AGX_DEV void bvh_build_large_env(int env, int nt, int npad, int ppo, const float *__restrict__ tri_world, float *nodes,
                                 unsigned char *slab, unsigned long long *tile, float *red) {
  const bool box_objects = (ppo & AGX_BVH_BOX_OBJECTS) != 0;
  ppo = bvh_ppo(ppo);  // (always the full sort; the object-level build is an LDS builder)
  const LargeSlab lay = large_slab(nt, npad);
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(slab);
  int *parent = reinterpret_cast<int *>(slab + lay.parent);
  int *child = reinterpret_cast<int *>(slab + lay.child);
  int *counter = reinterpret_cast<int *>(slab + lay.counter);
  float *ocen = reinterpret_cast<float *>(slab + lay.ocen);  // [K][8] object_sort_centre's record in the first four
  const int tid = threadIdx.x;
  const float *tris = tri_world + (size_t)env * nt * 9;
  float *out = nodes + (size_t)env * (nt - 1) * 16;

  // --- Morton grid (centre_grid).  The objects' bounds are read from memory directly: the LDS build's detour through per-triangle
  // bounds in LDS has no room here
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const int K = ppo > 0 ? nt / ppo : 0;
  for (int o = tid; o < K; o += kLargeThreads) {
    const float *t = tris + (size_t)o * ppo * 9;
    float alo[3] = {INFINITY, INFINITY, INFINITY}, ahi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int j = 0; j < ppo; ++j) {
      float tlo[3], thi[3];
      tri_bounds(t + 9 * j, tlo, thi);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        alo[c] = fminf(alo[c], tlo[c]);
        ahi[c] = fmaxf(ahi[c], thi[c]);
      }
    }
    // (object_sort_centre's arithmetic, written out: see the note below the loops)
    const bool parked = tri_parked(t);
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
  // From here to the sort the LDS build's calls -- soup_sort_centre, centre_grid, triangle_key, and object_sort_centre above --
  // are written out line for line.  This kernel keeps its speed only with all of them inline in its own text: with any one of
  // them as a call the build of an 8192-triangle soup took 565 us instead of 554 (all 32 combinations timed), at equal
  // registers, scratch and occupancy.  The rules are those of agx_bvh_parts.h; tests/test_gpu_bvh_tree_pin.py holds the two
  // texts together, node block for node block.
  for (int f = tid; f < nt && ppo <= 0; f += kLargeThreads) {
    const float *t = tris + (size_t)f * 9;
    if (tri_parked(t)) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float cen = (t[c] + t[3 + c] + t[6 + c]) * (1.0f / 3.0f);
      lo[c] = fminf(lo[c], cen);
      hi[c] = fmaxf(hi[c], cen);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float a = lo[c], b = hi[c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      a = fminf(a, __shfl_xor(a, off));
      b = fmaxf(b, __shfl_xor(b, off));
    }
    if ((tid & 63) == 0) {
      red[c * (kLargeThreads / 64) + (tid >> 6)] = a;
      red[(3 + c) * (kLargeThreads / 64) + (tid >> 6)] = b;
    }
  }
  __syncthreads();  // the waves' bounds in LDS, the objects' centres in the slab
  float blo[3], bhi[3], inv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float a = INFINITY, b = -INFINITY;
#pragma unroll
    for (int wv = 0; wv < kLargeThreads / 64; ++wv) {
      a = fminf(a, red[c * (kLargeThreads / 64) + wv]);
      b = fmaxf(b, red[(3 + c) * (kLargeThreads / 64) + wv]);
    }
    blo[c] = a;
    bhi[c] = b;
    const float ext = b - a;
    inv[c] = (ext > 0.0f && ext < INFINITY) ? 1023.0f / ext : 0.0f;
  }
  const float max_ext = fmaxf(fmaxf(bhi[0] - blo[0], bhi[1] - blo[1]), bhi[2] - blo[2]);
  // --- keys, padded to npad
  for (int f = tid; f < npad; f += kLargeThreads) {
    unsigned long long key = ~0ull;
    if (f < nt) {
      const float *t = tris + (size_t)f * 9;
      uint32_t code = 0;
      float big = 0.0f;
      bool parked;
      if (ppo > 0) {
        const float *oc = ocen + 8 * (f / ppo);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float qv = fminf(fmaxf((oc[c] - blo[c]) * inv[c], 0.0f), 1023.0f);
          code |= expand_bits10((uint32_t)qv) << (2 - c);
        }
        big = oc[3];
        parked = big < 0.0f;
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float cen = (t[c] + t[3 + c] + t[6 + c]) * (1.0f / 3.0f);
          const float qv = fminf(fmaxf((cen - blo[c]) * inv[c], 0.0f), 1023.0f);
          code |= expand_bits10((uint32_t)qv) << (2 - c);
          big = fmaxf(big, fmaxf(fmaxf(t[c], t[3 + c]), t[6 + c]) - fminf(fminf(t[c], t[3 + c]), t[6 + c]));
        }
        parked = tri_parked(t);
      }
      if (big > kBvhLargeFraction * max_ext) code |= 1u << 30;
      if (parked) code = kParkedCode;
      if (ppo > 0 && !parked) {
        const V3 e1 = V3{t[3] - t[0], t[4] - t[1], t[5] - t[2]}, e2 = V3{t[6] - t[0], t[7] - t[1], t[8] - t[2]};
        const V3 nrm = cross_plain(e1, e2);
        const float ax = fabsf(nrm.x), ay = fabsf(nrm.y), az = fabsf(nrm.z);
        const int d = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
        const float comp = d == 0 ? nrm.x : (d == 1 ? nrm.y : nrm.z);
        code = (code & ~7u) | (uint32_t)(2 * d + (comp < 0.0f ? 1 : 0));
      }
      key = ((unsigned long long)code << 32) | (unsigned long long)(uint32_t)f;
    }
    keys[f] = key;
  }
  __syncthreads();
  bitonic_sort_large(keys, npad, tile, tid);  // (ends behind a barrier)
  // --- radix tree
  const int n_int = nt - 1;
  for (int i = tid; i < n_int; i += kLargeThreads) {
    int left, right, j;
    karras_node(keys, nt, i, left, right, j);
    child[2 * i] = left;
    child[2 * i + 1] = right;
    parent[left] = i;
    parent[right] = i;
    counter[i] = j << 2;  // arrival count in the two low bits; the other end of the node's key range above them
  }
  if (tid == 0) parent[0] = -1;
  __syncthreads();
  // --- bottom-up: a thread carries its box up and leaves it in the parent's record; the second arriver at a node goes on with
  // the union of the two.  Release before the arrival atomic, acquire after it -- at WORKGROUP scope, which is enough only
  // because both arrivers belong to this workgroup, i.e. run on one CU and share its L1 (see the head of the file).
  for (int i = tid; i < nt; i += kLargeThreads) {
    float bx[6];
    leaf_box(tris, key_index(keys[i]), bx);
    int c = n_int + i, node = parent[c];
    while (node >= 0) {
      const int side = child[2 * node + 1] == c ? 1 : 0;
      float *rec = out + (size_t)node * 16;
      float *mine = rec + 8 * side;
      mine[0] = bx[0]; mine[1] = bx[1]; mine[2] = bx[2];
      mine[4] = bx[3]; mine[5] = bx[4]; mine[6] = bx[5];
      __threadfence_block();  // release: this thread's box is written before the arrival
      if ((atomicAdd(&counter[node], 1) & 3) == 0) break;
      __threadfence_block();  // acquire: the sibling's box is read after the arrival
      const float *sib = rec + 8 * (1 - side);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        bx[k] = fminf(bx[k], sib[k]);
        bx[3 + k] = fmaxf(bx[3 + k], sib[4 + k]);
      }
      c = node;
      node = parent[node];
    }
  }
  __syncthreads();
  mark_box_objects<kLargeThreads>(box_objects, nt, tris, keys, counter, parent);  // (objroot[] in parent[], dead since the propagation)
  // --- emit: the child boxes are in place; the references
  for (int i = tid; i < n_int; i += kLargeThreads) {
    float *o = out + (size_t)i * 16;
    int obj;
    if (object_node(keys, counter, i, obj)) {  // the box's frame is its record (nobody reads its child boxes)
      box_object_record(tris, obj, o);
      continue;
    }
    int ref[2], second[2];
#pragma unroll
    for (int side = 0; side < 2; ++side) ref[side] = child_ref(keys, child, counter, n_int, child[2 * i + side], second[side]);
    o[3] = __int_as_float(ref[0]);
    o[7] = __int_as_float(ref[1]);
    o[11] = __int_as_float(second[0]);
    o[15] = __int_as_float(second[1]);
  }
}

// persistent grid: workgroup b owns slab b and builds the envs it pulls from the work list (or every gridDim.x-th env)
__global__ void __launch_bounds__(kLargeThreads) k_bvh_build_large(int n, int nt, int npad, int ppo, const float *__restrict__ tri_world,
                                                                   int32_t *work, float *nodes, unsigned char *scratch, size_t slab_bytes) {
  __shared__ __align__(16) unsigned long long tile[kLargeTile];
  __shared__ float red[6 * (kLargeThreads / 64)];
  unsigned char *slab = scratch + (size_t)blockIdx.x * slab_bytes;
  if (!work) {  // every env
    for (int env = blockIdx.x; env < n; env += gridDim.x) {
      bvh_build_large_env(env, nt, npad, ppo, tri_world, nodes, slab, tile, red);
      __syncthreads();  // slab and LDS are reused by the next env
    }
    return;
  }
  for_each_listed_env(work, [&](int env) { bvh_build_large_env(env, nt, npad, ppo, tri_world, nodes, slab, tile, red); });
}

static int large_grid(int n) { return n < kLargeMaxGrid ? n : kLargeMaxGrid; }

// argument checks of the large build, all before anything touches the GPU
static int large_check(const char *what, int n, int nt, int prims_per_object, const uint8_t *mask, const int32_t *work, const void *scratch,
                       size_t scratch_bytes) {
  AGX_REQUIRE(n > 0, "%s: bad num_envs %d", what, n);
  AGX_REQUIRE(nt >= 2 && nt <= kBvhLargeMaxTris, "%s: num_tris %d outside [2, %d] (global-memory LBVH build)", what, nt, kBvhLargeMaxTris);
  if (int e = bvh_check_objects(nt, prims_per_object, false)) return e;
  AGX_REQUIRE(!mask || work, "%s: a masked rebuild needs the work buffer (int32[num_envs + 2])", what);
  AGX_REQUIRE(scratch, "%s: null scratch buffer", what);
  const size_t need = agx_bvh_large_scratch_bytes(n, nt);
  AGX_REQUIRE(scratch_bytes >= need, "%s: scratch buffer of %zu bytes is smaller than the %zu bytes agx_bvh_large_scratch_bytes(%d, %d) asks for",
              what, scratch_bytes, need, n, nt);
  return AGX_OK;
}

static int large_launch(int n, int nt, int prims_per_object, const float *tri_world, const uint8_t *mask, float *nodes, int32_t *work,
                        void *scratch, void *stream) {
  const int npad = bvh_npad(nt);
  if (mask)
    if (int e = compact_mask_launch(n, mask, work, stream)) return e;
  hipLaunchKernelGGL(k_bvh_build_large, dim3(large_grid(n)), dim3(kLargeThreads), 0, (hipStream_t)stream, n, nt, npad, prims_per_object,
                     tri_world, mask ? work : nullptr, nodes, static_cast<unsigned char *>(scratch), large_slab(nt, npad).bytes);
  return check_launch("agx_bvh_build_large");
}

}  // namespace agx

using namespace agx;

extern "C" size_t agx_bvh_large_scratch_bytes(int n, int nt) {
  if (n <= 0 || nt < 2 || nt > kBvhLargeMaxTris) return 0;
  return (size_t)large_grid(n) * large_slab(nt, bvh_npad(nt)).bytes;
}

extern "C" int agx_bvh_build_large(int n, int nt, int prims_per_object, const float *tri_world, const uint8_t *mask, float *nodes,
                                   int32_t *work, void *scratch, size_t scratch_bytes, void *stream) {
  if (int e = large_check("agx_bvh_build_large", n, nt, prims_per_object, mask, work, scratch, scratch_bytes)) return e;
  AGX_REQUIRE(tri_world && nodes, "agx_bvh_build_large: null buffer");
  return large_launch(n, nt, prims_per_object, tri_world, mask, nodes, work, scratch, stream);
}

extern "C" int agx_scene_refresh_large(int n, int nt, int na, const float *tri_local, const int32_t *tri_asset, const float *asset_state,
                                       const float *half_extents, int prims_per_object, const uint8_t *mask, float *tri_world, float *boxes,
                                       float *nodes, int32_t *work, void *scratch, size_t scratch_bytes, void *stream) {
  if (int e = large_check("agx_scene_refresh_large", n, nt, prims_per_object, mask, work, scratch, scratch_bytes)) return e;
  AGX_REQUIRE(na > 0 && na <= 65535, "agx_scene_refresh_large: num_assets %d outside [1, 65535]", na);
  AGX_REQUIRE(tri_local && tri_asset && asset_state && tri_world && nodes, "agx_scene_refresh_large: null buffer");
  AGX_REQUIRE(!boxes || half_extents, "collision boxes need the half extents");
  // the stand-alone launches of the LDS path's every-env refresh, each looking at the mask itself, then the build
  if (int e = agx_scene_transform(n, nt, na, tri_local, tri_asset, asset_state, mask, tri_world, stream)) return e;
  if (boxes)
    if (int e = agx_boxes_from_assets(n, na, asset_state, half_extents, mask, boxes, stream)) return e;
  return large_launch(n, nt, prims_per_object, tri_world, mask, nodes, work, scratch, stream);
}
