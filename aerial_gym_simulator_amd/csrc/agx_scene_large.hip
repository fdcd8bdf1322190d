// LBVH build for scenes above the LDS-resident builder's cap (agx_scene.hip, kBvhMaxTris): the same tree as bvh_build_env<false>
// -- same keys, same order, same radix tree, same records -- with the working arrays in a caller-provided slab of GLOBAL memory.
// It serves the reference's Warp mesh build / refit behind asset_manager.py:51-71 for whatever mesh a user brings.
//
// ONE workgroup builds ONE env, and each resident workgroup owns one slab (slab = blockIdx.x): nothing is handed from one
// workgroup to another inside the launch, and there is no grid-wide synchronisation.  Everything the kernel re-reads from memory
// was written by the SAME workgroup, and a workgroup sits on one CU: its waves share that CU's vector L1, so the workgroup-scope
// discipline of the LDS build -- __syncthreads() between phases, __threadfence_block() around the arrival atomic -- carries over to
// global memory unchanged.  It would NOT hold between workgroups (another CU's L1 is never refreshed by this CU's stores).
// For the same reason the slab and the node block are read through ordinary vector loads only: their pointers carry no
// `const __restrict__`, so the compiler cannot turn a wave-uniform read of freshly written data into a scalar-cache load.
//
// Slab of an env of T triangles (npad = T rounded up to a power of two), 40 B per triangle at the most, each array 16-byte aligned:
//     keys    [npad]   u64  [flag | 30-bit Morton] . [triangle index], sorted in place
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
// DEPTH.  The keys are unique.  Their upper word is [flag | 30-bit Morton], 31 significant bits -- or the parked marker
// 0xFFFFFFFE, which sets bit 31 too: 32 --, and the index below this cap has 16: two keys differ in one of at most 48 bit
// positions.  A radix tree node splits on one bit and every level below it on a later one, so a root-to-leaf path has at most
// 48 internal nodes (47 while nothing is parked) -- below the ray-cast's packet stack of kStackDepth = 64 entries, which WRAPS
// SILENTLY.  Raising the cap adds one level per doubling: redo this count before you do.
constexpr int kBvhLargeMaxTris = 65536;
constexpr int kLargeMaxGrid = 256;  // one workgroup per CU; 256 slabs of 2.1 MB at the cap: 0.53 GiB of scratch

__host__ __device__ constexpr size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
static int large_npad(int nt) {
  int npad = 1;
  while (npad < nt) npad <<= 1;
  return npad;
}
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

// box of triangle f, grown by kBoxEps (a leaf's box)
AGX_DEV void leaf_box(const float *__restrict__ tris, int f, float (&o)[6]) {
  const float *t = tris + (size_t)f * 9;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o[k] = fminf(fminf(t[k], t[3 + k]), t[6 + k]) - kBoxEps;
    o[3 + k] = fmaxf(fmaxf(t[k], t[3 + k]), t[6 + k]) + kBoxEps;
  }
}

AGX_DEV void bvh_build_large_env(int env, int nt, int npad, int ppo, const float *__restrict__ tri_world, float *nodes,
                                 unsigned char *slab, unsigned long long *tile, float *red) {
  const bool box_objects = (ppo & AGX_BVH_BOX_OBJECTS) != 0;
  ppo &= ~(AGX_BVH_FULL_SORT | AGX_BVH_BOX_OBJECTS | AGX_BVH_OBJECT_TREE);  // (always the full sort; the object-level build is an LDS builder)
  const LargeSlab lay = large_slab(nt, npad);
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(slab);
  int *parent = reinterpret_cast<int *>(slab + lay.parent);
  int *child = reinterpret_cast<int *>(slab + lay.child);
  int *counter = reinterpret_cast<int *>(slab + lay.counter);
  float *ocen = reinterpret_cast<float *>(slab + lay.ocen);  // [K][8] centre, largest extent (< 0: parked), -
  const int tid = threadIdx.x;
  const float *tris = tri_world + (size_t)env * nt * 9;
  float *out = nodes + (size_t)env * (nt - 1) * 16;

  // --- Morton grid = bounds of the sort centres of everything that is in the env (parked obstacles stay out); with ppo > 0 the
  // sort centre is the OBJECT's (bvh_build_env, agx_scene.hip: the same arithmetic, min / max are exact in any order)
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const int K = ppo > 0 ? nt / ppo : 0;
  for (int o = tid; o < K; o += kLargeThreads) {
    const float *t = tris + (size_t)o * ppo * 9;
    float alo[3] = {INFINITY, INFINITY, INFINITY}, ahi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int j = 0; j < ppo; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        alo[c] = fminf(alo[c], fminf(fminf(t[9 * j + c], t[9 * j + 3 + c]), t[9 * j + 6 + c]));
        ahi[c] = fmaxf(ahi[c], fmaxf(fmaxf(t[9 * j + c], t[9 * j + 3 + c]), t[9 * j + 6 + c]));
      }
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
    inv[c] = (ext > 0.0f && ext < INFINITY) ? 1023.0f / ext : 0.0f;  // ext = -inf - inf when every primitive is parked
  }
  const float max_ext = fmaxf(fmaxf(bhi[0] - blo[0], bhi[1] - blo[1]), bhi[2] - blo[2]);
  // --- keys: [large flag | 30-bit Morton code of the sort centre] . [triangle index]   (bvh_build_env's full-sort keys)
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
      if (big > kBvhLargeFraction * max_ext) code |= 1u << 30;  // wall slabs: their own subtree under the root
      if (parked) code = 0xFFFFFFFEu;                            // one subtree at the end of the order, culled at its root
      if (ppo > 0 && !parked) {  // the three finest Morton bits become the triangle's face class: two-triangle leaves
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
  // --- Karras 2012 radix tree: internal nodes 0..nt-2, leaves nt-1+i (i = sorted position)
  const int n_int = nt - 1;
  for (int i = tid; i < n_int; i += kLargeThreads) {
    const int d = (delta_keys(keys, nt, i, i + 1) - delta_keys(keys, nt, i, i - 1)) >= 0 ? 1 : -1;
    const int dmin = delta_keys(keys, nt, i, i - d);
    int lmax = 2;
    while (delta_keys(keys, nt, i, i + lmax * d) > dmin) lmax <<= 1;
    int l = 0;
    for (int t = lmax >> 1; t >= 1; t >>= 1)
      if (delta_keys(keys, nt, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = delta_keys(keys, nt, i, j);
    int s = 0, t = l;
    do {
      t = (t + 1) >> 1;
      if (delta_keys(keys, nt, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int gamma = i + s * d + min(d, 0);
    const int left = (min(i, j) == gamma) ? (n_int + gamma) : gamma;
    const int right = (max(i, j) == gamma + 1) ? (n_int + gamma + 1) : (gamma + 1);
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
    leaf_box(tris, (int)(uint32_t)(keys[i] & 0xFFFFFFFFull), bx);
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
  // --- AGX_BVH_BOX_OBJECTS: which internal nodes are the root of ONE box object?  (the three steps of agx_bvh_parts.h; the verdict
  // goes into bit 0 of counter[], objroot[] lives in parent[], dead since the propagation)
  int *objroot = parent;  // [nt / 12]
  const int n_obj = nt / 12;
  if (box_objects) {
    for (int o = tid; o < n_obj; o += kLargeThreads) objroot[o] = -1;
    __syncthreads();
    for (int i = tid + 1; i < n_int; i += kLargeThreads) {  // (never the root: it has no parent to carry the reference)
      const int j = counter[i] >> 2;
      const int first = min(i, j), last = max(i, j);
      if (last - first != 11) continue;
      const int obj = (int)(uint32_t)(keys[first] & 0xFFFFFFFFull) / 12;
      bool same = true;
      for (int r = 1; r < 12; ++r) same = same && ((int)(uint32_t)(keys[first + r] & 0xFFFFFFFFull) / 12 == obj);
      if (same) objroot[obj] = i;  // (one node at most has exactly this range)
    }
    __syncthreads();
    for (int f = tid; f < n_obj * 12; f += kLargeThreads) {
      const int obj = f / 12, q = f - obj * 12;
      if (objroot[obj] < 0) continue;
      const float *t = tris + (size_t)obj * 12 * 9;
      BoxFrame F;
      uint32_t ids = 0u, ids2 = 0u;
      bool ok = box_frame(t, F) && box_triangle_ok(F, t + 9 * q, q, ids);
      const int mate = q == 0 ? 2 : (q == 10 ? 11 : (q == 1 ? 5 : (q == 7 ? 9 : (q == 3 ? 8 : (q == 4 ? 6 : -1)))));
      if (ok && mate >= 0) ok = box_triangle_ok(F, t + 9 * mate, mate, ids2) && __popc(ids | ids2) == 4;
      if (!ok) objroot[obj] = -1;  // (every writer stores the same value)
    }
    __syncthreads();
  }
  for (int i = tid; i < n_int; i += kLargeThreads) counter[i] &= ~3;
  __syncthreads();
  if (box_objects) {
    for (int o = tid; o < n_obj; o += kLargeThreads)
      if (objroot[o] >= 0) counter[objroot[o]] |= 1;
    __syncthreads();
  }
  // --- emit: the child boxes are in place; the references.  A child whose own two children are both leaves is folded into a
  // two-triangle leaf (first triangle in the child slot, second in the pad slot); the folded node is never visited.
  for (int i = tid; i < n_int; i += kLargeThreads) {
    float *o = out + (size_t)i * 16;
    if (counter[i] & 1) {  // this node IS an object node: the box's frame is its record (nobody reads its child boxes)
      const int j = counter[i] >> 2;
      box_object_record(tris, (int)(uint32_t)(keys[min(i, j)] & 0xFFFFFFFFull) / 12, o);
      continue;
    }
    int ref[2], second[2];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const int c = child[2 * i + side];
      second[side] = -1;
      if (c >= n_int) {
        ref[side] = ~(int)(uint32_t)(keys[c - n_int] & 0xFFFFFFFFull);
      } else if (counter[c] & 1) {
        ref[side] = c | AGX_BVH_OBJECT_REF;  // the child is an OBJECT NODE: the tree ends at the box
      } else if (child[2 * c] >= n_int && child[2 * c + 1] >= n_int) {
        ref[side] = ~(int)(uint32_t)(keys[child[2 * c] - n_int] & 0xFFFFFFFFull);
        second[side] = (int)(uint32_t)(keys[child[2 * c + 1] - n_int] & 0xFFFFFFFFull);
      } else {
        ref[side] = c;
      }
    }
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
  __shared__ int next;
  unsigned char *slab = scratch + (size_t)blockIdx.x * slab_bytes;
  if (!work) {  // every env
    for (int env = blockIdx.x; env < n; env += gridDim.x) {
      bvh_build_large_env(env, nt, npad, ppo, tri_world, nodes, slab, tile, red);
      __syncthreads();  // slab and LDS are reused by the next env
    }
    return;
  }
  const int count = work[0];
  while (true) {
    if (threadIdx.x == 0) next = atomicAdd(&work[1], 1);
    __syncthreads();
    const int idx = next;
    __syncthreads();  // everybody has read `next` before thread 0 overwrites it; also fences the reuse of slab and LDS
    if (idx >= count) break;
    bvh_build_large_env(work[2 + idx], nt, npad, ppo, tri_world, nodes, slab, tile, red);
  }
}

static int large_grid(int n) { return n < kLargeMaxGrid ? n : kLargeMaxGrid; }

// argument checks of the large build, all before anything touches the GPU
static int large_check(const char *what, int n, int nt, int prims_per_object, const uint8_t *mask, const int32_t *work, const void *scratch,
                       size_t scratch_bytes) {
  AGX_REQUIRE(n > 0, "%s: bad num_envs %d", what, n);
  AGX_REQUIRE(nt >= 2 && nt <= kBvhLargeMaxTris, "%s: num_tris %d outside [2, %d] (global-memory LBVH build)", what, nt, kBvhLargeMaxTris);
  const int ppo = prims_per_object & ~(AGX_BVH_FULL_SORT | AGX_BVH_BOX_OBJECTS | AGX_BVH_OBJECT_TREE);
  AGX_REQUIRE(!(prims_per_object & AGX_BVH_BOX_OBJECTS) || ppo == 12, "AGX_BVH_BOX_OBJECTS goes with objects of 12 triangles");
  AGX_REQUIRE(ppo == 0 || (ppo >= 9 && nt % ppo == 0), "prims_per_object must be 0 or >= 9 and divide num_tris");
  AGX_REQUIRE(!mask || work, "%s: a masked rebuild needs the work buffer (int32[num_envs + 2])", what);
  AGX_REQUIRE(scratch, "%s: null scratch buffer", what);
  const size_t need = agx_bvh_large_scratch_bytes(n, nt);
  AGX_REQUIRE(scratch_bytes >= need, "%s: scratch buffer of %zu bytes is smaller than the %zu bytes agx_bvh_large_scratch_bytes(%d, %d) asks for",
              what, scratch_bytes, need, n, nt);
  return AGX_OK;
}

static int large_launch(int n, int nt, int prims_per_object, const float *tri_world, const uint8_t *mask, float *nodes, int32_t *work,
                        void *scratch, void *stream) {
  const int npad = large_npad(nt);
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
  return (size_t)large_grid(n) * large_slab(nt, large_npad(nt)).bytes;
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
