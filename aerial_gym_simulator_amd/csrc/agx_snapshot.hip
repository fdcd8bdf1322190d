// Snapshot / restore / fork of the simulator state: a table of live tensors <-> one block of 32-bit words
// (include/aerial_gym_hip.h, "snapshot / restore / fork").  One launch per call whatever the table holds: every entry owns a run
// of workgroups, a workgroup finds its entry by a scan of the (scalar, kernel-argument) prefix of workgroup counts.
// No LDS, no inter-workgroup synchronisation, plain stores; the block is a buffer of its own, so nothing is copied in place.
#include "agx_common.h"

namespace agx {

constexpr int kSnapThreads = 256;
constexpr int kSnapWordsPerThread = 16;
constexpr int kSnapTile = kSnapThreads * kSnapWordsPerThread;  // words of an entry one workgroup moves

struct SnapBlocks {
  int32_t first[AGX_SNAPSHOT_MAX_ENTRIES + 1];  // first workgroup of entry e; first[count] = grid size
};

__device__ __forceinline__ uint32_t words_of(const AgxSnapshotEntry &e, int n) {
  return e.layout == AGX_SNAP_GLOBAL ? (uint32_t)e.rows : (uint32_t)e.rows * (uint32_t)n;
}

// GATHER: block <- live (mask, src: unused).  !GATHER: live <- block.
template <bool GATHER>
__global__ void __launch_bounds__(kSnapThreads) k_state_copy(AgxSnapshotTable T, SnapBlocks G, int n, uint32_t *__restrict__ block,
                                                             const int32_t *__restrict__ src, const uint8_t *__restrict__ mask) {
  if (!GATHER && src != nullptr) {
    // every wave checks the whole index before it stores anything: a bad entry means that NO wave of the launch writes
    bool bad = false;
    for (int i = threadIdx.x & 63; i < n; i += 64) bad |= (uint32_t)src[i] >= (uint32_t)n;
    if (__ballot(bad) != 0ull) {
      if (blockIdx.x == 0 && threadIdx.x == 0) *T.error = 1u;
      return;
    }
  }
  int e = 0;
  while (e + 1 < T.count && (int)blockIdx.x >= G.first[e + 1]) ++e;  // uniform: scalar loads of the kernel arguments
  const AgxSnapshotEntry E = T.entry[e];
  const uint32_t W = words_of(E, n);
  const uint32_t tile0 = (uint32_t)((int)blockIdx.x - G.first[e]) * (uint32_t)kSnapTile;
  uint32_t *__restrict__ blk = block + (size_t)E.block_row * (size_t)n;
  const bool identity = GATHER || (src == nullptr && mask == nullptr);
  if (E.layout == AGX_SNAP_GLOBAL && mask != nullptr) return;  // global words move only when every env does

  if (identity) {
    const bool blk16 = ((reinterpret_cast<uintptr_t>(blk) & 15u) == 0);
    if (E.elem_size == 4 && blk16 && (reinterpret_cast<uintptr_t>(E.ptr) & 15u) == 0) {
      uint32_t *__restrict__ live = static_cast<uint32_t *>(E.ptr);
#pragma unroll
      for (int k = 0; k < kSnapWordsPerThread / 4; ++k) {
        const uint32_t w = tile0 + ((uint32_t)k * kSnapThreads + threadIdx.x) * 4u;
        if (w + 3u < W) {
          if (GATHER) *reinterpret_cast<uint4 *>(blk + w) = *reinterpret_cast<const uint4 *>(live + w);
          else *reinterpret_cast<uint4 *>(live + w) = *reinterpret_cast<const uint4 *>(blk + w);
        } else {
          for (uint32_t t = w; t < W; ++t) {  // (w + 3 >= W: at most three words, in one lane of the entry's last tile)
            if (GATHER) blk[t] = live[t];
            else live[t] = blk[t];
          }
        }
      }
      return;
    }
    if (E.elem_size == 1 && blk16 && (reinterpret_cast<uintptr_t>(E.ptr) & 3u) == 0) {
      uint8_t *__restrict__ live = static_cast<uint8_t *>(E.ptr);
#pragma unroll
      for (int k = 0; k < kSnapWordsPerThread / 4; ++k) {
        const uint32_t w = tile0 + ((uint32_t)k * kSnapThreads + threadIdx.x) * 4u;
        if (w + 3u < W) {
          if (GATHER) {
            const uint32_t b = *reinterpret_cast<const uint32_t *>(live + w);
            *reinterpret_cast<uint4 *>(blk + w) = make_uint4(b & 255u, (b >> 8) & 255u, (b >> 16) & 255u, b >> 24);
          } else {
            const uint4 v = *reinterpret_cast<const uint4 *>(blk + w);
            *reinterpret_cast<uint32_t *>(live + w) = (v.x & 255u) | ((v.y & 255u) << 8) | ((v.z & 255u) << 16) | (v.w << 24);
          }
        } else {
          for (uint32_t t = w; t < W; ++t) {
            if (GATHER) blk[t] = live[t];
            else live[t] = (uint8_t)blk[t];
          }
        }
      }
      return;
    }
  }

  // word by word: a mask, a source index, or pointers the wide accesses cannot take
  const uint32_t rows = (uint32_t)E.rows, un = (uint32_t)n;
#pragma unroll 4
  for (int k = 0; k < kSnapWordsPerThread; ++k) {
    const uint32_t w = tile0 + (uint32_t)k * kSnapThreads + threadIdx.x;
    if (w >= W) break;
    uint32_t bw = w;
    if (!identity && E.layout != AGX_SNAP_GLOBAL) {
      uint32_t env, r;
      if (E.layout == AGX_SNAP_SOA) { r = w / un; env = w - r * un; }
      else { env = w / rows; r = w - env * rows; }
      if (mask != nullptr && mask[env] == 0) continue;
      const uint32_t s = src != nullptr ? (uint32_t)src[env] : env;  // (range-checked above)
      bw = E.layout == AGX_SNAP_SOA ? r * un + s : s * rows + r;
    }
    if (E.elem_size == 4) {
      uint32_t *__restrict__ live = static_cast<uint32_t *>(E.ptr);
      if (GATHER) blk[bw] = live[w];
      else live[w] = blk[bw];
    } else {
      uint8_t *__restrict__ live = static_cast<uint8_t *>(E.ptr);
      if (GATHER) blk[bw] = live[w];
      else live[w] = (uint8_t)blk[bw];
    }
  }
}

static int snapshot_grid(const AgxSnapshotTable *T, int n, const char *what, SnapBlocks *G) {
  AGX_REQUIRE(T != nullptr, "%s: null table", what);
  AGX_REQUIRE(n > 0, "%s: num_envs must be > 0 (got %d)", what, n);
  AGX_REQUIRE(T->count >= 1 && T->count <= AGX_SNAPSHOT_MAX_ENTRIES, "%s: %d table entries (1 .. %d)", what, T->count,
              AGX_SNAPSHOT_MAX_ENTRIES);
  long long row = 0, blocks = 0;
  for (int e = 0; e < T->count; ++e) {
    const AgxSnapshotEntry &E = T->entry[e];
    AGX_REQUIRE(E.ptr != nullptr, "%s: entry %d has a null pointer", what, e);
    AGX_REQUIRE(E.rows > 0 && (long long)E.rows * n < (1ll << 31), "%s: entry %d: rows %d x %d envs is outside (0, 2^31)", what, e,
                E.rows, n);
    AGX_REQUIRE(E.elem_size == 1 || E.elem_size == 4, "%s: entry %d: element size %d (1 or 4)", what, e, E.elem_size);
    AGX_REQUIRE(E.layout >= AGX_SNAP_SOA && E.layout <= AGX_SNAP_GLOBAL, "%s: entry %d: layout %d", what, e, E.layout);
    AGX_REQUIRE(E.block_row == row, "%s: entry %d starts at block row %d, the entries before it end at %lld", what, e, E.block_row, row);
    row += E.rows;
    const long long words = E.layout == AGX_SNAP_GLOBAL ? (long long)E.rows : (long long)E.rows * n;
    G->first[e] = (int32_t)blocks;
    blocks += (words + kSnapTile - 1) / kSnapTile;
    AGX_REQUIRE(blocks < (1ll << 31), "%s: grid too large", what);
  }
  AGX_REQUIRE(row == T->block_rows, "%s: block_rows %d, the entries hold %lld", what, T->block_rows, row);
  for (int e = T->count; e <= AGX_SNAPSHOT_MAX_ENTRIES; ++e) G->first[e] = (int32_t)blocks;
  return AGX_OK;
}

}  // namespace agx

using namespace agx;

extern "C" int agx_state_gather(const AgxSnapshotTable *table, int n, void *block, void *stream) {
  SnapBlocks G;
  if (int rc = snapshot_grid(table, n, "agx_state_gather", &G)) return rc;
  AGX_REQUIRE(block != nullptr && (reinterpret_cast<uintptr_t>(block) & 3u) == 0, "agx_state_gather: block is null or not word aligned");
  hipLaunchKernelGGL(k_state_copy<true>, dim3(G.first[table->count]), dim3(kSnapThreads), 0, (hipStream_t)stream, *table, G, n,
                     static_cast<uint32_t *>(block), (const int32_t *)nullptr, (const uint8_t *)nullptr);
  return check_launch("agx_state_gather");
}

extern "C" int agx_state_scatter(const AgxSnapshotTable *table, int n, const void *block, const int32_t *src_index, const uint8_t *mask,
                                 void *stream) {
  SnapBlocks G;
  if (int rc = snapshot_grid(table, n, "agx_state_scatter", &G)) return rc;
  AGX_REQUIRE(block != nullptr && (reinterpret_cast<uintptr_t>(block) & 3u) == 0, "agx_state_scatter: block is null or not word aligned");
  AGX_REQUIRE(src_index == nullptr || table->error != nullptr, "agx_state_scatter: src_index needs table->error");
  hipLaunchKernelGGL(k_state_copy<false>, dim3(G.first[table->count]), dim3(kSnapThreads), 0, (hipStream_t)stream, *table, G, n,
                     static_cast<uint32_t *>(const_cast<void *>(block)), src_index, mask);
  if (int rc = check_launch("agx_state_scatter")) return rc;
  if (src_index != nullptr) {
    uint32_t bad = 0;
    hipError_t e = hipMemcpyAsync(&bad, table->error, sizeof(bad), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return fail(AGX_E_LAUNCH, "agx_state_scatter: reading the error word: %s", hipGetErrorString(e));
    if (bad != 0) {
      (void)hipMemsetAsync(table->error, 0, sizeof(bad), (hipStream_t)stream);
      return fail(AGX_E_ARG, "agx_state_scatter: src_index has an entry outside [0, %d): nothing was written", n);
    }
  }
  return AGX_OK;
}
