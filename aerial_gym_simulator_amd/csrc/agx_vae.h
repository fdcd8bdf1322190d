// What the fp32 (agx_vae.hip) and the bf16 (agx_vae_bf16.hip) kernels of the VAE encoder share: the tile both are built on (a wave
// owns 32 output pixels and CT x 32 output channels of a 32x32 matrix-instruction result), the choice of CT, the ELU of the
// epilogue, and bf16 <-> fp32 on host and device.
#pragma once
#include "agx_common.h"
#include "agx_device_math.h"

namespace agx {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kVaeWavesPerBlock = 4;

inline int round_up8(int k) { return (k + 7) & ~7; }
inline int round_up16(int k) { return (k + 15) & ~15; }
inline size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// channel tiles per wave: 4 when that still leaves the device full of waves (the gathered operand is then used four times);
// the choice moves no result bit
inline int vae_channel_tiles(int cout, int tiles) {
  int ct = 4;
  while (ct > 1 && (cout % (32 * ct) != 0 || (long long)tiles * (cout / (32 * ct)) < 2048)) ct >>= 1;
  return ct;
}

AGX_DEV float vae_elu(float v) { return (v > 0.0f) ? v : expm1_cw(v); }

// fp32 -> bf16, round to nearest even (a NaN stays a quiet NaN); bf16 -> fp32 is exact
__host__ __device__ inline uint16_t bf16_rne(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x0040u);
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
__host__ __device__ inline float bf16_widen(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

}  // namespace agx
