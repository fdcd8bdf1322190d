// The bf16 path of the VAE depth-image encoder: the same implicit GEMM  D[co][pixel] = sum_k W[co][k] X[k][pixel]  as agx_vae.hip,
// on v_mfma_f32_32x32x16_bf16.  DESIGN.md "VAE encoder", the bf16 paragraph.
//
// Activations are [B][H][W][C] bf16 and k = (kh, kw, ci) with ci fastest, so the eight consecutive k a lane supplies to one
// instruction (B[k = 8 (l >> 5) + j][pixel = l & 31]) are eight consecutive channels of ONE input pixel: one 16-byte load, under
// one predicate (a tap outside the image or a pixel past the batch is not addressed at all).  The weights come [Cout][Kp]: the
// lane's A fragment (A[co = l & 31][k = 8 (l >> 5) + j]) is 16 contiguous bytes of its weight row.  A wave owns 32 output pixels
// and CT x 32 output channels, so the gathered B fragment is used CT times.  The result tile has its pixel on the lane and four
// runs of four consecutive channels in the 16 registers: the epilogue stores 8 bytes (bf16) or 16 bytes (fp32) at a time.
// An output element is one chain of instructions k0 = 0, 16, 32, ... whatever CT, the tile or the batch is.
#include "agx_vae.h"

#include <vector>

namespace {
using namespace agx;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

enum { kNhwc16 = 0, kNhwc8 = 1, kImage = 2 };  // how the B operand is gathered

// waves per workgroup: 4, as the fp32 kernel; the waves of a workgroup share nothing (a switch for measuring other counts)
#ifndef AGX_VAE_BF16_WAVES
#define AGX_VAE_BF16_WAVES kVaeWavesPerBlock
#endif
constexpr int kWaves = AGX_VAE_BF16_WAVES;

struct ConvB {
  const void *x;
  const uint16_t *w;
  const float *bias;
  const uint16_t *add;
  void *y;
  const int32_t *row_map, *col_map;
  int cin, cout, kh, kw, stride, pad_h, pad_w, in_h, in_w, out_h, out_w, src_h, src_w;
  int k, kp;   // K = cin kh kw and K rounded up to 16 (the packed weights' row length)
  int pixels;  // batch * out_h * out_w
  int elu, out_f32;
};

AGX_DEV bf16x8 as_frag(uint4 u) { return __builtin_bit_cast(bf16x8, u); }

AGX_DEV uint32_t pack2(float lo, float hi) { return (uint32_t)bf16_rne(lo) | ((uint32_t)bf16_rne(hi) << 16); }

template <int CT>
AGX_DEV void mfma_step(f32x16 (&acc)[CT], const uint16_t *__restrict__ wk, size_t tile_stride, uint4 b) {
  uint4 av[CT];
#pragma unroll
  for (int t = 0; t < CT; ++t) av[t] = *reinterpret_cast<const uint4 *>(wk + (size_t)t * tile_stride);
#pragma unroll
  for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(av[t]), as_frag(b), acc[t], 0, 0, 0);
}

template <int CT, int MODE>
__global__ void __launch_bounds__(64 * kWaves) k_vae_conv_bf16(ConvB a) {
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if ((long long)tile * 32 >= (long long)a.pixels) return;  // the whole wave
  const int col = lane & 31, half = lane >> 5;
  const int pix = tile * 32 + col;
  const bool live = pix < a.pixels;
  const int ohw = a.out_h * a.out_w;
  const int pc = live ? pix : 0;
  const int n = pc / ohw, rem = pc - n * ohw;
  const int oh = rem / a.out_w, ow = rem - oh * a.out_w;
  const int ih0 = oh * a.stride - a.pad_h, iw0 = ow * a.stride - a.pad_w;
  const int co0 = blockIdx.y * (32 * CT);
  // this lane's weight row, at its half of every 16-k step
  const uint16_t *__restrict__ wl = a.w + (size_t)(co0 + col) * (size_t)a.kp + (size_t)(8 * half);
  const size_t tile_stride = (size_t)32 * (size_t)a.kp;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  f32x16 acc[CT];
#pragma unroll
  for (int t = 0; t < CT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

  if (MODE == kNhwc16) {
    // cin % 16 == 0: a 16-k step lies inside one tap, and the tap is the same for the whole wave
    const uint16_t *__restrict__ xn = (const uint16_t *)a.x + (size_t)n * (size_t)a.in_h * (size_t)a.in_w * (size_t)a.cin + (size_t)(8 * half);
    for (int r = 0; r < a.kh; ++r) {
      const int ih = ih0 + r;
      const bool row_ok = live && (unsigned)ih < (unsigned)a.in_h;
      for (int c = 0; c < a.kw; ++c) {
        const int iw = iw0 + c;
        const bool ok = row_ok && (unsigned)iw < (unsigned)a.in_w;
        const uint16_t *__restrict__ px = xn + (ok ? ((size_t)ih * (size_t)a.in_w + (size_t)iw) * (size_t)a.cin : (size_t)0);
        const uint16_t *__restrict__ wt = wl + (size_t)(r * a.kw + c) * (size_t)a.cin;
        for (int cb = 0; cb < a.cin; cb += 16) {
          uint4 b = zero;
          if (ok) b = *reinterpret_cast<const uint4 *>(px + cb);
          mfma_step<CT>(acc, wt + cb, tile_stride, b);
        }
      }
    }
  } else if (MODE == kNhwc8) {
    // cin % 8 == 0 only: the two halves of a step may lie in different taps
    const uint16_t *__restrict__ xn = (const uint16_t *)a.x + (size_t)n * (size_t)a.in_h * (size_t)a.in_w * (size_t)a.cin;
    for (int k0 = 0; k0 < a.kp; k0 += 16) {
      const int kk = k0 + 8 * half;
      const int tap = kk / a.cin, ci = kk - tap * a.cin;
      const int r = tap / a.kw, c = tap - r * a.kw;
      const int ih = ih0 + r, iw = iw0 + c;
      uint4 b = zero;
      if (live && kk < a.k && (unsigned)ih < (unsigned)a.in_h && (unsigned)iw < (unsigned)a.in_w)
        b = *reinterpret_cast<const uint4 *>(xn + ((size_t)ih * (size_t)a.in_w + (size_t)iw) * (size_t)a.cin + (size_t)ci);
      mfma_step<CT>(acc, wl + k0, tile_stride, b);
    }
  } else {
    // the fp32 planar image (cin == 1): taps gathered singly, optionally through the index tables, rounded to bf16 here
    const float *__restrict__ xn = (const float *)a.x + (size_t)n * (size_t)a.src_h * (size_t)a.src_w;
    for (int k0 = 0; k0 < a.kp; k0 += 16) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int kk = k0 + 8 * half + j;
        const int r = kk / a.kw, c = kk - r * a.kw;
        const int ih = ih0 + r, iw = iw0 + c;
        v[j] = 0.0f;
        if (live && kk < a.k && (unsigned)ih < (unsigned)a.in_h && (unsigned)iw < (unsigned)a.in_w) {
          int sr = ih, sc = iw;
          if (a.row_map) {  // (clamped: a table entry outside the source reads its edge, never outside the buffer)
            sr = min(max(a.row_map[ih], 0), a.src_h - 1);
            sc = min(max(a.col_map[iw], 0), a.src_w - 1);
          }
          v[j] = xn[(size_t)sr * (size_t)a.src_w + (size_t)sc];
        }
      }
      const uint4 b = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
      mfma_step<CT>(acc, wl + k0, tile_stride, b);
    }
  }
  if (!live) return;
  // result register i of lane l: channel (i & 3) + 8 (i >> 2) + 4 (l >> 5) of the 32, pixel l & 31
#pragma unroll
  for (int t = 0; t < CT; ++t) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int co = co0 + 32 * t + 8 * g + 4 * half;
      const size_t idx = (size_t)pix * (size_t)a.cout + (size_t)co;
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = acc[t][4 * g + i] + a.bias[co + i];
      if (a.add) {
        const uint2 s = *reinterpret_cast<const uint2 *>(a.add + idx);
        v[0] = v[0] + bf16_widen((uint16_t)(s.x & 0xFFFFu));
        v[1] = v[1] + bf16_widen((uint16_t)(s.x >> 16));
        v[2] = v[2] + bf16_widen((uint16_t)(s.y & 0xFFFFu));
        v[3] = v[3] + bf16_widen((uint16_t)(s.y >> 16));
      }
      if (a.elu) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = vae_elu(v[i]);
      }
      if (a.out_f32) *reinterpret_cast<float4 *>((float *)a.y + idx) = make_float4(v[0], v[1], v[2], v[3]);
      else *reinterpret_cast<uint2 *>((uint16_t *)a.y + idx) = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
    }
  }
}

template <int MODE>
void launch(const ConvB &a, hipStream_t stream) {
  const int tiles = (a.pixels + 31) / 32;
  const int ct = vae_channel_tiles(a.cout, tiles);
  const dim3 grid((unsigned)((tiles + kWaves - 1) / kWaves), (unsigned)(a.cout / (32 * ct))), block(64 * kWaves);
  if (ct == 4) hipLaunchKernelGGL((k_vae_conv_bf16<4, MODE>), grid, block, 0, stream, a);
  else if (ct == 2) hipLaunchKernelGGL((k_vae_conv_bf16<2, MODE>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((k_vae_conv_bf16<1, MODE>), grid, block, 0, stream, a);
}

bool pack_shape_ok(const AgxVaeConv *S) {
  return S && S->cin > 0 && S->cout > 0 && S->kh > 0 && S->kw > 0 && (long long)S->cin * S->kh * S->kw <= (1 << 24);
}
}  // namespace

extern "C" size_t agx_vae_packed_bf16_elems(const AgxVaeConv *S) {
  if (!pack_shape_ok(S)) return 0;
  return (size_t)S->cout * (size_t)round_up16(S->cin * S->kh * S->kw);
}

extern "C" int agx_vae_pack_weight_bf16(const AgxVaeConv *S, const float *w, uint16_t *packed) {
  AGX_REQUIRE(pack_shape_ok(S) && w && packed, "agx_vae_pack_weight_bf16: bad arguments");
  const int k = S->cin * S->kh * S->kw, kp = round_up16(k);
  for (int co = 0; co < S->cout; ++co) {
    uint16_t *row = packed + (size_t)co * kp;
    for (int r = 0; r < S->kh; ++r)
      for (int c = 0; c < S->kw; ++c)
        for (int ci = 0; ci < S->cin; ++ci)
          row[(r * S->kw + c) * S->cin + ci] = bf16_rne(w[(((size_t)co * S->cin + ci) * S->kh + r) * S->kw + c]);
    for (int kk = k; kk < kp; ++kk) row[kk] = 0;
  }
  return AGX_OK;
}

extern "C" int agx_vae_unpack_weight_bf16(const AgxVaeConv *S, const uint16_t *packed, float *w) {
  AGX_REQUIRE(pack_shape_ok(S) && w && packed, "agx_vae_unpack_weight_bf16: bad arguments");
  const int kp = round_up16(S->cin * S->kh * S->kw);
  for (int co = 0; co < S->cout; ++co)
    for (int r = 0; r < S->kh; ++r)
      for (int c = 0; c < S->kw; ++c)
        for (int ci = 0; ci < S->cin; ++ci)
          w[(((size_t)co * S->cin + ci) * S->kh + r) * S->kw + c] = bf16_widen(packed[(size_t)co * kp + (r * S->kw + c) * S->cin + ci]);
  return AGX_OK;
}

extern "C" int agx_vae_conv2d_bf16(int batch, const void *x, const uint16_t *w_packed, const float *bias, const uint16_t *add, void *y,
                                   const AgxVaeConv *S, int flags, const int32_t *row_map, const int32_t *col_map, void *stream) {
  AGX_REQUIRE(S && x && w_packed && bias && y, "agx_vae_conv2d_bf16: null buffer (shape, x, w_packed, bias and y are required)");
  AGX_REQUIRE((flags & ~(AGX_VAE_ELU | AGX_VAE_OUT_F32 | AGX_VAE_IN_IMAGE_F32)) == 0, "agx_vae_conv2d_bf16: flags = %d has unknown bits", flags);
  AGX_REQUIRE(batch > 0 && S->cin > 0 && S->cout > 0 && S->kh > 0 && S->kw > 0 && S->stride > 0 && S->pad_h >= 0 && S->pad_w >= 0 &&
                  S->in_h > 0 && S->in_w > 0 && S->src_h > 0 && S->src_w > 0,
              "agx_vae_conv2d_bf16: sizes out of range");
  AGX_REQUIRE(S->cout % 32 == 0, "agx_vae_conv2d_bf16: cout = %d must be a multiple of 32", S->cout);
  const bool image = (flags & AGX_VAE_IN_IMAGE_F32) != 0;
  AGX_REQUIRE(!image || S->cin == 1, "agx_vae_conv2d_bf16: AGX_VAE_IN_IMAGE_F32 needs cin == 1, not cin = %d", S->cin);
  AGX_REQUIRE(image || S->cin % 8 == 0, "agx_vae_conv2d_bf16: cin = %d must be a multiple of 8 for a [B][H][W][C] bf16 input", S->cin);
  AGX_REQUIRE(S->in_h + 2 * S->pad_h >= S->kh && S->in_w + 2 * S->pad_w >= S->kw && S->out_h == (S->in_h + 2 * S->pad_h - S->kh) / S->stride + 1 &&
                  S->out_w == (S->in_w + 2 * S->pad_w - S->kw) / S->stride + 1,
              "agx_vae_conv2d_bf16: out %d x %d is not (in + 2 pad - k) / stride + 1 of in %d x %d", S->out_h, S->out_w, S->in_h, S->in_w);
  AGX_REQUIRE((row_map != nullptr) == (col_map != nullptr), "agx_vae_conv2d_bf16: row_map and col_map come together");
  AGX_REQUIRE(image || !row_map, "agx_vae_conv2d_bf16: row_map / col_map need AGX_VAE_IN_IMAGE_F32");
  AGX_REQUIRE(row_map || (S->src_h == S->in_h && S->src_w == S->in_w), "agx_vae_conv2d_bf16: without index tables src must equal in");
  AGX_REQUIRE(((uintptr_t)x & (image ? 3 : 15)) == 0, "agx_vae_conv2d_bf16: x must be %d-byte aligned", image ? 4 : 16);
  AGX_REQUIRE(((uintptr_t)w_packed & 15) == 0, "agx_vae_conv2d_bf16: w_packed must be 16-byte aligned");
  AGX_REQUIRE(((uintptr_t)add & 15) == 0, "agx_vae_conv2d_bf16: add must be 16-byte aligned");
  AGX_REQUIRE(((uintptr_t)y & 15) == 0, "agx_vae_conv2d_bf16: y must be 16-byte aligned");
  AGX_REQUIRE(((uintptr_t)bias & 3) == 0, "agx_vae_conv2d_bf16: bias must be 4-byte aligned");
  const long long k = (long long)S->cin * S->kh * S->kw, pixels = (long long)batch * S->out_h * S->out_w;
  AGX_REQUIRE(k <= (1 << 24) && pixels <= 0x7FFFFFFF - 128, "agx_vae_conv2d_bf16: K = %lld or %lld output pixels: too many", k, pixels);
  ConvB a;
  a.x = x; a.w = w_packed; a.bias = bias; a.add = add; a.y = y;
  a.row_map = row_map; a.col_map = col_map;
  a.cin = S->cin; a.cout = S->cout; a.kh = S->kh; a.kw = S->kw; a.stride = S->stride; a.pad_h = S->pad_h; a.pad_w = S->pad_w;
  a.in_h = S->in_h; a.in_w = S->in_w; a.out_h = S->out_h; a.out_w = S->out_w; a.src_h = S->src_h; a.src_w = S->src_w;
  a.k = (int)k; a.kp = round_up16((int)k);
  a.pixels = (int)pixels;
  a.elu = (flags & AGX_VAE_ELU) ? 1 : 0;
  a.out_f32 = (flags & AGX_VAE_OUT_F32) ? 1 : 0;
  if (image) launch<kImage>(a, (hipStream_t)stream);
  else if (a.cin % 16 == 0) launch<kNhwc16>(a, (hipStream_t)stream);
  else launch<kNhwc8>(a, (hipStream_t)stream);
  return check_launch("agx_vae_conv2d_bf16");
}

extern "C" int agx_vae_linear_bf16(int batch, const uint16_t *x, const uint16_t *w_packed, const float *bias, void *y, int in_features,
                                   int out_features, int flags, void *stream) {
  AGX_REQUIRE((flags & AGX_VAE_IN_IMAGE_F32) == 0, "agx_vae_linear_bf16: flags = %d: AGX_VAE_IN_IMAGE_F32 is for convolutions", flags);
  AgxVaeConv S = {};
  S.cin = in_features; S.cout = out_features;
  S.kh = S.kw = S.stride = 1;
  S.in_h = S.in_w = S.out_h = S.out_w = S.src_h = S.src_w = 1;
  return agx_vae_conv2d_bf16(batch, x, w_packed, bias, nullptr, y, &S, flags, nullptr, nullptr, stream);
}
