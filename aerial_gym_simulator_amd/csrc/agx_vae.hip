// VAE depth-image encoder (aerial_gym/utils/vae/VAE.py ImgEncoder, the sampling of VAE.encode): nine convolutions, two dense
// layers and the reparametrisation.  DESIGN.md "VAE encoder".
//
// One kernel does every layer: an implicit GEMM  D[co][pixel] = sum_k W[co][k] X[k][pixel]  on the exact-fp32 matrix
// instruction v_mfma_f32_32x32x2_f32, k = (ci, kh, kw) flattened in torch's weight order.  A wave owns 32 output pixels and
// CT x 32 output channels.  Per instruction lane l supplies A = W[co = l & 31][k0 + (l >> 5)] and B = X[k0 + (l >> 5)][pixel = l & 31];
// the hardware adds the two products in k order, so an output element is the fmaf chain k = 0, 1, 2, ... whatever CT, the tile
// or the batch is.  X is never materialised: a lane gathers its tap from the NCHW input (zero outside the image and past K), for
// conv0 optionally through a row and a column index table (the nearest-neighbour resize).  The weights come repacked [K8][Cout]:
// the 32 lanes of a half-wave read 32 consecutive floats.  The result tile has its pixel on the lane and its channels in the 16
// registers: every store instruction writes 32 consecutive pixels of one channel plane.
#include "agx_common.h"
#include "agx_device_math.h"
#include "agx_rng.h"
#include "agx_task_parts.h"
#include "agx_vae.h"

#include <vector>

namespace {
using namespace agx;

constexpr int kLatent = 64;
constexpr int kWavesPerBlock = kVaeWavesPerBlock;

struct ConvK {
  const float *x, *w, *bias, *add;
  float *y;
  const int32_t *row_map, *col_map;
  int cin, cout, kh, kw, stride, pad_h, pad_w, in_h, in_w, out_h, out_w, src_h, src_w;
  int k8;      // K rounded up to a multiple of 8 (the packed weights' rows)
  int pixels;  // batch * out_h * out_w
  int elu;
};

template <int CT>
__global__ void __launch_bounds__(64 * kWavesPerBlock) k_vae_conv(ConvK a) {
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if ((long long)tile * 32 >= (long long)a.pixels) return;  // the whole wave (64-bit: the last block's tiles may lie past 2^31)
  const int col = lane & 31, half = lane >> 5;
  const int pix = tile * 32 + col;
  const bool live = pix < a.pixels;
  const int ohw = a.out_h * a.out_w;
  const int pc = live ? pix : 0;
  const int n = pc / ohw, rem = pc - n * ohw;
  const int oh = rem / a.out_w, ow = rem - oh * a.out_w;
  const int ih0 = oh * a.stride - a.pad_h, iw0 = ow * a.stride - a.pad_w;
  const size_t plane = (size_t)a.src_h * (size_t)a.src_w;
  const float *__restrict__ xn = a.x + (size_t)n * (size_t)a.cin * plane;
  // this lane's tap (ci, r, c) of k = k0 + half; it advances by two per instruction
  const int khw = a.kh * a.kw;
  int ci = half / khw;
  int r = (half - ci * khw) / a.kw;
  int c = half - ci * khw - r * a.kw;
  const int co0 = blockIdx.y * (32 * CT);
  const float *__restrict__ wl = a.w + (size_t)half * (size_t)a.cout + (size_t)(co0 + col);
  f32x16 acc[CT];
#pragma unroll
  for (int t = 0; t < CT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

  for (int k0 = 0; k0 < a.k8; k0 += 8) {
    float b[4], wv[4][CT];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ih = ih0 + r, iw = iw0 + c;
      float v = 0.0f;
      if (live && ci < a.cin && (unsigned)ih < (unsigned)a.in_h && (unsigned)iw < (unsigned)a.in_w) {
        int sr = ih, sc = iw;
        if (a.row_map) {  // (clamped: a table entry outside the source reads its edge, never outside the buffer)
          sr = min(max(a.row_map[ih], 0), a.src_h - 1);
          sc = min(max(a.col_map[iw], 0), a.src_w - 1);
        }
        v = xn[(size_t)ci * plane + (size_t)sr * (size_t)a.src_w + (size_t)sc];
      }
      b[u] = v;
#pragma unroll
      for (int t = 0; t < CT; ++t) wv[u][t] = wl[(size_t)(k0 + 2 * u) * (size_t)a.cout + (size_t)(32 * t)];
      c += 2;
      while (c >= a.kw) { c -= a.kw; ++r; }
      while (r >= a.kh) { r -= a.kh; ++ci; }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[u][t], b[u], acc[t], 0, 0, 0);
  }
  if (!live) return;
  // result register i of lane l: channel (i & 3) + 8 (i >> 2) + 4 (l >> 5) of the 32, pixel l & 31
#pragma unroll
  for (int t = 0; t < CT; ++t) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int co = co0 + 32 * t + (i & 3) + 8 * (i >> 2) + 4 * half;
      const size_t idx = ((size_t)n * (size_t)a.cout + (size_t)co) * (size_t)ohw + (size_t)rem;
      float v = acc[t][i] + a.bias[co];
      if (a.add) v = v + a.add[idx];
      if (a.elu) v = vae_elu(v);
      a.y[idx] = v;
    }
  }
}

// normal j of env `genv` at env step `step`: pair p = j / 2 from uniforms (2 p, 2 p + 1) = entries 2 (p & 1), 2 (p & 1) + 1 of block p / 2
AGX_DEV float vae_normal(uint64_t seed, int genv, int step, int j) {
  const F4 f = rng_block(seed, genv, step, RNG_VAE_EPS, j >> 2);
  const int e = j & 2;
  float z0, z1;
  normal_pair(e ? f.v[2] : f.v[0], e ? f.v[3] : f.v[1], z0, z1);
  return (j & 1) ? z1 : z0;
}

__global__ void k_vae_sample(int n, const float *__restrict__ z, const float *__restrict__ eps, float *__restrict__ latents,
                             float *__restrict__ means, float *__restrict__ stdv, uint64_t seed, int env_base, int step) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * kLatent) return;
  const int env = i / kLatent, j = i - env * kLatent;
  const float mean = z[(size_t)env * (2 * kLatent) + j];
  const float logvar = z[(size_t)env * (2 * kLatent) + kLatent + j];
  const float sd = exp_cw(0.5f * logvar);
  const float e = eps ? eps[i] : vae_normal(seed, env_base + env, step, j);
  const float t = e * sd;
  latents[i] = mean + t;
  if (means) means[i] = mean;
  if (stdv) stdv[i] = sd;
}

__global__ void k_vae_noise(int n, uint64_t seed, int env_base, int step, float *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * kLatent) return;
  const int env = i / kLatent;
  out[i] = vae_normal(seed, env_base + env, step, i - env * kLatent);
}

__global__ void k_vae_place(int n, const float *__restrict__ latents, float *__restrict__ obs, int obs_dim, int obs_offset) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * kLatent) return;
  const int env = i / kLatent;
  obs[(size_t)env * (size_t)obs_dim + (size_t)(obs_offset + (i - env * kLatent))] = latents[i];
}

// ---- the encoder's layer table: Cin, Cout, kernel, stride, pad (h, w), the layer whose output it reads (-1: the image) ----
struct LayerDef {
  int cin, cout, k, stride, pad_h, pad_w, input;
};
constexpr int kConvLayers = 9;
const LayerDef kLayers[AGX_VAE_LAYERS] = {
    {1, 32, 5, 2, 2, 2, -1},    // 0 conv0
    {32, 32, 3, 2, 2, 2, 0},    // 1 conv0_1        (ELU)
    {32, 32, 5, 2, 1, 1, 1},    // 2 conv1_0
    {32, 64, 3, 1, 1, 1, 2},    // 3 conv1_1        (+ conv0_jump_2, ELU)
    {32, 64, 4, 2, 1, 1, 1},    // 4 conv0_jump_2
    {64, 64, 5, 2, 2, 2, 3},    // 5 conv2_0
    {64, 128, 3, 2, 1, 1, 5},   // 6 conv2_1        (+ conv1_jump_3, ELU)
    {64, 128, 5, 4, 2, 1, 3},   // 7 conv1_jump_3
    {128, 128, 5, 2, 0, 0, 6},  // 8 conv3_0
    {2304, 512, 1, 1, 0, 0, 8}, // 9 dense0         (ELU)
    {512, 128, 1, 1, 0, 0, 9},  // 10 dense1
};
// the order the layers run in (a jump convolution before the sum that reads it)
const int kOrder[AGX_VAE_LAYERS] = {0, 1, 2, 4, 3, 5, 7, 6, 8, 9, 10};

bool geometry(int image_h, int image_w, int hw[AGX_VAE_LAYERS][2]) {
  for (int l = 0; l < kConvLayers; ++l) {
    const LayerDef &L = kLayers[l];
    const int ih = L.input < 0 ? image_h : hw[L.input][0], iw = L.input < 0 ? image_w : hw[L.input][1];
    if (ih + 2 * L.pad_h < L.k || iw + 2 * L.pad_w < L.k) return false;
    hw[l][0] = (ih + 2 * L.pad_h - L.k) / L.stride + 1;
    hw[l][1] = (iw + 2 * L.pad_w - L.k) / L.stride + 1;
  }
  hw[9][0] = hw[9][1] = hw[10][0] = hw[10][1] = 1;
  return hw[3][0] == hw[4][0] && hw[3][1] == hw[4][1] && hw[6][0] == hw[7][0] && hw[6][1] == hw[7][1] && hw[8][0] == 3 && hw[8][1] == 6;
}

}  // namespace

struct AgxVaeEncoder {
  int image_h, image_w;
  int precision;  // AGX_VAE_FP32 / AGX_VAE_BF16
  int hw[AGX_VAE_LAYERS][2];
  size_t out_bytes[AGX_VAE_LAYERS];  // per env: fp32, or bf16 for every layer but dense1
  void *w[AGX_VAE_LAYERS];           // device, packed: float [K8][Cout], or bf16 [Cout][Kp]
  float *b[AGX_VAE_LAYERS];          // device
};

extern "C" size_t agx_vae_packed_floats(int cout, int k) {
  if (cout <= 0 || k <= 0) return 0;
  return (size_t)round_up8(k) * (size_t)cout;
}

extern "C" int agx_vae_pack_weight(int cout, int k, const float *w, float *packed) {
  AGX_REQUIRE(cout > 0 && k > 0 && w && packed, "agx_vae_pack_weight: bad arguments");
  const int k8 = round_up8(k);
  for (int kk = 0; kk < k8; ++kk)
    for (int co = 0; co < cout; ++co) packed[(size_t)kk * cout + co] = kk < k ? w[(size_t)co * k + kk] : 0.0f;
  return AGX_OK;
}

extern "C" int agx_vae_unpack_weight(int cout, int k, const float *packed, float *w) {
  AGX_REQUIRE(cout > 0 && k > 0 && w && packed, "agx_vae_unpack_weight: bad arguments");
  for (int co = 0; co < cout; ++co)
    for (int kk = 0; kk < k; ++kk) w[(size_t)co * k + kk] = packed[(size_t)kk * cout + co];
  return AGX_OK;
}

extern "C" int agx_vae_conv2d(int batch, const float *x, const float *w_packed, const float *bias, const float *add, float *y,
                              const AgxVaeConv *S, int flags, const int32_t *row_map, const int32_t *col_map, void *stream) {
  AGX_REQUIRE(S && x && w_packed && bias && y, "agx_vae_conv2d: null buffer");
  AGX_REQUIRE(batch > 0 && S->cin > 0 && S->cout > 0 && S->cout % 32 == 0 && S->kh > 0 && S->kw > 0 && S->stride > 0 && S->pad_h >= 0 &&
                  S->pad_w >= 0 && S->in_h > 0 && S->in_w > 0 && S->src_h > 0 && S->src_w > 0,
              "agx_vae_conv2d: sizes out of range (cout = %d must be a multiple of 32)", S->cout);
  AGX_REQUIRE(S->in_h + 2 * S->pad_h >= S->kh && S->in_w + 2 * S->pad_w >= S->kw && S->out_h == (S->in_h + 2 * S->pad_h - S->kh) / S->stride + 1 &&
                  S->out_w == (S->in_w + 2 * S->pad_w - S->kw) / S->stride + 1,
              "agx_vae_conv2d: out %d x %d is not (in + 2 pad - k) / stride + 1 of in %d x %d", S->out_h, S->out_w, S->in_h, S->in_w);
  AGX_REQUIRE((row_map != nullptr) == (col_map != nullptr), "agx_vae_conv2d: row_map and col_map come together");
  AGX_REQUIRE(row_map || (S->src_h == S->in_h && S->src_w == S->in_w), "agx_vae_conv2d: without index tables src must equal in");
  AGX_REQUIRE((flags & ~AGX_VAE_ELU) == 0, "agx_vae_conv2d: flags = %d", flags);
  const long long k = (long long)S->cin * S->kh * S->kw, pixels = (long long)batch * S->out_h * S->out_w;
  AGX_REQUIRE(k <= (1 << 24) && pixels <= 0x7FFFFFFF - 128, "agx_vae_conv2d: K = %lld or %lld output pixels: too many", k, pixels);
  ConvK a;
  a.x = x; a.w = w_packed; a.bias = bias; a.add = add; a.y = y;
  a.row_map = row_map; a.col_map = col_map;
  a.cin = S->cin; a.cout = S->cout; a.kh = S->kh; a.kw = S->kw; a.stride = S->stride; a.pad_h = S->pad_h; a.pad_w = S->pad_w;
  a.in_h = S->in_h; a.in_w = S->in_w; a.out_h = S->out_h; a.out_w = S->out_w; a.src_h = S->src_h; a.src_w = S->src_w;
  a.k8 = round_up8((int)k);
  a.pixels = (int)pixels;
  a.elu = (flags & AGX_VAE_ELU) ? 1 : 0;
  const int tiles = (a.pixels + 31) / 32;
  const int ct = vae_channel_tiles(a.cout, tiles);
  const dim3 grid((unsigned)((tiles + kWavesPerBlock - 1) / kWavesPerBlock), (unsigned)(a.cout / (32 * ct))), block(64 * kWavesPerBlock);
  if (ct == 4) hipLaunchKernelGGL(k_vae_conv<4>, grid, block, 0, (hipStream_t)stream, a);
  else if (ct == 2) hipLaunchKernelGGL(k_vae_conv<2>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(k_vae_conv<1>, grid, block, 0, (hipStream_t)stream, a);
  return check_launch("agx_vae_conv2d");
}

extern "C" int agx_vae_linear(int batch, const float *x, const float *w_packed, const float *bias, float *y, int in_features,
                              int out_features, int flags, void *stream) {
  AgxVaeConv S = {};
  S.cin = in_features; S.cout = out_features;
  S.kh = S.kw = S.stride = 1;
  S.in_h = S.in_w = S.out_h = S.out_w = S.src_h = S.src_w = 1;
  return agx_vae_conv2d(batch, x, w_packed, bias, nullptr, y, &S, flags, nullptr, nullptr, stream);
}

extern "C" int agx_vae_geometry(int image_h, int image_w, int32_t *out_hw) {
  AGX_REQUIRE(out_hw, "agx_vae_geometry: null buffer");
  AGX_REQUIRE(image_h > 0 && image_w > 0 && image_h <= 8192 && image_w <= 8192, "agx_vae_geometry: image_res = (%d, %d)", image_h, image_w);
  int hw[AGX_VAE_LAYERS][2] = {};
  const bool ok = geometry(image_h, image_w, hw);
  for (int l = 0; l < AGX_VAE_LAYERS; ++l) { out_hw[2 * l] = hw[l][0]; out_hw[2 * l + 1] = hw[l][1]; }
  AGX_REQUIRE(ok, "agx_vae_geometry: image_res = (%d, %d) ends in %d x %d x 128, dense0 needs 3 x 6 x 128 (the reference's (270, 480) does)",
              image_h, image_w, hw[8][0], hw[8][1]);
  return AGX_OK;
}

extern "C" int agx_vae_sample(int n, const float *z, const float *eps, float *latents, float *means, float *stdv, uint64_t rng_seed,
                              int env_index_base, int env_step, void *stream) {
  AGX_REQUIRE(n > 0 && n <= (1 << 24) && z && latents, "agx_vae_sample: bad arguments");
  hipLaunchKernelGGL(k_vae_sample, dim3(blocks_for(n * kLatent, 256)), dim3(256), 0, (hipStream_t)stream, n, z, eps, latents, means, stdv,
                     rng_seed, env_index_base, env_step);
  return check_launch("agx_vae_sample");
}

extern "C" int agx_vae_noise(int n, uint64_t rng_seed, int env_index_base, int env_step, float *noise_out, void *stream) {
  AGX_REQUIRE(n > 0 && n <= (1 << 24) && noise_out, "agx_vae_noise: bad arguments");
  hipLaunchKernelGGL(k_vae_noise, dim3(blocks_for(n * kLatent, 256)), dim3(256), 0, (hipStream_t)stream, n, rng_seed, env_index_base,
                     env_step, noise_out);
  return check_launch("agx_vae_noise");
}

extern "C" int agx_vae_place_latents(int n, const float *latents, float *obs, int obs_dim, int obs_offset, void *stream) {
  AGX_REQUIRE(n > 0 && n <= (1 << 24) && latents && obs && obs_offset >= 0 && obs_dim >= obs_offset + kLatent,
              "agx_vae_place_latents: bad arguments (obs_dim %d, offset %d)", obs_dim, obs_offset);
  hipLaunchKernelGGL(k_vae_place, dim3(blocks_for(n * kLatent, 256)), dim3(256), 0, (hipStream_t)stream, n, latents, obs, obs_dim, obs_offset);
  return check_launch("agx_vae_place_latents");
}

extern "C" int agx_vae_destroy(AgxVaeEncoder *enc) {
  if (!enc) return AGX_OK;
  for (int l = 0; l < AGX_VAE_LAYERS; ++l) {
    if (enc->w[l]) (void)hipFree(enc->w[l]);
    if (enc->b[l]) (void)hipFree(enc->b[l]);
  }
  delete enc;
  return AGX_OK;
}

namespace {
// the shape a layer's weights are packed under on the bf16 path: dense0 reads conv3_0's [3][6][128] output flattened
AgxVaeConv pack_shape_bf16(int l) {
  AgxVaeConv S = {};
  S.cin = kLayers[l].cin; S.cout = kLayers[l].cout; S.kh = S.kw = kLayers[l].k;
  if (l == 9) { S.cin = 128; S.kh = 3; S.kw = 6; }
  return S;
}
}  // namespace

extern "C" int agx_vae_create(const float *const *weights, const float *const *biases, int image_h, int image_w, int latent_dims,
                              AgxVaeEncoder **out) {
  return agx_vae_create_precision(weights, biases, image_h, image_w, latent_dims, AGX_VAE_FP32, out);
}

extern "C" int agx_vae_precision(const AgxVaeEncoder *enc) { return enc ? enc->precision : -1; }

extern "C" int agx_vae_create_precision(const float *const *weights, const float *const *biases, int image_h, int image_w, int latent_dims,
                                        int precision, AgxVaeEncoder **out) {
  AGX_REQUIRE(weights && biases && out, "agx_vae_create: null argument");
  *out = nullptr;
  AGX_REQUIRE(precision == AGX_VAE_FP32 || precision == AGX_VAE_BF16, "agx_vae_create_precision: precision = %d (AGX_VAE_FP32 or AGX_VAE_BF16)",
              precision);
  const bool bf16 = precision == AGX_VAE_BF16;
  AGX_REQUIRE(latent_dims == kLatent, "agx_vae_create: latent_dims = %d; this encoder (dense1: 512 -> 128) has 64", latent_dims);
  int32_t flat[2 * AGX_VAE_LAYERS];
  if (int e = agx_vae_geometry(image_h, image_w, flat)) return e;
  for (int l = 0; l < AGX_VAE_LAYERS; ++l) AGX_REQUIRE(weights[l] && biases[l], "agx_vae_create: layer %d: null weight or bias", l);
  AgxVaeEncoder *enc = new AgxVaeEncoder();
  enc->image_h = image_h; enc->image_w = image_w;
  enc->precision = precision;
  for (int l = 0; l < AGX_VAE_LAYERS; ++l) {
    enc->hw[l][0] = flat[2 * l]; enc->hw[l][1] = flat[2 * l + 1];
    enc->out_bytes[l] = (size_t)kLayers[l].cout * (size_t)enc->hw[l][0] * (size_t)enc->hw[l][1] * (bf16 && l != 10 ? sizeof(uint16_t) : sizeof(float));
    enc->w[l] = nullptr;
    enc->b[l] = nullptr;
  }
  for (int l = 0; l < AGX_VAE_LAYERS; ++l) {
    const LayerDef &L = kLayers[l];
    const int k = L.cin * L.k * L.k;
    std::vector<float> packed;
    std::vector<uint16_t> packed16;
    if (bf16) {
      const AgxVaeConv S = pack_shape_bf16(l);
      packed16.resize(agx_vae_packed_bf16_elems(&S));
      agx_vae_pack_weight_bf16(&S, weights[l], packed16.data());
    } else {
      packed.resize(agx_vae_packed_floats(L.cout, k));
      agx_vae_pack_weight(L.cout, k, weights[l], packed.data());
    }
    const void *src = bf16 ? (const void *)packed16.data() : (const void *)packed.data();
    const size_t bytes = bf16 ? packed16.size() * sizeof(uint16_t) : packed.size() * sizeof(float);
    hipError_t e = hipMalloc(&enc->w[l], bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&enc->b[l], (size_t)L.cout * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(enc->w[l], src, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(enc->b[l], biases[l], (size_t)L.cout * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      agx_vae_destroy(enc);
      return fail(AGX_E_LAUNCH, "agx_vae_create: layer %d: %s", l, hipGetErrorString(e));
    }
  }
  *out = enc;
  return AGX_OK;
}

namespace {
// byte offset of layer l's output inside a workspace laid out for `chunk` envs; l = AGX_VAE_LAYERS: the total.  A buffer holds
// `chunk` times the layer's bytes per env rounded up to 256, so every buffer is 256-byte aligned and the total is LINEAR in the
// chunk: a workspace of agx_vae_workspace_bytes(n) bytes runs exactly n envs per chunk.
size_t ws_offset(const AgxVaeEncoder *enc, int chunk, int l) {
  size_t off = 0;
  for (int j = 0; j < l; ++j) off += (size_t)chunk * align256(enc->out_bytes[j]);
  return off;
}
constexpr int kMaxChunk = 65536;
}  // namespace

extern "C" int agx_vae_envs_per_chunk(const AgxVaeEncoder *enc, size_t workspace_bytes, int num_envs) {
  if (!enc || num_envs <= 0) return 0;
  const size_t fit = workspace_bytes / ws_offset(enc, 1, AGX_VAE_LAYERS);
  const size_t cap = (size_t)(num_envs < kMaxChunk ? num_envs : kMaxChunk);
  return (int)(fit < cap ? fit : cap);
}

extern "C" size_t agx_vae_workspace_bytes(const AgxVaeEncoder *enc, int envs_per_chunk) {
  if (!enc || envs_per_chunk <= 0 || envs_per_chunk > 65536) return 0;
  return ws_offset(enc, envs_per_chunk, AGX_VAE_LAYERS);
}

extern "C" int agx_vae_layer_info(const AgxVaeEncoder *enc, int layer, int envs_per_chunk, const float **w_packed, const float **bias,
                                  size_t *out_offset_bytes) {
  AGX_REQUIRE(enc && layer >= 0 && layer < AGX_VAE_LAYERS && envs_per_chunk > 0 && envs_per_chunk <= 65536, "agx_vae_layer_info: bad arguments");
  if (w_packed) *w_packed = (const float *)enc->w[layer];
  if (bias) *bias = enc->b[layer];
  if (out_offset_bytes) *out_offset_bytes = ws_offset(enc, envs_per_chunk, layer);
  return AGX_OK;
}

namespace {
// agx_vae_encode on a bf16 handle: the same chunks and the same layer order, every layer one public bf16 call
int encode_bf16(AgxVaeEncoder *enc, int chunk, int num_envs, const float *pixels, int src_h, int src_w, const int32_t *row_map,
                const int32_t *col_map, const float *eps, float *latents, float *means, float *stdv, void *workspace, uint64_t rng_seed,
                int env_index_base, int env_step, void *stream) {
  void *out[AGX_VAE_LAYERS];
  for (int l = 0; l < AGX_VAE_LAYERS; ++l) out[l] = (char *)workspace + ws_offset(enc, chunk, l);
  for (int e0 = 0; e0 < num_envs; e0 += chunk) {
    const int c = num_envs - e0 < chunk ? num_envs - e0 : chunk;
    for (int o = 0; o < AGX_VAE_LAYERS; ++o) {
      const int l = kOrder[o];
      const LayerDef &L = kLayers[l];
      const void *x = L.input < 0 ? (const void *)(pixels + (size_t)e0 * (size_t)src_h * (size_t)src_w) : out[L.input];
      int flags = (l == 1 || l == 3 || l == 6 || l == 9) ? AGX_VAE_ELU : 0;
      const uint16_t *w = (const uint16_t *)enc->w[l];
      int e;
      if (l >= kConvLayers) {
        if (l == 10) flags |= AGX_VAE_OUT_F32;
        e = agx_vae_linear_bf16(c, (const uint16_t *)x, w, enc->b[l], out[l], L.cin, L.cout, flags, stream);
      } else {
        AgxVaeConv S;
        S.cin = L.cin; S.cout = L.cout; S.kh = S.kw = L.k; S.stride = L.stride; S.pad_h = L.pad_h; S.pad_w = L.pad_w;
        S.in_h = L.input < 0 ? enc->image_h : enc->hw[L.input][0];
        S.in_w = L.input < 0 ? enc->image_w : enc->hw[L.input][1];
        S.out_h = enc->hw[l][0]; S.out_w = enc->hw[l][1];
        S.src_h = L.input < 0 ? src_h : S.in_h;
        S.src_w = L.input < 0 ? src_w : S.in_w;
        if (L.input < 0) flags |= AGX_VAE_IN_IMAGE_F32;
        const uint16_t *add = (const uint16_t *)(l == 3 ? out[4] : (l == 6 ? out[7] : nullptr));
        e = agx_vae_conv2d_bf16(c, x, w, enc->b[l], add, out[l], &S, flags, L.input < 0 ? row_map : nullptr, L.input < 0 ? col_map : nullptr,
                                stream);
      }
      if (e) return e;
    }
    const size_t at = (size_t)e0 * kLatent;
    if (int e = agx_vae_sample(c, (const float *)out[10], eps ? eps + at : nullptr, latents + at, means ? means + at : nullptr,
                               stdv ? stdv + at : nullptr, rng_seed, env_index_base + e0, env_step, stream))
      return e;
  }
  return AGX_OK;
}
}  // namespace

extern "C" int agx_vae_encode(AgxVaeEncoder *enc, int num_envs, const float *pixels, int src_h, int src_w, const int32_t *row_map,
                              const int32_t *col_map, const float *eps, float *latents, float *means, float *stdv, void *workspace,
                              size_t workspace_bytes, uint64_t rng_seed, int env_index_base, int env_step, void *stream) {
  AGX_REQUIRE(enc && pixels && latents && workspace, "agx_vae_encode: null argument");
  AGX_REQUIRE(num_envs > 0 && num_envs <= (1 << 24) && src_h > 0 && src_w > 0, "agx_vae_encode: sizes out of range");
  AGX_REQUIRE(((uintptr_t)workspace & 255) == 0, "agx_vae_encode: the workspace must be 256-byte aligned");
  AGX_REQUIRE((row_map != nullptr) == (col_map != nullptr), "agx_vae_encode: row_map and col_map come together");
  AGX_REQUIRE(row_map || (src_h == enc->image_h && src_w == enc->image_w), "agx_vae_encode: a %d x %d image needs index tables to %d x %d",
              src_h, src_w, enc->image_h, enc->image_w);
  const int chunk = agx_vae_envs_per_chunk(enc, workspace_bytes, num_envs);  // the largest the workspace holds
  AGX_REQUIRE(chunk >= 1, "agx_vae_encode: workspace of %zu bytes, one env needs %zu", workspace_bytes, ws_offset(enc, 1, AGX_VAE_LAYERS));
  if (enc->precision == AGX_VAE_BF16)
    return encode_bf16(enc, chunk, num_envs, pixels, src_h, src_w, row_map, col_map, eps, latents, means, stdv, workspace, rng_seed, env_index_base,
                       env_step, stream);
  float *out[AGX_VAE_LAYERS];
  for (int l = 0; l < AGX_VAE_LAYERS; ++l) out[l] = (float *)((char *)workspace + ws_offset(enc, chunk, l));
  for (int e0 = 0; e0 < num_envs; e0 += chunk) {
    const int c = num_envs - e0 < chunk ? num_envs - e0 : chunk;
    for (int o = 0; o < AGX_VAE_LAYERS; ++o) {
      const int l = kOrder[o];
      const LayerDef &L = kLayers[l];
      const float *x = L.input < 0 ? pixels + (size_t)e0 * (size_t)src_h * (size_t)src_w : out[L.input];
      const int flags = (l == 1 || l == 3 || l == 6 || l == 9) ? AGX_VAE_ELU : 0;
      int e;
      if (l >= kConvLayers) {
        e = agx_vae_linear(c, x, (const float *)enc->w[l], enc->b[l], out[l], L.cin, L.cout, flags, stream);
      } else {
        AgxVaeConv S;
        S.cin = L.cin; S.cout = L.cout; S.kh = S.kw = L.k; S.stride = L.stride; S.pad_h = L.pad_h; S.pad_w = L.pad_w;
        S.in_h = L.input < 0 ? enc->image_h : enc->hw[L.input][0];
        S.in_w = L.input < 0 ? enc->image_w : enc->hw[L.input][1];
        S.out_h = enc->hw[l][0]; S.out_w = enc->hw[l][1];
        S.src_h = L.input < 0 ? src_h : S.in_h;
        S.src_w = L.input < 0 ? src_w : S.in_w;
        const float *add = l == 3 ? out[4] : (l == 6 ? out[7] : nullptr);
        e = agx_vae_conv2d(c, x, (const float *)enc->w[l], enc->b[l], add, out[l], &S, flags, L.input < 0 ? row_map : nullptr,
                           L.input < 0 ? col_map : nullptr, stream);
      }
      if (e) return e;
    }
    const size_t at = (size_t)e0 * kLatent;
    if (int e = agx_vae_sample(c, out[10], eps ? eps + at : nullptr, latents + at, means ? means + at : nullptr, stdv ? stdv + at : nullptr,
                               rng_seed, env_index_base + e0, env_step, stream))
      return e;
  }
  return AGX_OK;
}
