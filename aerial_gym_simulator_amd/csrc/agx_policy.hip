// Actor MLP of a trained policy (examples/rl_games_example/rl_games_inference.py:7-48 and what rl_games' player does around it:
// input normalisation, sampling, clamping) as ONE launch.  DESIGN.md "Policy actor".
//
// A workgroup of four waves owns a tile of 32 envs: the B column of v_mfma_f32_32x32x2_f32.  The activations of the tile live in
// LDS as [width][32] (env on the fast axis), ping-ponging between two buffers; they never go to memory.  Per layer the waves
// split the output channels in tiles of 32 (wave w: tiles w, w + 4, w + 8, w + 12); a wave runs the k loop of csrc/agx_vae.hip
// on its tiles: lane l supplies A = W[co = l & 31][k0 + (l >> 5)] from the packed [K8][Cout] weights and B = X[k0 + (l >> 5)][env =
// l & 31] from LDS, the hardware adds the two products in k order.  An output is therefore the fmaf chain k = 0, 1, 2, ... from 0,
// then + bias, then the activation -- the bits of agx_vae_linear applied layer by layer, whatever the batch, the env's place in
// it or the number of tiles a wave holds.  Weights stream from L2 four chunks of 8 k ahead of the instructions that use them.
#include "agx_common.h"
#include "agx_device_math.h"
#include "agx_rng.h"
#include "agx_task_parts.h"

#include <vector>

namespace {
using namespace agx;

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWaves = 4;
constexpr int kTile = 32;                                    // envs per workgroup
static_assert(AGX_POLICY_MAX_WIDTH / 32 <= 4 * kWaves, "a wave holds at most four channel tiles (layer_tiles<1 .. 4>)");
constexpr size_t kLdsLimit = 160 * 1024;
constexpr int kMaxEncoderLayers = AGX_POLICY_MAX_LAYERS - 2;
constexpr int kMaxMaps = kMaxEncoderLayers + 3;  // the recurrent actor's: the encoder's layers, then w_ih, w_hh and the head
static_assert(kMaxMaps == AGX_POLICY_MAX_LAYERS + 1, "the per-map arrays hold every layer either check admits");

struct PolicyK {
  const float *w[AGX_POLICY_MAX_LAYERS];  // packed [k8][cout]
  const float *b[AGX_POLICY_MAX_LAYERS];  // [cout]
  int k8[AGX_POLICY_MAX_LAYERS];          // rows of the packed weights = width of the layer's input in LDS
  int cout[AGX_POLICY_MAX_LAYERS];        // multiple of 32 (the last layer padded)
  int num_layers, in_dim, out_dim, activation;
  const float *obs, *eps, *logstd, *mean, *denom;
  float *actions, *mu_out;
  float clip;
  int n, flags, env_base, step;
  int buf1;  // first float of the second activation buffer
  uint64_t seed;
};

// normal j of env `genv` at env step `step`: the pairing of vae_normal (agx_vae.hip) under its own stream id
AGX_DEV float policy_normal(uint64_t seed, int genv, int step, int j) {
  const F4 f = rng_block(seed, genv, step, RNG_POLICY_EPS, j >> 2);
  const int e = j & 2;
  float z0, z1;
  normal_pair(e ? f.v[2] : f.v[0], e ? f.v[3] : f.v[1], z0, z1);
  return (j & 1) ? z1 : z0;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kRing = 5;          // chunks of 8 k a wave holds: one in use, kAhead in flight
constexpr int kAhead = kRing - 1;

template <int NT>
AGX_DEV void load_chunk(float (&dst)[4][NT], const float *__restrict__ wl, int k0, int cout) {
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int t = 0; t < NT; ++t) dst[u][t] = wl[(size_t)(k0 + 2 * u) * (size_t)cout + (size_t)(32 * kWaves * t)];
}

template <int NT>
AGX_DEV void mfma_chunk(f32x16 (&acc)[NT], const float (&wv)[4][NT], const float *__restrict__ xl, int k0) {
  float b[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) b[u] = xl[(k0 + 2 * u) * kTile];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[u][t], b[u], acc[t], 0, 0, 0);
}

// one layer for the NT channel tiles of this wave: tiles wave, wave + 4, ...
template <int NT>
AGX_DEV void layer_tiles(const float *__restrict__ w, const float *__restrict__ bias, const float *__restrict__ x, float *__restrict__ y,
                         int k8, int cout, int activation, int wave, int lane) {
  const int col = lane & 31, half = lane >> 5;
  const float *__restrict__ wl = w + (size_t)half * (size_t)cout + (size_t)(32 * wave + col);
  const float *__restrict__ xl = x + half * kTile + col;
  // result register i of lane l: channel (i & 3) + 8 (i >> 2) + 4 (l >> 5) of the 32, env l & 31.  The biases of a lane's sixteen
  // channels are four runs of four: fetched here, in front of the k loop, not one by one behind it
  f32x4 bv[NT][4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) bv[t][q] = *(const f32x4 *)(bias + 32 * (wave + kWaves * t) + 8 * q + 4 * half);
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
  // a ring of chunks of 8 k: kAhead in flight while one is used.  The main loop is one basic block (the ring index is a
  // compile-time constant in it), so the compiler counts the loads in flight instead of waiting for all of them.  A chunk past the
  // end re-reads the last one (in bounds).
  float ring[kRing][4][NT];
  const int chunks = k8 >> 3, last = k8 - 8;
#pragma unroll
  for (int s = 0; s < kAhead; ++s) load_chunk<NT>(ring[s], wl, min(8 * s, last), cout);
  int c = 0;
  for (; c + kRing <= chunks; c += kRing) {
#pragma unroll
    for (int s = 0; s < kRing; ++s) {
      load_chunk<NT>(ring[(s + kAhead) % kRing], wl, min(8 * (c + s + kAhead), last), cout);
      mfma_chunk<NT>(acc, ring[s], xl, 8 * (c + s));
    }
  }
#pragma unroll
  for (int s = 0; s < kRing - 1; ++s) {
    if (c + s < chunks) {
      if (c + s + kAhead < chunks) load_chunk<NT>(ring[(s + kAhead) % kRing], wl, 8 * (c + s + kAhead), cout);
      mfma_chunk<NT>(acc, ring[s], xl, 8 * (c + s));
    }
  }
  float v[NT][16];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) v[t][i] = acc[t][i] + bv[t][i >> 2][i & 3];
  if (activation == AGX_POLICY_ELU) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) v[t][i] = (v[t][i] > 0.0f) ? v[t][i] : expm1_cw(v[t][i]);
  } else if (activation == AGX_POLICY_RELU) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) v[t][i] = (v[t][i] < 0.0f) ? 0.0f : v[t][i];
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) y[(32 * (wave + kWaves * t) + (i & 3) + 8 * (i >> 2) + 4 * half) * kTile + col] = v[t][i];
}

__global__ void __launch_bounds__(64 * kWaves) k_policy_act(PolicyK a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long env0 = (long long)blockIdx.x * kTile;
  const int live = (int)min((long long)kTile, (long long)a.n - env0);  // envs of this tile, 1 .. 32
  // ---- the observations, transposed into [k8][32]; dead envs and the k padding are zero ----
  {
    float *__restrict__ x0 = lds;
    const float *__restrict__ src = a.obs + (size_t)env0 * (size_t)a.in_dim;
    const int k8 = a.k8[0];
    for (int i = tid; i < kTile * k8; i += 64 * kWaves) {
      // lanes run along the envs: LDS words in order (lanes along k would all hit one bank); the 32 rows a load instruction
      // touches are one contiguous piece of obs, and the next k reads the same cache lines
      const int k = i >> 5, col = i & 31;
      float v = 0.0f;
      if (col < live && k < a.in_dim) {
        v = src[(size_t)col * (size_t)a.in_dim + (size_t)k];
        if (a.mean) {
          v = (v - a.mean[k]) / a.denom[k];
          v = (v < -a.clip) ? -a.clip : ((v > a.clip) ? a.clip : v);
        }
      }
      x0[k * kTile + col] = v;
    }
  }
  __syncthreads();
  // ---- the layers ----
  for (int l = 0; l < a.num_layers; ++l) {
    const float *__restrict__ x = lds + ((l & 1) ? a.buf1 : 0);
    float *__restrict__ y = lds + ((l & 1) ? 0 : a.buf1);
    const int cout = a.cout[l], tiles = cout >> 5;
    const int nt = wave < tiles ? (tiles - wave + kWaves - 1) / kWaves : 0;  // wave-uniform
    const int act = (l + 1 < a.num_layers) ? a.activation : AGX_POLICY_NONE;
    if (nt == 1) layer_tiles<1>(a.w[l], a.b[l], x, y, a.k8[l], cout, act, wave, lane);
    else if (nt == 2) layer_tiles<2>(a.w[l], a.b[l], x, y, a.k8[l], cout, act, wave, lane);
    else if (nt == 3) layer_tiles<3>(a.w[l], a.b[l], x, y, a.k8[l], cout, act, wave, lane);
    else if (nt == 4) layer_tiles<4>(a.w[l], a.b[l], x, y, a.k8[l], cout, act, wave, lane);
    __syncthreads();
  }
  // ---- mean -> (sample) -> (clamp) -> [N][out], rows of the tile contiguous ----
  const float *__restrict__ mu_t = lds + ((a.num_layers & 1) ? a.buf1 : 0);
  const size_t out0 = (size_t)env0 * (size_t)a.out_dim;
  for (int i = tid; i < live * a.out_dim; i += 64 * kWaves) {
    const int col = i / a.out_dim, j = i - col * a.out_dim;
    const float mu = mu_t[j * kTile + col];
    float v = mu;
    if (a.flags & AGX_POLICY_SAMPLE) {
      const float sigma = exp_cw(a.logstd[j]);
      const float e = a.eps ? a.eps[out0 + i] : policy_normal(a.seed, a.env_base + (int)env0 + col, a.step, j);
      const float t = e * sigma;
      v = mu + t;
    }
    if (a.flags & AGX_POLICY_CLAMP) v = (v < -1.0f) ? -1.0f : ((v > 1.0f) ? 1.0f : v);
    a.actions[out0 + i] = v;
    if (a.mu_out) a.mu_out[out0 + i] = mu;
  }
}

__global__ void k_policy_noise(int n, int out_dim, uint64_t seed, int env_base, int step, float *__restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n * out_dim) return;
  const int env = (int)(i / out_dim);
  out[i] = policy_normal(seed, env_base + env, step, (int)(i - (long long)env * out_dim));
}

// ---- recurrent actor: encoder MLP -> GRU cell -> linear head as ONE launch ----------------------------------------------------
// sample-factory's actor with a recurrent core (sf_inference_class.py:80-101, nn_inference_class.py:77-101).  The mapping of
// k_policy_act: a workgroup of four waves owns 32 envs, every linear map is layer_tiles.  LDS, in floats per env column:
//   [buf0 | buf1]  the encoder's ping-pong pair (activation a lives in buffer a & 1; the encoder's output is the cell's input x)
//   [h]            H: the state of the tile, h' in place after the gates
//   [gi | gh]      3H each: W_ih x + b_ih and W_hh h + b_hh, gate order r, z, n; afterwards the head's output (<= 128 <= 6H rows)
// Nothing crosses workgroups: a tile reads its rows of the state buffer before the gates and writes them after.
// The observation loop, the sampling epilogue and the layer dispatch are stated here a second time on purpose: one workgroup's chain
// of layers is the call's latency, and any change to this kernel's text reschedules it.  Shared device functions cost k_recurrent_act
// 0.15 to 0.37 us per call (sharing the observation loop alone: 0.16 to 0.28), and k_policy_act through run_layer needs 208 VGPRs
// instead of 178 (profiles/policy_refactor_codegen.md, profiles/policy_refactor_ab.json).
struct RecurrentK {
  const float *w[kMaxMaps];  // encoder layers 0 .. L-1, then w_ih, w_hh, head: packed [k8][cout]
  const float *b[kMaxMaps];
  int k8[kMaxMaps];
  int cout[kMaxMaps];
  int num_encoder_layers, in_dim, hidden, num_actions, adaptive, activation;
  const float *obs, *eps, *logstd, *mean, *denom;
  const uint8_t *done0, *done1;
  float *state, *actions, *mu_out, *logstd_out;
  float clip;
  int n, flags, env_base, step;
  int buf1, off_h, off_gi;  // first float of the second ping-pong buffer, of h, of gi (gh follows gi)
  uint64_t seed;
};

AGX_DEV void run_layer(const float *__restrict__ w, const float *__restrict__ bias, const float *__restrict__ x, float *__restrict__ y, int k8,
                       int cout, int act, int wave, int lane) {
  const int tiles = cout >> 5;
  const int nt = wave < tiles ? (tiles - wave + kWaves - 1) / kWaves : 0;  // wave-uniform, <= 4 (the check: cout <= 512)
  if (nt == 1) layer_tiles<1>(w, bias, x, y, k8, cout, act, wave, lane);
  else if (nt == 2) layer_tiles<2>(w, bias, x, y, k8, cout, act, wave, lane);
  else if (nt == 3) layer_tiles<3>(w, bias, x, y, k8, cout, act, wave, lane);
  else if (nt == 4) layer_tiles<4>(w, bias, x, y, k8, cout, act, wave, lane);
}

__global__ void __launch_bounds__(64 * kWaves) k_recurrent_act(RecurrentK a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long env0 = (long long)blockIdx.x * kTile;
  const int live = (int)min((long long)kTile, (long long)a.n - env0);  // envs of this tile, 1 .. 32
  const int L = a.num_encoder_layers, H = a.hidden;
  const bool after = (a.flags & AGX_POLICY_RESET_AFTER) != 0;
  float *__restrict__ hl = lds + a.off_h;
  // ---- the observations as in k_policy_act, and the state of the tile: [H][32], dead envs and flagged ones (reset before) zero ----
  {
    float *__restrict__ x0 = lds;
    const float *__restrict__ src = a.obs + (size_t)env0 * (size_t)a.in_dim;
    const int k8 = a.k8[0];
    for (int i = tid; i < kTile * k8; i += 64 * kWaves) {
      const int k = i >> 5, col = i & 31;
      float v = 0.0f;
      if (col < live && k < a.in_dim) {
        v = src[(size_t)col * (size_t)a.in_dim + (size_t)k];
        if (a.mean) {
          v = (v - a.mean[k]) / a.denom[k];
          v = (v < -a.clip) ? -a.clip : ((v > a.clip) ? a.clip : v);
        }
      }
      x0[k * kTile + col] = v;
    }
    // lanes along the envs, like the observations: LDS words in order.  In memory neighbouring lanes are a row of H floats apart,
    // so an instruction touches 32 cache lines -- which the following values of j read again out of L2.  The state is
    // H x 128 bytes per tile against a kernel bound by its matrix chain; the store after the gates mirrors it
    const float *__restrict__ hs = a.state + (size_t)env0 * (size_t)H;
    for (int i = tid; i < kTile * H; i += 64 * kWaves) {
      const int j = i >> 5, col = i & 31;
      float v = 0.0f;
      if (col < live) {
        bool flagged = false;
        if (!after) flagged = (a.done0 && a.done0[env0 + col]) || (a.done1 && a.done1[env0 + col]);
        if (!flagged) v = hs[(size_t)col * (size_t)H + (size_t)j];
      }
      hl[j * kTile + col] = v;
    }
  }
  __syncthreads();
  // ---- the encoder: the activation follows every layer ----
  for (int l = 0; l < L; ++l) {
    const float *__restrict__ x = lds + ((l & 1) ? a.buf1 : 0);
    float *__restrict__ y = lds + ((l & 1) ? 0 : a.buf1);
    run_layer(a.w[l], a.b[l], x, y, a.k8[l], a.cout[l], a.activation, wave, lane);
    __syncthreads();
  }
  // ---- the cell ----
  const float *__restrict__ xe = lds + ((L & 1) ? a.buf1 : 0);
  float *__restrict__ gi = lds + a.off_gi;
  float *__restrict__ gh = gi + 3 * H * kTile;
  run_layer(a.w[L], a.b[L], xe, gi, a.k8[L], a.cout[L], AGX_POLICY_NONE, wave, lane);
  run_layer(a.w[L + 1], a.b[L + 1], hl, gh, a.k8[L + 1], a.cout[L + 1], AGX_POLICY_NONE, wave, lane);
  __syncthreads();
  {
    float *__restrict__ hs = a.state + (size_t)env0 * (size_t)H;
    for (int i = tid; i < kTile * H; i += 64 * kWaves) {
      const int j = i >> 5, col = i & 31;
      const float sr = gi[j * kTile + col] + gh[j * kTile + col];
      const float r = sigmoid_cw(sr);
      const float sz = gi[(H + j) * kTile + col] + gh[(H + j) * kTile + col];
      const float z = sigmoid_cw(sz);
      const float t = r * gh[(2 * H + j) * kTile + col];
      const float u = gi[(2 * H + j) * kTile + col] + t;
      const float nn = tanh_cw(u);
      const float omz = 1.0f - z;
      const float b = omz * nn;
      const float c = z * hl[j * kTile + col];
      const float hn = b + c;
      hl[j * kTile + col] = hn;  // this thread's own element: in place
      if (col < live) {
        bool flagged = false;
        if (after) flagged = (a.done0 && a.done0[env0 + col]) || (a.done1 && a.done1[env0 + col]);
        hs[(size_t)col * (size_t)H + (size_t)j] = flagged ? 0.0f : hn;
      }
    }
  }
  __syncthreads();
  // ---- the head: H -> P rows padded to 32, written over gi (and into gh: both are dead) ----
  float *po = gi;
  run_layer(a.w[L + 2], a.b[L + 2], hl, po, a.k8[L + 2], a.cout[L + 2], AGX_POLICY_NONE, wave, lane);
  __syncthreads();
  // ---- mean -> (sample) -> (clamp) -> [N][A] ----
  const int A = a.num_actions;
  const size_t out0 = (size_t)env0 * (size_t)A;
  for (int i = tid; i < live * A; i += 64 * kWaves) {
    const int col = i / A, j = i - col * A;
    const float mu = po[j * kTile + col];
    const bool have_ls = a.adaptive || a.logstd;
    const float ls = a.adaptive ? po[(A + j) * kTile + col] : (a.logstd ? a.logstd[j] : 0.0f);
    float v = mu;
    if (a.flags & AGX_POLICY_SAMPLE) {
      const float sigma = exp_cw(ls);
      const float e = a.eps ? a.eps[out0 + i] : policy_normal(a.seed, a.env_base + (int)env0 + col, a.step, j);
      const float t = e * sigma;
      v = mu + t;
    }
    if (a.flags & AGX_POLICY_CLAMP) v = (v < -1.0f) ? -1.0f : ((v > 1.0f) ? 1.0f : v);
    a.actions[out0 + i] = v;
    if (a.mu_out) a.mu_out[out0 + i] = mu;
    if (a.logstd_out && have_ls) a.logstd_out[out0 + i] = ls;
  }
}

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// ---- the host side both actors share.  `entry` is the name of the C entry a message begins with ---------------------------------
struct ActorCommon {
  float *w[kMaxMaps], *b[kMaxMaps];  // device; a null entry is a map the actor does not have
  int k8[kMaxMaps], cout[kMaxMaps];
  float *mean, *denom, *logstd;  // device, allocated by create; in use once set
  bool has_norm, has_logstd;
  float clip;
  int in_dim, num_actions;
  int buf1;
  size_t lds_bytes;
};

// floats per env column of the two ping-pong buffers: activation a (0 = the input, padded to 8, .. count = the last map's output,
// padded to 32 when pad_last) lives in buffer a & 1.  The one statement of that rule
void pingpong_widths(int count, const int32_t *dims, bool pad_last, int width[2]) {
  width[0] = width[1] = 0;
  for (int a = 0; a <= count; ++a) {
    const int wa = a == 0 ? round_up(dims[0], 8) : (a == count && pad_last ? round_up(dims[a], 32) : dims[a]);
    if (wa > width[a & 1]) width[a & 1] = wa;
  }
}

// map l = torch's w [co][k] and b [co]: the rows padded to a multiple of 32 with zero weights and zero biases (padding the caller
// never sees; hidden widths are multiples of 32 already), packed [k8][cout], on the device
hipError_t upload_map(ActorCommon &c, int l, int co, int k, const float *w, const float *b) {
  const int cop = round_up(co, 32);
  c.k8[l] = round_up(k, 8);
  c.cout[l] = cop;
  std::vector<float> padded((size_t)cop * k, 0.0f), bias((size_t)cop, 0.0f);
  for (size_t i = 0; i < (size_t)co * k; ++i) padded[i] = w[i];
  for (int i = 0; i < co; ++i) bias[i] = b[i];
  std::vector<float> packed(agx_vae_packed_floats(cop, k));
  agx_vae_pack_weight(cop, k, padded.data(), packed.data());
  hipError_t e = hipMalloc((void **)&c.w[l], packed.size() * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void **)&c.b[l], bias.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(c.w[l], packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(c.b[l], bias.data(), bias.size() * sizeof(float), hipMemcpyHostToDevice);
  return e;
}

// what a create does once its maps are up: the normaliser's and the log-std's buffers, and the kernel's dynamic-LDS attribute
hipError_t finish_create(ActorCommon &c, const void *kernel) {
  hipError_t e = hipMalloc((void **)&c.mean, (size_t)c.in_dim * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void **)&c.denom, (size_t)c.in_dim * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void **)&c.logstd, (size_t)c.num_actions * sizeof(float));
  // above 64 KiB of dynamic LDS the runtime may want to be told; a runtime that refuses the attribute refuses the launch too, and
  // says so there.  The attribute belongs to the kernel, not to this actor: always the limit the checks admit, so that a smaller
  // actor created later does not lower it under an earlier one
  if (e == hipSuccess) {
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit);
    (void)hipGetLastError();
  }
  return e;
}

void free_actor(ActorCommon &c) {
  for (int l = 0; l < kMaxMaps; ++l) {
    if (c.w[l]) (void)hipFree(c.w[l]);
    if (c.b[l]) (void)hipFree(c.b[l]);
  }
  if (c.mean) (void)hipFree(c.mean);
  if (c.denom) (void)hipFree(c.denom);
  if (c.logstd) (void)hipFree(c.logstd);
}

int set_input_norm(const char *entry, ActorCommon &c, const float *mean, const float *denom, float clip) {
  if (!mean && !denom) { c.has_norm = false; return AGX_OK; }
  AGX_REQUIRE(mean && denom, "%s: mean and denom come together", entry);
  AGX_REQUIRE(clip > 0.0f, "%s: clip = %g must be positive", entry, (double)clip);
  hipError_t e = hipMemcpy(c.mean, mean, (size_t)c.in_dim * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(c.denom, denom, (size_t)c.in_dim * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(AGX_E_LAUNCH, "%s: %s", entry, hipGetErrorString(e));
  c.clip = clip;
  c.has_norm = true;
  return AGX_OK;
}

int set_logstd(const char *entry, ActorCommon &c, const float *logstd) {
  if (!logstd) { c.has_logstd = false; return AGX_OK; }
  hipError_t e = hipMemcpy(c.logstd, logstd, (size_t)c.num_actions * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(AGX_E_LAUNCH, "%s: %s", entry, hipGetErrorString(e));
  c.has_logstd = true;
  return AGX_OK;
}

int launch_noise(const char *entry, const ActorCommon *c, int num_envs, uint64_t rng_seed, int env_index_base, int env_step, float *noise_out,
                 void *stream) {
  AGX_REQUIRE(c && noise_out, "%s: null argument", entry);
  AGX_REQUIRE(num_envs > 0 && num_envs <= (1 << 22), "%s: num_envs = %d, supported: 1 .. %d", entry, num_envs, 1 << 22);
  const long long total = (long long)num_envs * c->num_actions;
  hipLaunchKernelGGL(k_policy_noise, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, num_envs, c->num_actions, rng_seed,
                     env_index_base, env_step, noise_out);
  return check_launch(entry);
}

// the fields PolicyK and RecurrentK have in common
template <class K>
void fill_common(K &a, const ActorCommon &c, int num_envs, const float *obs, float *actions, float *mu_out, const float *eps, int flags,
                 uint64_t rng_seed, int env_index_base, int env_step) {
  for (size_t l = 0; l < sizeof(a.w) / sizeof(a.w[0]); ++l) { a.w[l] = c.w[l]; a.b[l] = c.b[l]; a.k8[l] = c.k8[l]; a.cout[l] = c.cout[l]; }
  a.in_dim = c.in_dim;
  a.obs = obs; a.eps = eps; a.logstd = c.has_logstd ? c.logstd : nullptr;
  a.mean = c.has_norm ? c.mean : nullptr; a.denom = c.has_norm ? c.denom : nullptr;
  a.actions = actions; a.mu_out = mu_out;
  a.clip = c.clip;
  a.n = num_envs; a.flags = flags; a.env_base = env_index_base; a.step = env_step;
  a.buf1 = c.buf1;
  a.seed = rng_seed;
}
}  // namespace

struct AgxPolicy {
  ActorCommon c;
  int num_layers, activation;
};

struct AgxRecurrent {
  ActorCommon c;
  int num_encoder_layers, activation, hidden, adaptive;
  int off_h, off_gi;
};

extern "C" int agx_policy_destroy(AgxPolicy *p) {
  if (!p) return AGX_OK;
  free_actor(p->c);
  delete p;
  return AGX_OK;
}

extern "C" int agx_policy_check(int num_layers, const int32_t *dims, size_t *lds_bytes) {
  AGX_REQUIRE(dims, "agx_policy_create: null dims");
  AGX_REQUIRE(num_layers >= 1 && num_layers <= AGX_POLICY_MAX_LAYERS, "agx_policy_create: num_layers = %d, supported: 1 .. %d", num_layers,
              AGX_POLICY_MAX_LAYERS);
  AGX_REQUIRE(dims[0] >= 1 && dims[0] <= AGX_POLICY_MAX_WIDTH, "agx_policy_create: input width %d, supported: 1 .. %d", dims[0],
              AGX_POLICY_MAX_WIDTH);
  for (int l = 1; l < num_layers; ++l)
    AGX_REQUIRE(dims[l] >= 32 && dims[l] <= AGX_POLICY_MAX_WIDTH && dims[l] % 32 == 0,
                "agx_policy_create: hidden width %d (output of layer %d): a multiple of 32 up to %d is supported", dims[l], l - 1,
                AGX_POLICY_MAX_WIDTH);
  AGX_REQUIRE(dims[num_layers] >= 1 && dims[num_layers] <= AGX_POLICY_MAX_WIDTH, "agx_policy_create: output width %d, supported: 1 .. %d",
              dims[num_layers], AGX_POLICY_MAX_WIDTH);
  int width[2];
  pingpong_widths(num_layers, dims, true, width);  // activation num_layers is the mean
  const size_t bytes = (size_t)(width[0] + width[1]) * kTile * sizeof(float);
  AGX_REQUIRE(bytes <= kLdsLimit, "agx_policy_create: activations of widths %d + %d for 32 envs need %zu bytes of LDS, a workgroup has %zu",
              width[0], width[1], bytes, kLdsLimit);
  if (lds_bytes) *lds_bytes = bytes;
  return AGX_OK;
}

extern "C" int agx_policy_create(int num_layers, const int32_t *dims, const float *const *weights, const float *const *biases,
                                 int hidden_activation, AgxPolicy **out) {
  AGX_REQUIRE(out, "agx_policy_create: null handle pointer");
  *out = nullptr;
  AGX_REQUIRE(dims && weights && biases, "agx_policy_create: null argument");
  size_t lds_bytes = 0;
  if (int e = agx_policy_check(num_layers, dims, &lds_bytes)) return e;
  AGX_REQUIRE(hidden_activation == AGX_POLICY_NONE || hidden_activation == AGX_POLICY_ELU || hidden_activation == AGX_POLICY_RELU,
              "agx_policy_create: hidden_activation = %d (AGX_POLICY_NONE, _ELU or _RELU)", hidden_activation);
  for (int l = 0; l < num_layers; ++l) AGX_REQUIRE(weights[l] && biases[l], "agx_policy_create: layer %d: null weight or bias", l);
  AgxPolicy *p = new AgxPolicy();  // zeros and null pointers
  p->num_layers = num_layers;
  p->activation = hidden_activation;
  p->c.in_dim = dims[0];
  p->c.num_actions = dims[num_layers];
  p->c.lds_bytes = lds_bytes;
  int width[2];
  pingpong_widths(num_layers, dims, true, width);
  p->c.buf1 = width[0] * kTile;
  hipError_t e = hipSuccess;
  for (int l = 0; l < num_layers && e == hipSuccess; ++l) e = upload_map(p->c, l, dims[l + 1], dims[l], weights[l], biases[l]);
  if (e == hipSuccess) e = finish_create(p->c, (const void *)k_policy_act);
  if (e != hipSuccess) {
    agx_policy_destroy(p);
    (void)hipGetLastError();
    return fail(AGX_E_LAUNCH, "agx_policy_create: %s", hipGetErrorString(e));
  }
  *out = p;
  return AGX_OK;
}

extern "C" int agx_policy_set_input_norm(AgxPolicy *p, const float *mean, const float *denom, float clip) {
  AGX_REQUIRE(p, "agx_policy_set_input_norm: null handle");
  return set_input_norm("agx_policy_set_input_norm", p->c, mean, denom, clip);
}

extern "C" int agx_policy_set_logstd(AgxPolicy *p, const float *logstd) {
  AGX_REQUIRE(p, "agx_policy_set_logstd: null handle");
  return set_logstd("agx_policy_set_logstd", p->c, logstd);
}

extern "C" int agx_policy_act(AgxPolicy *p, int num_envs, const float *obs, float *actions, float *mu_out, const float *eps, int flags,
                              uint64_t rng_seed, int env_index_base, int env_step, void *stream) {
  AGX_REQUIRE(p, "agx_policy_act: null handle");
  AGX_REQUIRE(num_envs >= 0 && num_envs <= (1 << 22), "agx_policy_act: num_envs = %d, supported: 0 .. %d", num_envs, 1 << 22);
  AGX_REQUIRE((flags & ~(AGX_POLICY_SAMPLE | AGX_POLICY_CLAMP)) == 0, "agx_policy_act: flags = %d", flags);
  AGX_REQUIRE(!(flags & AGX_POLICY_SAMPLE) || p->c.has_logstd, "agx_policy_act: AGX_POLICY_SAMPLE needs a logstd (agx_policy_set_logstd)");
  if (num_envs == 0) return AGX_OK;
  AGX_REQUIRE(obs, "agx_policy_act: null obs");
  AGX_REQUIRE(actions, "agx_policy_act: null actions");
  PolicyK a;
  fill_common(a, p->c, num_envs, obs, actions, mu_out, eps, flags, rng_seed, env_index_base, env_step);
  a.num_layers = p->num_layers; a.out_dim = p->c.num_actions; a.activation = p->activation;
  hipLaunchKernelGGL(k_policy_act, dim3((unsigned)((num_envs + kTile - 1) / kTile)), dim3(64 * kWaves), p->c.lds_bytes, (hipStream_t)stream, a);
  return check_launch("agx_policy_act");
}

extern "C" int agx_policy_noise(const AgxPolicy *p, int num_envs, uint64_t rng_seed, int env_index_base, int env_step, float *noise_out,
                                void *stream) {
  return launch_noise("agx_policy_noise", p ? &p->c : nullptr, num_envs, rng_seed, env_index_base, env_step, noise_out, stream);
}

extern "C" int agx_recurrent_destroy(AgxRecurrent *p) {
  if (!p) return AGX_OK;
  free_actor(p->c);
  delete p;
  return AGX_OK;
}

extern "C" int agx_recurrent_check(int num_encoder_layers, const int32_t *dims, int hidden, int head_out, size_t *lds_bytes) {
  const int L = num_encoder_layers;
  AGX_REQUIRE(dims, "agx_recurrent_create: null dims");
  AGX_REQUIRE(L >= 1 && L <= kMaxEncoderLayers, "agx_recurrent_create: num_encoder_layers = %d, supported: 1 .. %d", L, kMaxEncoderLayers);
  AGX_REQUIRE(dims[0] >= 1 && dims[0] <= AGX_POLICY_MAX_WIDTH, "agx_recurrent_create: input width %d, supported: 1 .. %d", dims[0],
              AGX_POLICY_MAX_WIDTH);
  for (int l = 1; l <= L; ++l)
    AGX_REQUIRE(dims[l] >= 32 && dims[l] <= AGX_POLICY_MAX_WIDTH && dims[l] % 32 == 0,
                "agx_recurrent_create: encoder width %d (output of layer %d): a multiple of 32 up to %d is supported", dims[l], l - 1,
                AGX_POLICY_MAX_WIDTH);
  AGX_REQUIRE(hidden >= 32 && hidden <= AGX_POLICY_MAX_WIDTH && hidden % 32 == 0,
              "agx_recurrent_create: hidden size %d: a multiple of 32 within 32 .. %d is supported", hidden, AGX_POLICY_MAX_WIDTH);
  AGX_REQUIRE(head_out >= 1 && head_out <= 128, "agx_recurrent_create: head width %d, supported: 1 .. 128 (64 actions, means and log-std)",
              head_out);
  int width[2];
  pingpong_widths(L, dims, false, width);  // activation L is the cell's input
  // x (the ping-pong pair), h, gi and gh are live together in the cell
  const size_t bytes = (size_t)(width[0] + width[1] + 7 * hidden) * kTile * sizeof(float);
  AGX_REQUIRE(bytes <= kLdsLimit,
              "agx_recurrent_create: encoder activations of widths %d + %d and the cell's 7 x %d (h, gi, gh) for 32 envs need %zu bytes of "
              "LDS, a workgroup has %zu", width[0], width[1], hidden, bytes, kLdsLimit);
  // 3 x hidden channels are at most sixteen tiles of 32, four per wave: implied by the LDS limit (7 x 192 x 128 bytes exceed it)
  AGX_REQUIRE(3 * hidden <= 32 * 4 * kWaves, "agx_recurrent_create: hidden size %d: 3 x hidden exceeds %d gate channels", hidden, 32 * 4 * kWaves);
  if (lds_bytes) *lds_bytes = bytes;
  return AGX_OK;
}

extern "C" int agx_recurrent_create(int num_encoder_layers, const int32_t *dims, int hidden, int num_actions, int adaptive_stddev,
                                    const float *const *enc_weights, const float *const *enc_biases, const float *w_ih, const float *w_hh,
                                    const float *b_ih, const float *b_hh, const float *head_weight, const float *head_bias,
                                    int hidden_activation, AgxRecurrent **out) {
  AGX_REQUIRE(out, "agx_recurrent_create: null handle pointer");
  *out = nullptr;
  AGX_REQUIRE(dims && enc_weights && enc_biases && w_ih && w_hh && b_ih && b_hh && head_weight && head_bias, "agx_recurrent_create: null argument");
  AGX_REQUIRE(num_actions >= 1 && num_actions <= 64, "agx_recurrent_create: num_actions = %d, supported: 1 .. 64", num_actions);
  const int L = num_encoder_layers, H = hidden, P = adaptive_stddev ? 2 * num_actions : num_actions;
  size_t lds_bytes = 0;
  if (int e = agx_recurrent_check(L, dims, H, P, &lds_bytes)) return e;
  AGX_REQUIRE(hidden_activation == AGX_POLICY_ELU || hidden_activation == AGX_POLICY_RELU,
              "agx_recurrent_create: hidden_activation = %d (AGX_POLICY_ELU or _RELU)", hidden_activation);
  for (int l = 0; l < L; ++l) AGX_REQUIRE(enc_weights[l] && enc_biases[l], "agx_recurrent_create: encoder layer %d: null weight or bias", l);
  AgxRecurrent *p = new AgxRecurrent();  // zeros and null pointers
  p->num_encoder_layers = L; p->activation = hidden_activation; p->hidden = H; p->adaptive = adaptive_stddev ? 1 : 0;
  p->c.in_dim = dims[0];
  p->c.num_actions = num_actions;
  p->c.lds_bytes = lds_bytes;
  int width[2];
  pingpong_widths(L, dims, false, width);
  p->c.buf1 = width[0] * kTile;
  p->off_h = (width[0] + width[1]) * kTile;
  p->off_gi = p->off_h + H * kTile;
  hipError_t e = hipSuccess;
  static_assert(kMaxEncoderLayers + 3 <= kMaxMaps, "map L + 2 (the head) is the last entry");
  for (int l = 0; l < L && e == hipSuccess; ++l) e = upload_map(p->c, l, dims[l + 1], dims[l], enc_weights[l], enc_biases[l]);
  if (e == hipSuccess) e = upload_map(p->c, L, 3 * H, dims[L], w_ih, b_ih);
  if (e == hipSuccess) e = upload_map(p->c, L + 1, 3 * H, H, w_hh, b_hh);
  if (e == hipSuccess) e = upload_map(p->c, L + 2, P, H, head_weight, head_bias);
  if (e == hipSuccess) e = finish_create(p->c, (const void *)k_recurrent_act);
  if (e != hipSuccess) {
    agx_recurrent_destroy(p);
    (void)hipGetLastError();
    return fail(AGX_E_LAUNCH, "agx_recurrent_create: %s", hipGetErrorString(e));
  }
  *out = p;
  return AGX_OK;
}

extern "C" int agx_recurrent_set_input_norm(AgxRecurrent *p, const float *mean, const float *denom, float clip) {
  AGX_REQUIRE(p, "agx_recurrent_set_input_norm: null handle");
  return set_input_norm("agx_recurrent_set_input_norm", p->c, mean, denom, clip);
}

extern "C" int agx_recurrent_set_logstd(AgxRecurrent *p, const float *logstd) {
  AGX_REQUIRE(p, "agx_recurrent_set_logstd: null handle");
  AGX_REQUIRE(!p->adaptive, "agx_recurrent_set_logstd: the head is adaptive: it emits the log-std itself");
  return set_logstd("agx_recurrent_set_logstd", p->c, logstd);
}

extern "C" int agx_recurrent_act(AgxRecurrent *p, int num_envs, const float *obs, float *hidden, const uint8_t *done0, const uint8_t *done1,
                                 float *actions, float *mu_out, float *logstd_out, const float *eps, int flags, uint64_t rng_seed,
                                 int env_index_base, int env_step, void *stream) {
  AGX_REQUIRE(p, "agx_recurrent_act: null handle");
  AGX_REQUIRE(num_envs >= 0 && num_envs <= (1 << 22), "agx_recurrent_act: num_envs = %d, supported: 0 .. %d", num_envs, 1 << 22);
  AGX_REQUIRE((flags & ~(AGX_POLICY_SAMPLE | AGX_POLICY_CLAMP | AGX_POLICY_RESET_AFTER)) == 0, "agx_recurrent_act: flags = %d", flags);
  const bool have_logstd = p->adaptive || p->c.has_logstd;
  AGX_REQUIRE(!(flags & AGX_POLICY_SAMPLE) || have_logstd,
              "agx_recurrent_act: AGX_POLICY_SAMPLE needs a logstd (an adaptive head or agx_recurrent_set_logstd)");
  AGX_REQUIRE(!logstd_out || have_logstd, "agx_recurrent_act: logstd_out needs a logstd (an adaptive head or agx_recurrent_set_logstd)");
  if (num_envs == 0) return AGX_OK;
  AGX_REQUIRE(obs, "agx_recurrent_act: null obs");
  AGX_REQUIRE(hidden, "agx_recurrent_act: null hidden");
  AGX_REQUIRE(actions, "agx_recurrent_act: null actions");
  RecurrentK a;
  fill_common(a, p->c, num_envs, obs, actions, mu_out, eps, flags, rng_seed, env_index_base, env_step);
  a.num_encoder_layers = p->num_encoder_layers; a.hidden = p->hidden; a.num_actions = p->c.num_actions;
  a.adaptive = p->adaptive; a.activation = p->activation;
  a.done0 = done0; a.done1 = done1;
  a.state = hidden; a.logstd_out = logstd_out;
  a.off_h = p->off_h; a.off_gi = p->off_gi;
  hipLaunchKernelGGL(k_recurrent_act, dim3((unsigned)((num_envs + kTile - 1) / kTile)), dim3(64 * kWaves), p->c.lds_bytes, (hipStream_t)stream, a);
  return check_launch("agx_recurrent_act");
}

extern "C" int agx_recurrent_noise(const AgxRecurrent *p, int num_envs, uint64_t rng_seed, int env_index_base, int env_step, float *noise_out,
                                   void *stream) {
  return launch_noise("agx_recurrent_noise", p ? &p->c : nullptr, num_envs, rng_seed, env_index_base, env_step, noise_out, stream);
}
