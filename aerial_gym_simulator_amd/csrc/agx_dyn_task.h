#pragma once
// Task code: the position / navigation rewards and the navigation bookkeeping as device functions (the fused env steps run them as
// their epilogue), the observation writers, and the stand-alone reward and observation kernels with their entry points.
// Part of the one translation unit agx_dynamics.hip, which alone includes it (after the AGX_DYN_* switches and agx_task_parts.h).

namespace agx {
// position_setpoint_task.py:245-282 on registers; returns the reward, ORs the distance crash
AGX_DEV float reward_position(const EnvState &s, Q4 qveh, V3 wb, V3 tgt, bool &crash) {
  V3 pe = quat_apply(conj(qveh), tgt - s.p);  // quat_apply_inverse
  float dist = norm(pe);
  float pos_reward = 3.0f * exp_cw(-8.0f * dist * dist) + 2.0f * exp_cw(-4.0f * dist * dist);
  float dist_reward = (20.0f - dist) / 40.0f;
  V3 up = quat_rotate(s.q, V3{0.0f, 0.0f, 1.0f});  // quat_axis(q, 2)
  float tilt = fabsf(1.0f - up.z);
  float up_reward = (1.0f / (0.1f + tilt * tilt)) * 0.2f;  // `0.2 / tensor` is tensor.reciprocal() * 0.2 in torch (eager and TorchScript)
  float spin = norm(wb);
  float ang_reward = (1.0f / (1.0f + spin * spin)) * 3.0f;
  float total = pos_reward + dist_reward + pos_reward * (up_reward + ang_reward);
  total = 1.0f * total;
  if (dist > 8.0f) crash = true;
  if (crash) total = -20.0f;
  return total;
}

// navigation_task.py:416-521 on registers
AGX_DEV float reward_navigation(const float *rp, float cpf, V3 pe, V3 ppe, float a0, float a2, float a3, float p0, float p2,
                                float p3, bool crash) {
  float mult = 1.0f + 2.0f * cpf;
  float dist = norm(pe), prev_dist = norm(ppe);
  float pos_reward = exp_reward(rp[0], rp[1], dist);
  float close_reward = exp_reward(rp[2], rp[3], dist);
  float closer = prev_dist - dist;
  float closer_reward = (closer > 0.0f) ? rp[4] * closer : 2.0f * rp[4] * closer;
  float dist_reward = (20.0f - dist) / 20.0f;
  float dx = a0 - p0, dz = a2 - p2, dyaw = a3 - p3;
  float diff_pen = exp_penalty(rp[5], rp[6], dx) + exp_penalty(rp[7], rp[8], dz) + exp_penalty(rp[9], rp[10], dyaw);
  float abs_pen = cpf * exp_penalty(rp[11], rp[12], a0) + cpf * exp_penalty(rp[13], rp[14], a2) +
                  cpf * exp_penalty(rp[15], rp[16], a3);
  float total_pen = diff_pen + abs_pen;
  float r = mult * (pos_reward + close_reward + closer_reward + dist_reward) + total_pen;
  if (crash) r = rp[17];
  return r;
}

// NavigationTask bookkeeping (navigation_task.py:311-326) on the registers of the step's epilogue -- the arithmetic of k_nav_bookkeeping
// (agx_task_glue.hip): near = norm(target - p) < radius.  `store`: this lane stores the env's flags (one lane per env).  Must be
// reached by every lane of the wave that runs the epilogue (the counters are bumped once per wave).
AGX_DEV void nav_bookkeeping_epilogue(const AgxTaskArgs &T, int i, bool store, V3 tgt, V3 p, bool crashed, bool trunc) {
  const bool near = norm(tgt - p) < T.success_radius;
  const bool succ = store && trunc && near && !crashed;
  const bool tout = store && trunc && !succ && !crashed;
  if (store) {
    T.successes[i] = succ ? 1 : 0;
    T.timeouts[i] = tout ? 1 : 0;
  }
  const unsigned long long act = __ballot(true);
  const unsigned long long ms = __ballot(succ), mc = __ballot(store && crashed), mt = __ballot(tout);
  if ((int)(threadIdx.x & 63) == __ffsll((long long)act) - 1) {
    if (ms) atomicAdd(T.counters + 0, __popcll(ms));
    if (mc) atomicAdd(T.counters + 1, __popcll(mc));
    if (mt) atomicAdd(T.counters + 2, __popcll(mt));
  }
}

// ---------------------------------------------------------------------------------------
// Stand-alone task kernels (same device functions as the fused epilogue)
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_reward_position(AgxEnvBuffers B, int n, const float *__restrict__ target, int episode_len,
                                                          int reset_on_collision, float *__restrict__ reward) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool reset = false;
  if (i < n) {
    EnvState s = load_state(B.state, n, i);
    Q4 qveh = Q4{AGX_AT(B.derived, 3), AGX_AT(B.derived, 4), AGX_AT(B.derived, 5), AGX_AT(B.derived, 6)};
    V3 wb = V3{AGX_AT(B.derived, 13), AGX_AT(B.derived, 14), AGX_AT(B.derived, 15)};
    V3 tgt = V3{AGX_AT(target, 0), AGX_AT(target, 1), AGX_AT(target, 2)};
    bool crash = B.crashes[i] != 0;
    reward[i] = reward_position(s, qveh, wb, tgt, crash);
    B.crashes[i] = crash ? 1 : 0;
    reset = reset_set_truncate(B, i, crash, episode_len, reset_on_collision);
  }
  reset_flag_raise(B, reset);
}

// position_setpoint_task.py:194-203, obs [N][13] row-major (what the policy network consumes)
AGX_DEV void write_obs_position(const AgxEnvBuffers &B, int n, int i, V3 tgt, float *__restrict__ obs, const EnvState &s,
                                const Derived &d) {
  float v[13] = {tgt.x - s.p.x, tgt.y - s.p.y, tgt.z - s.p.z, s.q.x, s.q.y, s.q.z, s.q.w,
                 d.vbody.x, d.vbody.y, d.vbody.z, d.wbody.x, d.wbody.y, d.wbody.z};
  float *o = obs + (size_t)i * 13;
#pragma unroll
  for (int c = 0; c < 13; ++c) o[c] = v[c];
  if (float *rows = B.step_rows[B.flag_parity]) {
    float *r = rows + (size_t)i * 16;
    if (B.push_world > 0) {  // the 64-byte row as four 16-byte stores per destination
      row_store4_push(B, r, v[0], v[1], v[2], v[3]);
      row_store4_push(B, r + 4, v[4], v[5], v[6], v[7]);
      row_store4_push(B, r + 8, v[8], v[9], v[10], v[11]);
      row_store4_push(B, r + 12, v[12], B.step_reward[i], B.crashes[i] ? 1.0f : 0.0f, B.truncations[i] ? 1.0f : 0.0f);
    } else {
#pragma unroll
      for (int c = 0; c < 13; ++c) row_store(B, r + c, v[c]);
      write_step_row_tail(B, i, r, 13);
    }
  }
}
__global__ void __launch_bounds__(256) k_obs_position(AgxEnvBuffers B, int n, const float *__restrict__ target, float *__restrict__ obs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  push_wait_for_slot(B);
  if (i < n)
    write_obs_position(B, n, i, V3{AGX_AT(target, 0), AGX_AT(target, 1), AGX_AT(target, 2)}, obs, load_state(B.state, n, i),
                       load_derived(B.derived, n, i));
  step_rows_signal(B);
}

struct NavParams {
  float rp[18];
};

// navigation_task.py:416-521 (+ :305-309 truncation)
__global__ void __launch_bounds__(256) k_reward_navigation(AgxEnvBuffers B, int n, const float *__restrict__ target, NavParams R,
                                                            float cpf, float *__restrict__ pos_err,
                                                            float *__restrict__ prev_pos_err, int episode_len,
                                                            int reset_on_collision, float *__restrict__ reward) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool reset = false;
  if (i < n) {
    V3 p = V3{AGX_AT(B.state, 0), AGX_AT(B.state, 1), AGX_AT(B.state, 2)};
    Q4 qveh = Q4{AGX_AT(B.derived, 3), AGX_AT(B.derived, 4), AGX_AT(B.derived, 5), AGX_AT(B.derived, 6)};
    V3 tgt = V3{AGX_AT(target, 0), AGX_AT(target, 1), AGX_AT(target, 2)};
    V3 ppe = V3{AGX_AT(pos_err, 0), AGX_AT(pos_err, 1), AGX_AT(pos_err, 2)};
    AGX_AT(prev_pos_err, 0) = ppe.x; AGX_AT(prev_pos_err, 1) = ppe.y; AGX_AT(prev_pos_err, 2) = ppe.z;
    V3 pe = quat_rotate_inverse(qveh, tgt - p);
    AGX_AT(pos_err, 0) = pe.x; AGX_AT(pos_err, 1) = pe.y; AGX_AT(pos_err, 2) = pe.z;
    bool crash = B.crashes[i] != 0;
    reward[i] = reward_navigation(R.rp, cpf, pe, ppe, AGX_AT(B.actions, 0), AGX_AT(B.actions, 2), AGX_AT(B.actions, 3),
                                  AGX_AT(B.prev_actions, 0), AGX_AT(B.prev_actions, 2), AGX_AT(B.prev_actions, 3), crash);
    reset = reset_set_truncate(B, i, crash, episode_len, reset_on_collision);
  }
  reset_flag_raise(B, reset);
}

// navigation_task.py:369-393; one wave per env so the depth min-pool is a coalesced sweep
// (part, nparts): the env's work split over `nparts` waves -- the state part goes to the last one, the cell rows cy = part,
// part + nparts, ... of the min-pool to each; the minimum over the image comes back as this wave's share (the caller reduces).
AGX_DEV float obs_navigation_env(const AgxEnvBuffers &B, int n, int i, const float *__restrict__ target,
                                 const float *__restrict__ u_vec, const float *__restrict__ u_euler,
                                 const float *__restrict__ pixels, int ns, int H, int W, int gh, int gw, int obs_dim,
                                 float *__restrict__ obs, float *__restrict__ min_pixel, int part = 0, int nparts = 1) {
  const int lane = threadIdx.x & 63;
  float *o = obs + (size_t)i * obs_dim;
  float *row = B.step_rows[B.flag_parity] ? B.step_rows[B.flag_parity] + (size_t)i * (obs_dim + 3) : nullptr;
  float imin = INFINITY;  // NavigationTask.post_image_reward_addition on the same sweep (min_pixel != NULL, ns == 1)
  if (lane == 0 && part == nparts - 1) {
    V3 p = V3{AGX_AT(B.state, 0), AGX_AT(B.state, 1), AGX_AT(B.state, 2)};
    Q4 qveh = Q4{AGX_AT(B.derived, 3), AGX_AT(B.derived, 4), AGX_AT(B.derived, 5), AGX_AT(B.derived, 6)};
    V3 tgt = V3{AGX_AT(target, 0), AGX_AT(target, 1), AGX_AT(target, 2)};
    V3 v = quat_rotate_inverse(qveh, tgt - p);
    float u6[6];
    if (u_vec) {
#pragma unroll
      for (int c = 0; c < 3; ++c) { u6[c] = u_vec[(size_t)i * 3 + c]; u6[3 + c] = u_euler[(size_t)i * 3 + c]; }
    } else {
      rng_fill<6>(B.rng_seed, B.env_index_base + i, agx::step_index(B), RNG_OBS_NOISE, u6);
    }
    // 0.1 * 2 * rand_like(vec - 0.5): the -0.5 sits inside rand_like in the reference (:374)
    V3 pv = V3{v.x + 0.1f * 2.0f * u6[0], v.y + 0.1f * 2.0f * u6[1], v.z + 0.1f * 2.0f * u6[2]};
    float dist = norm(v);
    o[0] = pv.x / dist; o[1] = pv.y / dist; o[2] = pv.z / dist; o[3] = dist;
    float e0 = ssa(AGX_AT(B.derived, 0)), e1 = ssa(AGX_AT(B.derived, 1));
    o[4] = e0 + 0.1f * (u6[3] - 0.5f);
    o[5] = e1 + 0.1f * (u6[4] - 0.5f);
    o[6] = 0.0f;
    o[7] = AGX_AT(B.derived, 10); o[8] = AGX_AT(B.derived, 11); o[9] = AGX_AT(B.derived, 12);
    o[10] = AGX_AT(B.derived, 13); o[11] = AGX_AT(B.derived, 14); o[12] = AGX_AT(B.derived, 15);
    o[13] = AGX_AT(B.actions, 0); o[14] = AGX_AT(B.actions, 1); o[15] = AGX_AT(B.actions, 2); o[16] = AGX_AT(B.actions, 3);
    if (row) {
      for (int c = 0; c < 17 && c < obs_dim; ++c) row_store(B, row + c, o[c]);  // this lane's own stores
      write_step_row_tail(B, i, row, obs_dim);
    }
  }
  if (pixels) {
    // gh x gw min-pool of sensor 0's image as a COALESCED sweep: the wave reads 64 consecutive pixels of a row per load
    // (each lane keeps the minimum of its column over the rows of the cell row), then the columns of one cell are
    // reduced across lanes.  min is exact and order-free, so any arrangement gives the bits of the serial loop.
    const float *img = pixels + (size_t)i * ns * H * W;  // sensor 0
    const int ch = (H + gh - 1) / gh;
    // wide images (W >= 256, cells a multiple of 4 pixels wide: the 32 x 512 LiDAR): a lane takes 4 consecutive pixels per
    // load (1 KB per wave instruction instead of 256 B) and the sweep below runs over these groups of 4
    const bool vec4 = (W & 3) == 0 && W >= 256 && (((W + gw - 1) / gw) & 3) == 0 && ((size_t)img & 15) == 0;
    const int Wv = vec4 ? W >> 2 : W;                    // columns the sweep sees
    const int cw = ((W + gw - 1) / gw) >> (vec4 ? 2 : 0);  // cell width in such columns
    const bool pow2 = (cw & (cw - 1)) == 0 && cw < 64;
    for (int cy = part; cy < gh; cy += nparts) {
      const int y0 = cy * ch, y1 = min(y0 + ch, H);
      float cell = INFINITY;  // lane c < gw: cell (cy, c)
      for (int x0 = 0; x0 < Wv && y0 < y1; x0 += 64) {
        const int x = x0 + lane;
        float m = INFINITY;
        if (x < Wv) {
          // one wave per env: the rows of a cell are requested TOGETHER (batches of 8 loads in flight) -- issued one by one, the
          // 48 row loads of a 64 x 48 frame were 48 memory latencies in sequence and the whole kernel (min is exact: any order)
          for (int yb = y0; yb < y1; yb += 8) {
            if (vec4) {
              float4 v4[8];
#pragma unroll
              for (int r = 0; r < 8; ++r) {
                const int y = min(yb + r, y1 - 1);  // (a row read twice changes no minimum)
                v4[r] = *reinterpret_cast<const float4 *>(img + (size_t)y * W + 4 * x);
              }
#pragma unroll
              for (int r = 0; r < 8; ++r) {
                const float vv[4] = {v4[r].x, v4[r].y, v4[r].z, v4[r].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                  m = fminf(m, vv[k]);
                  float v10 = 10.0f * vv[k];
                  if (v10 < 0.0f) v10 = 10.0f;
                  imin = fminf(imin, v10);
                }
              }
            } else {
              float vr[8];
#pragma unroll
              for (int r = 0; r < 8; ++r) vr[r] = img[(size_t)min(yb + r, y1 - 1) * W + x];
#pragma unroll
              for (int r = 0; r < 8; ++r) {
                m = fminf(m, vr[r]);
                float v10 = 10.0f * vr[r];
                if (v10 < 0.0f) v10 = 10.0f;
                imin = fminf(imin, v10);
              }
            }
          }
        }
        if (pow2) {  // cells are aligned groups of cw lanes: butterfly inside the group, lane c fetches its group's value
          for (int sft = 1; sft < cw; sft <<= 1) m = fminf(m, __shfl_xor(m, sft));
          const int src = lane * cw - x0;
          const float t = __shfl(m, src & 63);
          if (src >= 0 && src < 64 && lane < gw) cell = fminf(cell, t);
        } else {
          const int c_lo = x0 / cw, c_hi = min(x0 + 63, Wv - 1) / cw;
          for (int c = c_lo; c <= c_hi; ++c) {  // wave-uniform: the cells this 64-column chunk touches
            float t = (x < Wv && x / cw == c) ? m : INFINITY;
            for (int off = 32; off > 0; off >>= 1) t = fminf(t, __shfl_xor(t, off));
            if (lane == c) cell = fminf(cell, t);
          }
        }
      }
      const int k = 17 + cy * gw + lane;
      if (lane < gw && k < obs_dim) {
        o[k] = cell;
        if (row) row_store(B, row + k, cell);
      }
    }
    if (min_pixel) {
      for (int off = 32; off > 0; off >>= 1) imin = fminf(imin, __shfl_xor(imin, off));
      if (lane == 0 && nparts == 1) min_pixel[i] = imin;
    }
  }
  return imin;
}
// Small batches (the 256 .. 2048 envs an RL run uses): one WORKGROUP per env, its four waves take every fourth cell row of the
// min-pool each and the last one the state part as well -- the one-wave-per-env form runs the eight cell rows' loads as eight
// memory round trips in sequence and the Philox draws of the state part in front of them (13 us at 256 envs; this one: 5).
// min is exact and order-free: the same bits.
__global__ void __launch_bounds__(256) k_obs_navigation_split(AgxEnvBuffers B, int n, const float *__restrict__ target,
                                                               const float *__restrict__ u_vec, const float *__restrict__ u_euler,
                                                               const float *__restrict__ pixels, int ns, int H, int W, int gh, int gw,
                                                               int obs_dim, float *__restrict__ obs, float *__restrict__ min_pixel) {
  __shared__ float wave_min[4];
  const int i = blockIdx.x, w = threadIdx.x >> 6;
  push_wait_for_slot(B);
  const float imin = obs_navigation_env(B, n, i, target, u_vec, u_euler, pixels, ns, H, W, gh, gw, obs_dim, obs, min_pixel, w, 4);
  if (min_pixel && pixels) {
    if ((threadIdx.x & 63) == 0) wave_min[w] = imin;
    __syncthreads();
    if (threadIdx.x == 0) min_pixel[i] = fminf(fminf(wave_min[0], wave_min[1]), fminf(wave_min[2], wave_min[3]));
  }
  step_rows_signal(B);
}
__global__ void __launch_bounds__(256) k_obs_navigation(AgxEnvBuffers B, int n, const float *__restrict__ target,
                                                         const float *__restrict__ u_vec, const float *__restrict__ u_euler,
                                                         const float *__restrict__ pixels, int ns, int H, int W, int gh, int gw,
                                                         int obs_dim, float *__restrict__ obs, float *__restrict__ min_pixel) {
  const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);  // one wave per env
  push_wait_for_slot(B);
  if (i < n) obs_navigation_env(B, n, i, target, u_vec, u_euler, pixels, ns, H, W, gh, gw, obs_dim, obs, min_pixel);
  step_rows_signal(B);
}
}  // namespace agx

extern "C" int agx_reward_position(const AgxEnvBuffers *B, int n, const float *target, int episode_len,
                                   int reset_on_collision, float *reward, void *stream) {
  if (int e = check_common(nullptr, B, n)) return e;
  AGX_REQUIRE(target && reward && B->reset_flag && B->reset_mask && B->state && B->derived && B->crashes && B->truncations &&
                  B->sim_steps,
              "null buffer");
  const int block = pick_block(n);
  hipLaunchKernelGGL(k_reward_position, dim3(blocks_for(n, block)), dim3(block), 0, (hipStream_t)stream, *B, n, target,
                     episode_len, reset_on_collision, reward);
  return check_launch("agx_reward_position");
}

extern "C" int agx_obs_position(const AgxEnvBuffers *B, int n, const float *target, float *obs, void *stream) {
  if (int e = check_common(nullptr, B, n)) return e;
  AGX_REQUIRE(target && obs && B->state && B->derived, "null buffer");
  const int block = pick_block(n);
  hipLaunchKernelGGL(k_obs_position, dim3(blocks_for(n, block)), dim3(block), 0, (hipStream_t)stream, *B, n, target, obs);
  return check_launch("agx_obs_position");
}

extern "C" int agx_reward_navigation(const AgxEnvBuffers *B, int n, const float *target, const float *rp, float cpf,
                                     float *pos_err, float *prev_pos_err, int episode_len, int reset_on_collision,
                                     float *reward, void *stream) {
  if (int e = check_common(nullptr, B, n)) return e;
  AGX_REQUIRE(target && rp && pos_err && prev_pos_err && reward && B->reset_flag && B->reset_mask, "null buffer");
  AGX_REQUIRE(B->state && B->derived && B->actions && B->prev_actions && B->crashes && B->truncations && B->sim_steps,
              "null env buffer");
  NavParams R;
  for (int c = 0; c < 18; ++c) R.rp[c] = rp[c];  // rp is a HOST pointer (18 config scalars)
  const int block = pick_block(n);
  hipLaunchKernelGGL(k_reward_navigation, dim3(blocks_for(n, block)), dim3(block), 0, (hipStream_t)stream, *B, n, target, R, cpf,
                     pos_err, prev_pos_err, episode_len, reset_on_collision, reward);
  return check_launch("agx_reward_navigation");
}

extern "C" int agx_obs_navigation(const AgxEnvBuffers *B, int n, const float *target, const float *u_vec,
                                  const float *u_euler, const float *pixels, int ns, int H, int W, int gh, int gw,
                                  int obs_dim, float *obs, float *min_pixel, void *stream) {
  if (int e = check_common(nullptr, B, n)) return e;
  AGX_REQUIRE(!min_pixel || (pixels && ns == 1), "min_pixel: needs the image, and covers it only with one sensor");
  AGX_REQUIRE(target && obs && B->state && B->derived && B->actions, "null buffer");
  AGX_REQUIRE((u_vec == nullptr) == (u_euler == nullptr), "u_vec and u_euler: both tensors or both NULL (device generator)");
  AGX_REQUIRE(obs_dim >= 17, "obs_dim must be >= 17");
  AGX_REQUIRE(!pixels || (ns > 0 && H > 0 && W > 0 && gh > 0 && gw > 0), "bad image sizes");
  if (pixels && n <= 2048 && gh >= 4)
    hipLaunchKernelGGL(k_obs_navigation_split, dim3(n), dim3(256), 0, (hipStream_t)stream, *B, n, target, u_vec, u_euler, pixels, ns, H,
                       W, gh, gw, obs_dim, obs, min_pixel);
  else
    hipLaunchKernelGGL(k_obs_navigation, dim3(blocks_for(n, 4)), dim3(256), 0, (hipStream_t)stream, *B, n, target, u_vec,
                       u_euler, pixels, ns, H, W, gh, gw, obs_dim, obs, min_pixel);
  return check_launch("agx_obs_navigation");
}
