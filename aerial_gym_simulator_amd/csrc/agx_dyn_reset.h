#pragma once
// The reset path: the draws (host tensors or Philox in place), the masked reset kernels with and without the position observation,
// the navigation robot side, the asset reset, and their entry points (agx_post_step_position included).
// Part of the one translation unit agx_dynamics.hip, which alone includes it (after the AGX_DYN_* switches).

namespace agx {
// ---------------------------------------------------------------------------------------
// Reset.  Uniform draws come either from tensors (host RNG, reference-faithful stream) or
// from Philox4x32-10 evaluated in place (sync-free mode).
// ---------------------------------------------------------------------------------------
// The uniform draws one env's reset consumes: env bounds (6), robot state (13), controller gains (12), and per motor
// (tau_inc, tau_dec, thrust, kT).
template <int M>
struct ResetDraws {
  float ub[6], us[13], ug[12], um[M][4];
};

// strict mode: the tensors torch drew (AoS, the reference's order)
// MOTORS = false (the ROV kind): BaseROV.reset_idx draws nothing for the motors, u_tau_inc .. u_kT may be NULL
template <int M, bool MOTORS = true>
AGX_DEV void host_reset_draws(const AgxRobotParams &P, const AgxResetArgs &R, int i, ResetDraws<M> &D) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    D.ub[c] = R.u_bounds_lo[(size_t)i * 3 + c];
    D.ub[3 + c] = R.u_bounds_hi[(size_t)i * 3 + c];
  }
#pragma unroll
  for (int c = 0; c < 13; ++c) D.us[c] = R.u_state[(size_t)i * 13 + c];
#pragma unroll
  for (int c = 0; c < 12; ++c) D.ug[c] = R.randomize_gains ? R.u_gains[(size_t)i * 12 + c] : 0.0f;
#pragma unroll
  for (int j = 0; j < (MOTORS ? M : 0); ++j) {
    size_t k = (size_t)i * M + j;
    D.um[j][0] = R.u_tau_inc[k];
    D.um[j][1] = R.u_tau_dec[k];
    D.um[j][2] = R.u_thrust[k];
    D.um[j][3] = P.use_rps ? R.u_kT[k] : 0.0f;
  }
}

// sync-free mode: the Philox blocks of a resetting env are evaluated by the WAVE, one block per lane (2 bounds + 4 state
// + 3 gains + M motor blocks of 4 draws), and handed to the env's own lane with v_readlane: a lane on its own would run
// the 9 + M blocks (10 rounds each) back to back, and with a few of 8192 envs resetting on almost every step that
// serial chain was the longest path of the reset / observation kernel.  Same (seed; env, episode, stream, block)
// coordinates, hence the same draws as rng_fill / rng_block in any other arrangement.  Must be called by all 64 lanes.
template <int M, bool MOTORS = true>
AGX_DEV void wave_reset_draws(const AgxResetArgs &R, int i, int ep, bool mine, ResetDraws<M> &D) {
  constexpr int NB = 9 + (MOTORS ? M : 0);
  const int lane = threadIdx.x & 63;
  int stream = RNG_MOTOR, blk = lane - 9;
  if (lane < 2) { stream = RNG_BOUNDS; blk = lane; }
  else if (lane < 6) { stream = RNG_STATE; blk = lane - 2; }
  else if (lane < 9) { stream = RNG_GAINS; blk = lane - 6; }
  unsigned long long todo = __ballot(mine);
  if (__popcll(todo) > 8) {  // a full reset (task.reset(), short episodes): every lane for itself is the shorter path
    if (mine) {
      rng_fill<6>(R.seed, i, ep, RNG_BOUNDS, D.ub);
      rng_fill<13>(R.seed, i, ep, RNG_STATE, D.us);
      if (R.randomize_gains) rng_fill<12>(R.seed, i, ep, RNG_GAINS, D.ug);
#pragma unroll
      for (int j = 0; j < (MOTORS ? M : 0); ++j) {
        F4 um = rng_block(R.seed, i, ep, RNG_MOTOR, j);
#pragma unroll
        for (int k = 0; k < 4; ++k) D.um[j][k] = um.v[k];
      }
    }
    return;
  }
  while (todo) {
    const int L = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int iL = __builtin_amdgcn_readlane(i, L), epL = __builtin_amdgcn_readlane(ep, L);
    F4 f{};
    if (lane < NB) f = rng_block(R.seed, iL, epL, stream, blk);
    const bool me = lane == L;
#define AGX_TAKE(dst, b, k)                                                                   \
  {                                                                                            \
    float v_ = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(f.v[k]), (b)));          \
    dst = me ? v_ : dst;                                                                       \
  }
#pragma unroll
    for (int c = 0; c < 6; ++c) AGX_TAKE(D.ub[c], c / 4, c % 4)
#pragma unroll
    for (int c = 0; c < 13; ++c) AGX_TAKE(D.us[c], 2 + c / 4, c % 4)
    if (R.randomize_gains) {
#pragma unroll
      for (int c = 0; c < 12; ++c) AGX_TAKE(D.ug[c], 6 + c / 4, c % 4)
    }
#pragma unroll
    for (int j = 0; j < (MOTORS ? M : 0); ++j) {
#pragma unroll
      for (int k = 0; k < 4; ++k) AGX_TAKE(D.um[j][k], 9 + j, k)
    }
#undef AGX_TAKE
  }
}

// BaseMultirotor.reset_idx / MotorModel.reset_idx / IsaacGymEnv.reset_idx of ONE env from its draws, in two halves: the values
// (arithmetic only: the helper wave of k_position_step_fused<AGX_STEP_ANY> evaluates them before it may store anything) ...
template <int M>
struct ResetValues {
  float bmin[3], bmax[3], gains[12], mot[M][4];  // mot[j]: tau_inc, tau_dec, thrust, kT
  EnvState s;
};
template <int M>
AGX_DEV ResetValues<M> reset_env_values(const AgxRobotParams &P, const AgxResetArgs &R, const ResetDraws<M> &D) {
  ResetValues<M> V;
  // IsaacGymEnv.reset_idx: env bounds first, the robot spawn uses them
  bounds_from_draws(R, D.ub, V.bmin, V.bmax);
  const float *bmin = V.bmin, *bmax = V.bmax;
  float r[13];
#pragma unroll
  for (int c = 0; c < 13; ++c) r[c] = (R.max_state[c] - R.min_state[c]) * D.us[c] + R.min_state[c];
  V.s.p = V3{bmin[0] + (bmax[0] - bmin[0]) * r[0], bmin[1] + (bmax[1] - bmin[1]) * r[1], bmin[2] + (bmax[2] - bmin[2]) * r[2]};
  V.s.q = quat_from_euler(r[3], r[4], r[5]);
  V.s.v = V3{r[7], r[8], r[9]};
  V.s.w = V3{r[10], r[11], r[12]};
#pragma unroll
  for (int c = 0; c < 12; ++c) V.gains[c] = (R.gains_max[c] - R.gains_min[c]) * D.ug[c] + R.gains_min[c];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    V.mot[j][0] = (R.tau_inc_max - R.tau_inc_min) * D.um[j][0] + R.tau_inc_min;
    V.mot[j][1] = (R.tau_dec_max - R.tau_dec_min) * D.um[j][1] + R.tau_dec_min;
    V.mot[j][2] = (P.max_thrust - P.min_thrust) * D.um[j][2] + P.min_thrust;
    V.mot[j][3] = (R.kT_max - R.kT_min) * D.um[j][3] + R.kT_min;
  }
  return V;
}
// ... and the stores
// MOTORS = false (the ROV kind): base_rov.py:171-198 does not call control_allocator.reset_idx -- motor thrusts and motor constants
// of a resetting env stay exactly as they are
template <int M, bool MOTORS = true>
AGX_DEV void reset_env_store(const AgxRobotParams &P, const AgxEnvBuffers &B, int n, const AgxResetArgs &R, int i, int ep,
                             const ResetValues<M> &V) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    AGX_AT(B.bounds_min, c) = V.bmin[c];
    AGX_AT(B.bounds_max, c) = V.bmax[c];
  }
  store_state(B.state, n, i, V.s);
  if (R.randomize_gains) {
#pragma unroll
    for (int c = 0; c < 12; ++c) AGX_AT(B.gains, c) = V.gains[c];
  }
#pragma unroll
  for (int j = 0; j < (MOTORS ? M : 0); ++j) {
    if (B.motor_tau_inc) AGX_AT(B.motor_tau_inc, j) = V.mot[j][0];
    if (B.motor_tau_dec) AGX_AT(B.motor_tau_dec, j) = V.mot[j][1];
    AGX_AT(B.motor_thrust, j) = V.mot[j][2];
    if (P.use_rps) AGX_AT(B.motor_kT, j) = V.mot[j][3];
  }
  B.sim_steps[i] = 0;
  if (B.episode_count) B.episode_count[i] = ep + 1;
}
// returns the new state
template <int M, bool MOTORS = true>
AGX_DEV EnvState reset_env(const AgxRobotParams &P, const AgxEnvBuffers &B, int n, const AgxResetArgs &R, int i, int ep,
                           const ResetDraws<M> &D) {
  const ResetValues<M> V = reset_env_values<M>(P, R, D);
  reset_env_store<M, MOTORS>(P, B, n, R, i, ep, V);
  return V.s;
}

// What follows the reset decision of one env step, for one env: the masked reset (base_multirotor.py:177-205,
// motor_model.py:140-154, env_manager.py:301) and, when WITH_OBS, the position task's observation of the post-reset state.
// `any`: some env of the batch resets (wave-uniform); s / d: the env's state and derived tensors as the step left them.
// Must be called by all 64 lanes (wave_reset_draws).
// ROV: BaseROV.reset_idx (base_rov.py:171-198) -- no motor draws, motor state untouched, Euler angles of the refresh without ssa().
template <int M, bool WITH_OBS, bool ROV = false>
AGX_DEV void reset_and_observe(const AgxRobotParams &P, const AgxEnvBuffers &B, int n, const AgxResetArgs &R, int i, bool valid,
                               bool any, bool mine, int ep, V3 tgt, float *__restrict__ obs, const EnvState &s, const Derived &d) {
  if (!any) {  // nobody resets: the reference does not touch anything
    if (WITH_OBS && valid) write_obs_position(B, n, i, tgt, obs, s, d);
    return;
  }
  ResetDraws<M> D{};
  if (R.u_state) {
    if (mine) host_reset_draws<M, !ROV>(P, R, i, D);
  } else {
    wave_reset_draws<M, !ROV>(R, B.env_index_base + i, ep, mine, D);  // draws are keyed by the GLOBAL env index
  }
  if (valid) {
    EnvState s2 = mine ? reset_env<M, !ROV>(P, B, n, R, i, ep, D) : s;
    // BaseMultirotor.reset_idx ends with an un-indexed update_states(): every env is refreshed
    // (lean: nobody reads the derived tensors before the next env step rewrites them; the observation reads the body velocities)
    const bool lean = (B.launch_flags & 4) != 0;
    Derived d2 = lean ? update_states_body(s2) : (ROV ? update_states_rov(s2) : update_states(s2));
    if (!lean) store_derived(B.derived, n, i, d2);
    if (WITH_OBS) write_obs_position(B, n, i, tgt, obs, s2, d2);
  }
}

// The reset / observation half of the env step as its own launch.  Every load is issued before the flag is looked at (one
// memory round trip instead of flag -> mask -> state in sequence).
template <int M, bool WITH_OBS>
__global__ void __launch_bounds__(256) k_reset_masked(AgxRobotParams P, AgxEnvBuffers B, int n, AgxResetArgs R,
                                                      const float *__restrict__ target, float *__restrict__ obs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) B.reset_flag[B.flag_parity ^ 1] = 0;  // the NEXT step's flag; nobody reads or writes it now
  if (WITH_OBS) push_wait_for_slot(B);
  const bool valid = i < n;
  EnvState s{};
  Derived d{};
  V3 tgt{};
  int mask = 0, ep = 0;
  if (valid) {
    s = load_state(B.state, n, i);
    if (WITH_OBS) {
      d = load_derived(B.derived, n, i);
      tgt = V3{AGX_AT(target, 0), AGX_AT(target, 1), AGX_AT(target, 2)};
    }
    mask = B.reset_mask[i];  // compared below, behind the last load (see reset_masked_quad_obs_body)
    if (B.episode_count) ep = B.episode_count[i];
  }
  const int flag = B.reset_flag[B.flag_parity];  // (one word: the branch is taken by whole waves)
  const bool any = flag != 0, mine = mask != 0;
  reset_and_observe<M, WITH_OBS>(P, B, n, R, i, valid, any, mine && any, ep, tgt, obs, s, d);
  if (WITH_OBS) step_rows_signal(B);
}

// k_reset_masked<8, WITH_OBS> of the ROV kind (AGX_LAUNCH_ROV): the same loads in the same order, reset_and_observe<8, WITH_OBS, true>
template <bool WITH_OBS>
__global__ void __launch_bounds__(256) k_reset_masked_rov(AgxRobotParams P, AgxEnvBuffers B, int n, AgxResetArgs R,
                                                          const float *__restrict__ target, float *__restrict__ obs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) B.reset_flag[B.flag_parity ^ 1] = 0;  // the NEXT step's flag; nobody reads or writes it now
  if (WITH_OBS) push_wait_for_slot(B);
  const bool valid = i < n;
  EnvState s{};
  Derived d{};
  V3 tgt{};
  int mask = 0, ep = 0;
  if (valid) {
    s = load_state(B.state, n, i);
    if (WITH_OBS) {
      d = load_derived(B.derived, n, i);
      tgt = V3{AGX_AT(target, 0), AGX_AT(target, 1), AGX_AT(target, 2)};
    }
    mask = B.reset_mask[i];
    if (B.episode_count) ep = B.episode_count[i];
  }
  const int flag = B.reset_flag[B.flag_parity];  // (one word: the branch is taken by whole waves)
  const bool any = flag != 0, mine = mask != 0;
  reset_and_observe<8, WITH_OBS, true>(P, B, n, R, i, valid, any, mine && any, ep, tgt, obs, s, d);
  if (WITH_OBS) step_rows_signal(B);
}

// The robot side of a navigation step in one launch (agx_nav_robot_side): the masked robot reset, the sensor mounts and the
// target of the envs that reset, the world pose of every sensor -- four dependent launches of ~5 us each at RL batch sizes.
// Same device functions as the stand-alone kernels, same order; what the later parts read (episode count, bounds, state) was
// written by the SAME thread, so program order is all the ordering it takes.
template <int M>
__global__ void __launch_bounds__(256) k_nav_robot_side(AgxRobotParams P, AgxEnvBuffers B, int n, AgxResetArgs R, AgxNavRobotSideArgs A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) B.reset_flag[B.flag_parity ^ 1] = 0;  // the NEXT step's flag; nobody reads or writes it now
  const bool valid = i < n;
  EnvState s{};
  int mask = 0, ep = 0;
  if (valid) {
    s = load_state(B.state, n, i);
    mask = B.reset_mask[i];  // compared below, behind the last load (see reset_masked_quad_obs_body)
    if (B.episode_count) ep = B.episode_count[i];
  }
  const int flag = B.reset_flag[B.flag_parity];  // (one word: the branch is taken by whole waves)
  const bool any = flag != 0, mine = mask != 0;
  reset_and_observe<M, false>(P, B, n, R, i, valid, any, mine && any, ep, V3{}, nullptr, s, Derived{});
  if (!valid) return;
  const int ns = A.num_sensors;
  if (any && mine) {
    if (A.randomize_mount) {
      Ratio3 Tr, Ro;
#pragma unroll
      for (int c = 0; c < 3; ++c) { Tr.lo[c] = A.mount_t_min[c]; Tr.hi[c] = A.mount_t_max[c]; Ro.lo[c] = A.mount_r_min[c]; Ro.hi[c] = A.mount_r_max[c]; }
      for (int q = 0; q < ns; ++q) sensor_mount_reset_env(B, i, q, i * ns + q, Tr, Ro, nullptr, nullptr, A.local_pos, A.local_quat);
    }
    if (A.reset_target) {
      Ratio3 Rt;
#pragma unroll
      for (int c = 0; c < 3; ++c) { Rt.lo[c] = A.target_ratio_min[c]; Rt.hi[c] = A.target_ratio_max[c]; }
      nav_target_reset_env(B, n, i, A.num_actions, Rt, nullptr, A.target, A.target_yaw, A.zero_prev_actions);
    }
  }
  const Q4 fq = Q4{A.frame_quat[0], A.frame_quat[1], A.frame_quat[2], A.frame_quat[3]};
  for (int q = 0; q < ns; ++q) sensor_pose_env(B, n, i, i * ns + q, A.local_pos, A.local_quat, fq, A.sensor_pos, A.sensor_quat);
}

// k_reset_masked<4, WITH_OBS> with four lanes per env (see k_env_step_quad_position): the refresh of every env's derived
// tensors and the observation are vector work; the reset of an env itself (rare: a few of 8192 per step) stays the scalar
// code, run by the first lane of the env's quad, which then hands the new state to the other three.
// HOST_DRAWS: the strict mode's uniforms come from tensors the host filled (R.u_state ...).  Its own instance, so that the
// kernel of the device-RNG mode holds none of those loads: at the join of the two paths the compiler otherwise waits
// (s_waitcnt vmcnt(N)) for loads that only the other path issued, and on gfx9 that counter also counts the STORES of a
// resetting env -- the slowest waves of the launch sat out their own stores' round trips twice.
template <bool HOST_DRAWS>
AGX_DEV void reset_masked_quad_obs_body(const AgxRobotParams &P, const AgxEnvBuffers &B, int n, const AgxResetArgs &R,
                                        const float *__restrict__ target, float *__restrict__ obs) {
  const int tid = threadIdx.x;
  const int l = tid & 3, l3 = l < 3 ? l : 2;
  const int i = blockIdx.x * 16 + (tid >> 2);
  const unsigned ol = ((unsigned)l * (unsigned)n + (unsigned)i) * 4u, ol3 = ((unsigned)l3 * (unsigned)n + (unsigned)i) * 4u;  // AGX_QAT
  if (blockIdx.x == 0 && tid == 0) B.reset_flag[B.flag_parity ^ 1] = 0;  // the NEXT step's flag; nobody reads or writes it now
  push_wait_for_slot(B);
  const bool valid = i < n;
  float p = 0.0f, q = 0.0f, v = 0.0f, w = 0.0f, vbody = 0.0f, wbody = 0.0f, tgt = 0.0f;
  int mask = 0, ep = 0, tail_crashed = 0, tail_truncated = 0;
  float tail_reward = 0.0f;
  float *const rows = B.step_rows[B.flag_parity];
  // every load is issued before ANY of them is looked at: one memory round trip.  (The mask is compared below, not here: a
  // compare inside this block made the compiler wait for the mask byte before it issued the episode count and the flag.)
  if (valid) {
    p = AGX_QAT(B.state, 0, ol3); q = AGX_QAT(B.state, 3, ol); v = AGX_QAT(B.state, 7, ol3); w = AGX_QAT(B.state, 10, ol3);
    vbody = AGX_QAT(B.derived, 10, ol3); wbody = AGX_QAT(B.derived, 13, ol3);
    tgt = AGX_QAT(target, 0, ol3);
    mask = B.reset_mask[i];
    if (B.episode_count) ep = B.episode_count[i];
    if (rows) {  // sharded run: reward | terminated | truncated ride behind the observation in the exchange row
      tail_reward = B.step_reward[i];
      tail_crashed = B.crashes[i];
      tail_truncated = B.truncations[i];
    }
  }
  const int flag = B.reset_flag[B.flag_parity];  // (one word: the branch is taken by whole waves)
  const bool any = flag != 0;
  const bool mine = mask != 0;
  if (any) {
    const bool lead = mine && l == 0;
    ResetDraws<4> D{};
    if (HOST_DRAWS) {
      if (lead) host_reset_draws<4>(P, R, i, D);
    } else {
      wave_reset_draws<4>(R, B.env_index_base + i, ep, lead, D);  // draws are keyed by the GLOBAL env index
    }
    if (__ballot(mine) != 0ull) {  // some env of this wave resets
      EnvState s{};
      if (lead) s = reset_env<4>(P, B, n, R, i, ep, D);
      // the quad takes the new state over from its first lane
      const float npv = q4::by_lane(l3, q4::bc<0>(s.p.x), q4::bc<0>(s.p.y), q4::bc<0>(s.p.z));
      const float nq = q4::by_lane(l, q4::bc<0>(s.q.x), q4::bc<0>(s.q.y), q4::bc<0>(s.q.z), q4::bc<0>(s.q.w));
      const float nv = q4::by_lane(l3, q4::bc<0>(s.v.x), q4::bc<0>(s.v.y), q4::bc<0>(s.v.z));
      const float nw = q4::by_lane(l3, q4::bc<0>(s.w.x), q4::bc<0>(s.w.y), q4::bc<0>(s.w.z));
      p = mine ? npv : p; q = mine ? nq : q; v = mine ? nv : v; w = mine ? nw : w;
    }
    // BaseMultirotor.reset_idx ends with an un-indexed update_states(): every env is refreshed
    const QuadDerived d = update_states_quad(q, v, w);
    if (valid) {
      if (l < 3) {
        AGX_QAT(B.derived, 0, ol) = d.euler;
        AGX_QAT(B.derived, 7, ol) = d.vveh;
        AGX_QAT(B.derived, 10, ol) = d.vbody;
        AGX_QAT(B.derived, 13, ol) = d.wbody;
      }
      AGX_QAT(B.derived, 3, ol) = d.qveh;
    }
    vbody = d.vbody;
    wbody = d.wbody;
  }
  if (valid) {  // position_setpoint_task.py:194-203: target - p | q | v_body | w_body
    float *o = obs + (size_t)i * 13;
    const float e = tgt - p;
    if (l < 3) { o[l] = e; o[7 + l] = vbody; o[10 + l] = wbody; }
    o[3 + l] = q;
    if (rows) {
      float *r = rows + (size_t)i * 16;
      if (B.push_world > 0) {
        // peer push: lane l stores elements 4 l .. 4 l + 3 of the row (e0 e1 e2 q0 | q1 q2 q3 vb0 | vb1 vb2 wb0 wb1 | wb2 reward
        // crashed truncated): the quad writes its env's 64-byte row as ONE line per destination, a wave 1 KB contiguous.
        // (the permutes are evaluated on the whole quad before the per-lane pick)
        const float e1 = q4::bc<1>(e), e2 = q4::bc<2>(e), q2 = q4::perm<0, 2, 2, 3>(q), q3 = q4::bc<3>(q);
        const float vb0 = q4::bc<0>(vbody), vb1 = q4::bc<1>(vbody), wb0 = q4::bc<0>(wbody), wb1 = q4::bc<1>(wbody), wb2 = q4::bc<2>(wbody);
        float t1 = 0.0f, t2 = 0.0f, t3 = 0.0f;
        if (l == 3) {
          t1 = tail_reward;
          t2 = tail_crashed ? 1.0f : 0.0f;
          t3 = tail_truncated ? 1.0f : 0.0f;
        }
        const float x0 = q4::by_lane(l, e, q, vb1, wb2);      // e0 (own) | q1 (own) | vb1 | wb2
        const float x1 = q4::by_lane(l, e1, q2, vbody, t1);   // e1 | q2 | vb2 (own) | reward
        const float x2 = q4::by_lane(l, e2, q3, wb0, t2);     // e2 | q3 | wb0 | crashed
        const float x3 = q4::by_lane(l, q, vb0, wb1, t3);     // q0 (own) | vb0 | wb1 | truncated
        row_store4_push(B, r + 4 * l, x0, x1, x2, x3);
      } else {
        if (l < 3) { row_store(B, r + l, e); row_store(B, r + 7 + l, vbody); row_store(B, r + 10 + l, wbody); }
        row_store(B, r + 3 + l, q);
        if (l == 0) {  // write_step_row_tail on the values loaded at the top
          row_store(B, r + 13, tail_reward);
          row_store(B, r + 14, tail_crashed ? 1.0f : 0.0f);
          row_store(B, r + 15, tail_truncated ? 1.0f : 0.0f);
        }
      }
    }
  }
  step_rows_signal(B);
}
__global__ void __launch_bounds__(64, 1) k_reset_masked_quad_obs(AgxRobotParams P, AgxEnvBuffers B, int n, AgxResetArgs R,
                                                                 const float *__restrict__ target, float *__restrict__ obs) {
  reset_masked_quad_obs_body<false>(P, B, n, R, target, obs);
}
__global__ void __launch_bounds__(64, 1) k_reset_masked_quad_obs_host_draws(AgxRobotParams P, AgxEnvBuffers B, int n, AgxResetArgs R,
                                                                            const float *__restrict__ target,
                                                                            float *__restrict__ obs) {
  reset_masked_quad_obs_body<true>(P, B, n, R, target, obs);
}

// AssetManager.reset_idx (asset_manager.py:51-71) + the half-obstacle resample (env_manager.py:283-295)
__global__ void __launch_bounds__(256) k_reset_assets(AgxEnvBuffers B, int n, int K, AgxResetArgs R, const float *__restrict__ u1,
                                                       const float *__restrict__ u2, const float *__restrict__ u_sel,
                                                       const float *__restrict__ min_ratio, const float *__restrict__ max_ratio,
                                                       int num_obstacles, int nk, float *__restrict__ asset_state) {
  // env on grid.x (2^31 blocks), asset chunk on grid.y: HIP caps grid.y at 65535, the env count has no such bound
  const int env = blockIdx.x;
  const int a = blockIdx.y * blockDim.x + threadIdx.x;
  if (a >= K) return;
  if (B.reset_flag[B.flag_parity] == 0 || B.reset_mask[env] == 0) return;
  reset_asset_one(B, R, env, a, K, u1, u2, u_sel, min_ratio, max_ratio, num_obstacles, nk, asset_state);
}
}  // namespace agx

static int check_reset(const AgxRobotParams *P, const AgxEnvBuffers *B, int n, const AgxResetArgs *R) {
  if (int e = check_common(P, B, n)) return e;
  AGX_REQUIRE(P && R && B->reset_flag && B->reset_mask && B->bounds_min && B->bounds_max, "null argument");
  const bool rov = (B->launch_flags & AGX_LAUNCH_ROV) != 0;  // no motor draws: u_tau_inc .. u_kT may be NULL
  if (R->u_state) {
    AGX_REQUIRE(R->u_bounds_lo && R->u_bounds_hi && (rov || (R->u_tau_inc && R->u_tau_dec && R->u_thrust)), "null reset input");
    AGX_REQUIRE(rov || !P->use_rps || R->u_kT, "null u_kT with use_rps");
    AGX_REQUIRE(!R->randomize_gains || R->u_gains, "null u_gains with randomize_gains");
  } else {
    AGX_REQUIRE(B->episode_count, "device RNG needs buf->episode_count");
  }
  AGX_REQUIRE(!R->randomize_gains || B->gains, "null gains with randomize_gains");
  return AGX_OK;
}

extern "C" int agx_reset_masked(const AgxRobotParams *P, const AgxEnvBuffers *B, int n, const AgxResetArgs *R,
                                void *stream) {
  if (int e = check_reset(P, B, n, R)) return e;
  const int block = pick_block(n);
  if (B->launch_flags & AGX_LAUNCH_ROV) {
    if (int e = check_rov(P, "agx_reset_masked")) return e;
    hipLaunchKernelGGL((k_reset_masked_rov<false>), dim3(blocks_for(n, block)), dim3(block), 0, (hipStream_t)stream, *P, *B, n, *R,
                       nullptr, nullptr);
    return check_launch("agx_reset_masked");
  }
  AGX_DISPATCH_M(P->num_motors, hipLaunchKernelGGL((k_reset_masked<kM, false>), dim3(blocks_for(n, block)), dim3(block), 0,
                                                   (hipStream_t)stream, *P, *B, n, *R, nullptr, nullptr));
  return check_launch("agx_reset_masked");
}

extern "C" int agx_nav_robot_side(const AgxRobotParams *P, const AgxEnvBuffers *B, int n, const AgxResetArgs *R,
                                  const AgxNavRobotSideArgs *A, void *stream) {
  if (int e = check_reset(P, B, n, R)) return e;
  AGX_REQUIRE(A, "null AgxNavRobotSideArgs");
  AGX_REQUIRE((B->launch_flags & AGX_LAUNCH_ROV) == 0, "AGX_LAUNCH_ROV: agx_nav_robot_side resets multirotors only (use agx_reset_masked)");
  AGX_REQUIRE(R->u_state == nullptr, "agx_nav_robot_side draws with the device generator only (sync-free mode)");
  AGX_REQUIRE(A->num_sensors >= 0 && (A->num_sensors == 0 || (A->local_pos && A->local_quat && A->sensor_pos && A->sensor_quat)),
              "sensor buffers missing");
  AGX_REQUIRE(!A->reset_target || (A->target && B->bounds_min && B->bounds_max), "target part needs target and the env bounds");
  AGX_REQUIRE((!A->reset_target && !(A->num_sensors && A->randomize_mount)) || B->episode_count, "device RNG needs buf->episode_count");
  AGX_REQUIRE(!A->zero_prev_actions || B->prev_actions, "zero_prev_actions needs buf->prev_actions");
  AGX_DISPATCH_M(P->num_motors, hipLaunchKernelGGL((k_nav_robot_side<kM>), dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream,
                                                   *P, *B, n, *R, *A));
  return check_launch("agx_nav_robot_side");
}

extern "C" int agx_post_step_position(const AgxRobotParams *P, const AgxEnvBuffers *B, int n, const AgxResetArgs *R,
                                      const float *target, float *obs, void *stream) {
  if (int e = check_reset(P, B, n, R)) return e;
  AGX_REQUIRE(target && obs && B->state && B->derived, "null buffer");
  const int block = pick_block(n);
  if (B->launch_flags & AGX_LAUNCH_ROV) {  // (never the lane-quad kernel)
    if (int e = check_rov(P, "agx_post_step_position")) return e;
    hipLaunchKernelGGL((k_reset_masked_rov<true>), dim3(blocks_for(n, block)), dim3(block), 0, (hipStream_t)stream, *P, *B, n, *R,
                       target, obs);
    return check_launch("agx_post_step_position");
  }
  if (block == 64 && P->num_motors == 4 && option_env_step_quad()) {
    if (R->u_state)
      hipLaunchKernelGGL(k_reset_masked_quad_obs_host_draws, dim3(blocks_for(n, 16)), dim3(64), 0, (hipStream_t)stream, *P, *B, n, *R,
                         target, obs);
    else
      hipLaunchKernelGGL(k_reset_masked_quad_obs, dim3(blocks_for(n, 16)), dim3(64), 0, (hipStream_t)stream, *P, *B, n, *R, target, obs);
    return check_launch("agx_post_step_position");
  }
  AGX_DISPATCH_M(P->num_motors, hipLaunchKernelGGL((k_reset_masked<kM, true>), dim3(blocks_for(n, block)), dim3(block), 0,
                                                   (hipStream_t)stream, *P, *B, n, *R, target, obs));
  return check_launch("agx_post_step_position");
}

extern "C" int agx_reset_assets(const AgxEnvBuffers *B, int n, int K, const AgxResetArgs *R, const float *u1, const float *u2,
                                const float *u_sel, const float *min_ratio, const float *max_ratio, int num_obstacles,
                                int num_keep, float *asset_state, void *stream) {
  if (int e = check_common(nullptr, B, n)) return e;
  AGX_REQUIRE(K > 0 && R && min_ratio && max_ratio && asset_state && B->reset_flag && B->reset_mask, "bad arguments");
  AGX_REQUIRE((u1 && u2 && u_sel && R->u_state) || (!u1 && !u2 && !u_sel && !R->u_state),
              "asset draws and robot draws must both come from tensors or both from the device generator");
  AGX_REQUIRE(u1 || B->episode_count, "device RNG needs buf->episode_count");
  AGX_REQUIRE(blocks_for(K, 64) <= 65535, "too many assets per env");
  dim3 grid(n, blocks_for(K, 64));
  hipLaunchKernelGGL(k_reset_assets, grid, dim3(64), 0, (hipStream_t)stream, *B, n, K, *R, u1, u2, u_sel, min_ratio, max_ratio,
                     num_obstacles, num_keep, asset_state);
  return check_launch("agx_reset_assets");
}
