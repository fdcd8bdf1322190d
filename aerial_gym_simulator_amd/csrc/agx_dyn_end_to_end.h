#pragma once
// Task side of the end-to-end motor-command set-point task (position_setpoint_task_sim2real_end_to_end.py of the reference, tinyprop +
// no_control): the action rescale in front of sim_env.step, compute_rewards_and_crashes + compute_reward + the truncation test, the
// noisy 15-D process_obs_for_task with its 6-D rotation, and the step's tail (masked reset + observation + prev_actions /
// prev_pos_error) as ONE launch.  One lane per env; env tensors component-major ([C][N]), the task's action tensors row-major
// ([N][4], one 16-byte access), observation rows of 15 floats (4-byte aligned: scalar stores).
// Part of the one translation unit agx_dynamics.hip, which alone includes it, behind agx_dyn_reset.h: the fused tail calls
// reset_and_observe.  Contraction is off there: every + - * / sqrt is one IEEE operation in the reference's order; exp / sin / cos /
// atan2 / asin are the correctly rounded ones of agx_device_math.h; torch.norm, torch.cross and quat_rotate are the forms restated there.

namespace agx {

// torch.clamp(x, -1, 1): a NaN stays a NaN
AGX_DEV float e2e_clamp1(float x) { return x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x); }

// step() up to sim_env.step (:164-168): task_config.process_actions_for_task (config :28-33), clamp(a, -1, 1) * (max - min) / 2 +
// (max + min) / 2 per column into the task's own tensor (the caller's is neither kept nor changed), and prev_position[:] = robot_position
__global__ void __launch_bounds__(256) k_e2e_pre_step(AgxEnvBuffers B, int n, const float *__restrict__ actions_in,
                                                       AgxEndToEndLimits L, float *__restrict__ actions, float *__restrict__ prev_position) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 a = *reinterpret_cast<const float4 *>(actions_in + (size_t)i * 4);
  float4 o;
  o.x = (e2e_clamp1(a.x) * (L.max[0] - L.min[0])) / 2.0f + (L.max[0] + L.min[0]) / 2.0f;
  o.y = (e2e_clamp1(a.y) * (L.max[1] - L.min[1])) / 2.0f + (L.max[1] + L.min[1]) / 2.0f;
  o.z = (e2e_clamp1(a.z) * (L.max[2] - L.min[2])) / 2.0f + (L.max[2] + L.min[2]) / 2.0f;
  o.w = (e2e_clamp1(a.w) * (L.max[3] - L.min[3])) / 2.0f + (L.max[3] + L.min[3]) / 2.0f;
  *reinterpret_cast<float4 *>(actions + (size_t)i * 4) = o;
  AGX_TASK_AT(prev_position, 0) = AGX_TASK_AT(B.state, 0);
  AGX_TASK_AT(prev_position, 1) = AGX_TASK_AT(B.state, 1);
  AGX_TASK_AT(prev_position, 2) = AGX_TASK_AT(B.state, 2);
}

// compute_reward (:267-309), before the crash line
AGX_DEV float e2e_reward_value(const AgxEndToEndReward &K, V3 err, float dist, float prev_dist, Q4 q, V3 v, V3 w, float4 a, float4 pa) {
  const float ez = err.z * K.z_error_weight;  // pos_error[:, 2] *= 11 AFTER the two distances were taken (:278-282)
  const float pos_reward = sum3(gain_exp(err.x, K.pos_gain[0], K.pos_exp[0]), gain_exp(err.y, K.pos_gain[0], K.pos_exp[0]),
                                gain_exp(ez, K.pos_gain[0], K.pos_exp[0])) +
                           sum3(gain_exp(err.x, K.pos_gain[1], K.pos_exp[1]), gain_exp(err.y, K.pos_gain[1], K.pos_exp[1]),
                                gain_exp(ez, K.pos_gain[1], K.pos_exp[1]));
  const V3 ups = quat_rotate(q, V3{0.0f, 0.0f, 1.0f});   // quat_axis(q, 2)
  const float upright_reward = gain_exp(1.0f - ups.z, K.upright_gain, K.upright_exp);
  const V3 forw = quat_rotate(q, V3{1.0f, 0.0f, 0.0f});  // quat_axis(q, 0)
  const float alignment_reward = gain_exp(1.0f - forw.x, K.alignment_gain, K.alignment_exp);
  const float angvel_reward = sum3(gain_exp(w.x, K.angvel_gain, K.angvel_exp), gain_exp(w.y, K.angvel_gain, K.angvel_exp),
                                   gain_exp(w.z, K.angvel_gain, K.angvel_exp));
  const float vel_reward = sum3(gain_exp(v.x, K.vel_gain, K.vel_exp), gain_exp(v.y, K.vel_gain, K.vel_exp),
                                gain_exp(v.z, K.vel_gain, K.vel_exp));
  const float action_cost = sum4(gain_exp_penalty(a.x - K.hover_thrust, K.action_gain, K.action_exp),
                                 gain_exp_penalty(a.y - K.hover_thrust, K.action_gain, K.action_exp),
                                 gain_exp_penalty(a.z - K.hover_thrust, K.action_gain, K.action_exp),
                                 gain_exp_penalty(a.w - K.hover_thrust, K.action_gain, K.action_exp));
  const float closer = prev_dist - dist;
  const float towards_goal_reward = (closer >= 0.0f) ? K.closer_gain * closer : K.farther_gain * closer;
  const float diff_penalty = sum4(gain_exp_penalty(a.x - pa.x, K.diff_gain, K.diff_exp), gain_exp_penalty(a.y - pa.y, K.diff_gain, K.diff_exp),
                                  gain_exp_penalty(a.z - pa.z, K.diff_gain, K.diff_exp), gain_exp_penalty(a.w - pa.w, K.diff_gain, K.diff_exp));
  return towards_goal_reward + (pos_reward * (((alignment_reward + vel_reward) + angvel_reward) + diff_penalty) +
                                ((((angvel_reward + vel_reward) + upright_reward) + pos_reward) + action_cost)) / K.divisor;  // :305
}

// compute_rewards_and_crashes (:232-252) + compute_reward + `truncations = sim_steps > episode_len` (:176-178) + the reset set of
// EnvManager.reset_terminated_and_truncated_envs, left exactly as k_sim2real_reward leaves it.  robot_linvel is the world-frame
// velocity of the state; robot_body_angvel the dict's tensor as EnvManager.step left it (B.derived: one sub-step stale).
__global__ void __launch_bounds__(256) k_e2e_reward(AgxEnvBuffers B, int n, const float *__restrict__ target,
                                                     const float *__restrict__ actions, const float *__restrict__ prev_actions,
                                                     const float *__restrict__ prev_pos_error, AgxEndToEndReward K, float crash_dist,
                                                     int episode_len, int reset_on_collision, float *__restrict__ reward) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool reset = false;
  if (i < n) {
    const V3 p = V3{AGX_TASK_AT(B.state, 0), AGX_TASK_AT(B.state, 1), AGX_TASK_AT(B.state, 2)};
    const Q4 q = Q4{AGX_TASK_AT(B.state, 3), AGX_TASK_AT(B.state, 4), AGX_TASK_AT(B.state, 5), AGX_TASK_AT(B.state, 6)};
    const V3 v = V3{AGX_TASK_AT(B.state, 7), AGX_TASK_AT(B.state, 8), AGX_TASK_AT(B.state, 9)};
    const V3 w = V3{AGX_TASK_AT(B.derived, 13), AGX_TASK_AT(B.derived, 14), AGX_TASK_AT(B.derived, 15)};
    const V3 err = V3{AGX_TASK_AT(target, 0), AGX_TASK_AT(target, 1), AGX_TASK_AT(target, 2)} - p;
    const V3 perr = V3{AGX_TASK_AT(prev_pos_error, 0), AGX_TASK_AT(prev_pos_error, 1), AGX_TASK_AT(prev_pos_error, 2)};
    const float4 a = *reinterpret_cast<const float4 *>(actions + (size_t)i * 4);
    const float4 pa = *reinterpret_cast<const float4 *>(prev_actions + (size_t)i * 4);
    const float dist = norm(err);
    reward[i] = e2e_reward_value(K, err, dist, norm(perr), q, v, w, a, pa);  // (not replaced on a crash)
    bool crash = B.crashes[i] != 0;
    if (dist > crash_dist) crash = true;  // :307
    B.crashes[i] = crash ? 1 : 0;
    reset = reset_set_truncate(B, i, crash, episode_len, reset_on_collision);
  }
  reset_flag_raise(B, reset);
}

// ---- the observation ----------------------------------------------------------------------------------------------------
// The twelve standard normals of one env's observation, in the reference's draw order (position, orientation, linear velocity,
// body angular velocity: :207-218), three each.  Host: z [4][N][3].  Device generator: stream RNG_E2E_OBS_NOISE of
// (seed; GLOBAL env index, env step), blocks 0-2 -> 12 uniforms -> 6 pairs.
struct E2ENoise {
  float z[12];
};
AGX_DEV E2ENoise e2e_noise(const AgxEnvBuffers &B, int n, int i, const float *__restrict__ z) {
  E2ENoise N;
  if (z) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int c = 0; c < 3; ++c) N.z[3 * g + c] = z[((size_t)g * (size_t)n + (size_t)i) * 3 + c];
    }
  } else {
    float u[12];
    rng_fill<12>(B.rng_seed, B.env_index_base + i, agx::step_index(B), RNG_E2E_OBS_NOISE, u);
#pragma unroll
    for (int j = 0; j < 6; ++j) normal_pair(u[2 * j], u[2 * j + 1], N.z[2 * j], N.z[2 * j + 1]);
  }
  return N;
}

constexpr float kE2EStdPos = 0.001f, kE2EStdLinvel = 0.002f, kE2EStdAngvel = 0.001f;
constexpr float kE2EStdEuler = (float)(3.141592653589793 / 1032);  // std = torch.pi / 1032: a double, rounded to float once

// process_obs_for_task (:204-225) of one env: position error | rotation_6d | world linear velocity | body angular velocity, each
// with its noise.  The rotation goes quaternion -> matrix -> Euler "ZYX" -> + noise -> matrix -> first two rows, through the four
// pytorch3d functions (transforms/rotation_conversions.py: quaternion_to_matrix, matrix_to_euler_angles + _angle_from_tan,
// euler_angles_to_matrix + _axis_angle_rotation, matrix_to_rotation_6d).  No clamp in front of asin, as there: an argument above 1
// in magnitude gives NaN.
AGX_DEV void e2e_write_obs(V3 err, Q4 q, V3 v, V3 w, const E2ENoise &N, float *__restrict__ of) {
  of[0] = err.x + N.z[0] * kE2EStdPos; of[1] = err.y + N.z[1] * kE2EStdPos; of[2] = err.z + N.z[2] * kE2EStdPos;
  // quaternion_to_matrix of (r, i, j, k) = (w, x, y, z): only the entries the Euler angles read
  const float r = q.w, qi = q.x, qj = q.y, qk = q.z;
  const float two_s = 2.0f / (((r * r + qi * qi) + qj * qj) + qk * qk);
  const float m00 = 1.0f - two_s * (qj * qj + qk * qk);
  const float m10 = two_s * (qi * qj + qk * r);
  const float m20 = two_s * (qi * qk - qj * r);
  const float m21 = two_s * (qj * qk + qi * r);
  const float m22 = 1.0f - two_s * (qi * qi + qj * qj);
  // matrix_to_euler_angles(., "ZYX") = (atan2(m10, m00), asin(-m20), atan2(m21, m22)); [:, [2, 1, 0]] = roll, pitch, yaw
  const float roll = atan2_cw(m21, m22) + N.z[3] * kE2EStdEuler;
  const float pitch = asin_cw(-m20) + N.z[4] * kE2EStdEuler;
  const float yaw = atan2_cw(m10, m00) + N.z[5] * kE2EStdEuler;
  // euler_angles_to_matrix((yaw, pitch, roll), "ZYX") = (Rz Ry) Rx, rows 0 and 1.  torch.matmul of 3 x 3 factors sums each entry's three
  // rounded products left to right (no fused multiply-add); with the zeros and ones of the factors Rz Ry has one product per entry,
  // and ((Rz Ry) Rx)[i][1] = A_i1 cx + A_i2 sx, [i][2] = A_i1 (-sx) + A_i2 cx
  float sz, cz, sy, cy, sx, cx;
  sincos_bounded(yaw, sz, cz);
  sincos_bounded(pitch, sy, cy);
  sincos_bounded(roll, sx, cx);
  const float a00 = cz * cy, a01 = -sz, a02 = cz * sy;
  const float a10 = sz * cy, a11 = cz, a12 = sz * sy;
  of[3] = a00;
  of[4] = a01 * cx + a02 * sx;
  of[5] = a01 * -sx + a02 * cx;
  of[6] = a10;
  of[7] = a11 * cx + a12 * sx;
  of[8] = a11 * -sx + a12 * cx;
  of[9] = v.x + N.z[6] * kE2EStdLinvel; of[10] = v.y + N.z[7] * kE2EStdLinvel; of[11] = v.z + N.z[8] * kE2EStdLinvel;
  of[12] = w.x + N.z[9] * kE2EStdAngvel; of[13] = w.y + N.z[10] * kE2EStdAngvel; of[14] = w.z + N.z[11] * kE2EStdAngvel;
}
// ... on the tensors as they stand in memory
AGX_DEV void e2e_observe(const AgxEnvBuffers &B, int n, int i, V3 tgt, const float *__restrict__ z, float *__restrict__ obs) {
  const V3 p = task_vec(B.state, 0, n, i);
  const Q4 q = task_quat(B.state, 3, n, i);
  const V3 v = task_vec(B.state, 7, n, i);
  const V3 w = task_vec(B.derived, 13, n, i);
  e2e_write_obs(tgt - p, q, v, w, e2e_noise(B, n, i, z), obs + (size_t)i * 15);
}

__global__ void __launch_bounds__(256) k_e2e_obs(AgxEnvBuffers B, int n, const float *__restrict__ target, const float *__restrict__ z,
                                                  float *__restrict__ obs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  e2e_observe(B, n, i, task_vec(target, 0, n, i), z, obs);
}

// the normals themselves, [4][N][3]: what k_e2e_obs with z == NULL scales and adds
__global__ void __launch_bounds__(256) k_e2e_noise(AgxEnvBuffers B, int n, float *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const E2ENoise N = e2e_noise(B, n, i, nullptr);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[((size_t)g * (size_t)n + (size_t)i) * 3 + c] = N.z[3 * g + c];
  }
}

// The tail of step() in one launch (:180-190 with return_state_before_reset False): the masked reset exactly as k_reset_masked<M, false>
// performs it (the NEXT step's flag cleared; some env resets => the derived tensors of EVERY env are refreshed), the task's own
// reset_idx (:146-153: some env resets => the target of EVERY env goes back to zero), then the observation of the post-reset tensors,
// then prev_actions <- actions and prev_pos_error <- target - robot_position (post-reset).  What the observation and the bookkeeping
// read was written, if at all, by the SAME lane in reset_and_observe: program order is all the ordering it takes.
template <int M>
__global__ void __launch_bounds__(256) k_e2e_post_step(AgxRobotParams P, AgxEnvBuffers B, int n, AgxResetArgs R, float *__restrict__ target,
                                                        const float *__restrict__ z, float *__restrict__ obs,
                                                        const float *__restrict__ actions, float *__restrict__ prev_actions,
                                                        float *__restrict__ prev_pos_error) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) B.reset_flag[B.flag_parity ^ 1] = 0;  // the NEXT step's flag; nobody reads or writes it now
  const bool valid = i < n;
  EnvState s{};
  V3 tgt{};
  int mask = 0, ep = 0;
  float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (valid) {
    s = load_state(B.state, n, i);
    tgt = task_vec(target, 0, n, i);
    mask = B.reset_mask[i];
    if (B.episode_count) ep = B.episode_count[i];
    a = *reinterpret_cast<const float4 *>(actions + (size_t)i * 4);
  }
  const int flag = B.reset_flag[B.flag_parity];  // (one word: the branch is taken by whole waves)
  const bool any = flag != 0, mine = mask != 0;
  reset_and_observe<M, false>(P, B, n, R, i, valid, any, mine && any, ep, V3{}, nullptr, s, Derived{});
  if (!valid) return;
  if (any) {
    tgt = V3{0.0f, 0.0f, 0.0f};
    AGX_TASK_AT(target, 0) = 0.0f; AGX_TASK_AT(target, 1) = 0.0f; AGX_TASK_AT(target, 2) = 0.0f;
  }
  __atomic_signal_fence(__ATOMIC_SEQ_CST);  // the loads below stay behind the reset's stores
  e2e_observe(B, n, i, tgt, z, obs);
  *reinterpret_cast<float4 *>(prev_actions + (size_t)i * 4) = a;
  AGX_TASK_AT(prev_pos_error, 0) = tgt.x - AGX_TASK_AT(B.state, 0);
  AGX_TASK_AT(prev_pos_error, 1) = tgt.y - AGX_TASK_AT(B.state, 1);
  AGX_TASK_AT(prev_pos_error, 2) = tgt.z - AGX_TASK_AT(B.state, 2);
}

}  // namespace agx

extern "C" int agx_end_to_end_pre_step(const AgxEnvBuffers *B, int n, const float *actions_in, const AgxEndToEndLimits *limits,
                                       float *actions, float *prev_position, void *stream) {
  if (int e = task_check("agx_end_to_end_pre_step", B, n)) return e;
  AGX_REQUIRE(actions_in && limits && actions && prev_position, "agx_end_to_end_pre_step: null argument");
  AGX_REQUIRE(aligned16(actions_in) && aligned16(actions), "agx_end_to_end_pre_step: the [N][4] action tensors must be 16-byte aligned");
  const int block = pick_block(n);
  hipLaunchKernelGGL(k_e2e_pre_step, dim3(blocks_for(n, block)), dim3(block), 0, (hipStream_t)stream, *B, n, actions_in, *limits, actions,
                     prev_position);
  return check_launch("agx_end_to_end_pre_step");
}

extern "C" int agx_end_to_end_reward(const AgxEnvBuffers *B, int n, const float *target, const float *actions, const float *prev_actions,
                                     const float *prev_pos_error, const AgxEndToEndReward *constants, float crash_dist, int episode_len,
                                     int reset_on_collision, float *reward, void *stream) {
  if (int e = task_check("agx_end_to_end_reward", B, n, true)) return e;
  AGX_REQUIRE(target && actions && prev_actions && prev_pos_error && constants && reward && B->derived && B->crashes && B->truncations &&
                  B->sim_steps && B->reset_mask && B->reset_flag,
              "agx_end_to_end_reward: null argument");
  AGX_REQUIRE(aligned16(actions) && aligned16(prev_actions), "agx_end_to_end_reward: the [N][4] action tensors must be 16-byte aligned");
  const int block = pick_block(n);
  hipLaunchKernelGGL(k_e2e_reward, dim3(blocks_for(n, block)), dim3(block), 0, (hipStream_t)stream, *B, n, target, actions, prev_actions,
                     prev_pos_error, *constants, crash_dist, episode_len, reset_on_collision, reward);
  return check_launch("agx_end_to_end_reward");
}

extern "C" int agx_end_to_end_obs(const AgxEnvBuffers *B, int n, const float *target, const float *noise, float *obs, void *stream) {
  if (int e = task_check("agx_end_to_end_obs", B, n)) return e;
  AGX_REQUIRE(target && obs && B->derived, "agx_end_to_end_obs: null argument");
  AGX_REQUIRE(!B->step_rows[0] && !B->step_rows[1], "agx_end_to_end_obs: exchange rows (step_rows) are not written for the 15-D observation");
  const int block = pick_block(n);
  hipLaunchKernelGGL(k_e2e_obs, dim3(blocks_for(n, block)), dim3(block), 0, (hipStream_t)stream, *B, n, target, noise, obs);
  return check_launch("agx_end_to_end_obs");
}

extern "C" int agx_end_to_end_noise(const AgxEnvBuffers *B, int n, float *noise_out, void *stream) {
  AGX_REQUIRE(B != nullptr && n > 0 && n <= (1 << 26) && noise_out, "agx_end_to_end_noise: bad arguments");
  const int block = pick_block(n);
  hipLaunchKernelGGL(k_e2e_noise, dim3(blocks_for(n, block)), dim3(block), 0, (hipStream_t)stream, *B, n, noise_out);
  return check_launch("agx_end_to_end_noise");
}

extern "C" int agx_post_step_end_to_end(const AgxRobotParams *P, const AgxEnvBuffers *B, int n, const AgxResetArgs *R, float *target,
                                        const float *noise, float *obs, const float *actions, float *prev_actions, float *prev_pos_error,
                                        void *stream) {
  if (int e = check_reset(P, B, n, R)) return e;
  AGX_REQUIRE(target && obs && actions && prev_actions && prev_pos_error && B->state && B->derived, "agx_post_step_end_to_end: null buffer");
  AGX_REQUIRE(!B->step_rows[0] && !B->step_rows[1], "agx_post_step_end_to_end: exchange rows (step_rows) are not written for the 15-D observation");
  AGX_REQUIRE((B->launch_flags & AGX_LAUNCH_LEAN) == 0, "agx_post_step_end_to_end: the observation reads robot_body_angvel, which the lean step does not maintain");
  AGX_REQUIRE((B->launch_flags & AGX_LAUNCH_ROV) == 0, "AGX_LAUNCH_ROV: agx_post_step_end_to_end resets multirotors only (use agx_reset_masked)");
  AGX_REQUIRE(aligned16(actions) && aligned16(prev_actions), "agx_post_step_end_to_end: the [N][4] action tensors must be 16-byte aligned");
  const int block = pick_block(n);
  AGX_DISPATCH_M(P->num_motors, hipLaunchKernelGGL((k_e2e_post_step<kM>), dim3(blocks_for(n, block)), dim3(block), 0, (hipStream_t)stream, *P,
                                                   *B, n, *R, target, noise, obs, actions, prev_actions, prev_pos_error));
  return check_launch("agx_post_step_end_to_end");
}
