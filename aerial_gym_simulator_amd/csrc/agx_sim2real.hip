// Task-side kernels of the two lmf2 sim2real set-point tasks (position_setpoint_task_sim2real.py and
// position_setpoint_task_acceleration_sim2real.py of the reference): what their step() does before sim_env.step, their
// compute_rewards_and_crashes + compute_reward + truncation test, and their noisy 17-D process_obs_for_task.  One lane per env;
// the env's tensors are read component-major ([C][N]), the task's own action tensors row-major ([N][4]: the tensor the
// caller hands to task.step() is one of them).  Every + - * / sqrt is one IEEE operation in the reference's order (the
// library is compiled with -ffp-contract=off); exp / sin / cos / atan2 / asin are the correctly rounded ones of
// agx_device_math.h; torch.norm, torch.cross and the quat_* helpers are the forms restated there.
#include "agx_task_parts.h"

namespace agx {

// step() up to sim_env.step (velocity :157-161, acceleration :161-170), in the reference's order: prev_actions <- what
// task.actions reads NOW (`before`: the tensor of the previous call, which the caller may have overwritten since -- it may be
// `actions` itself), prev_dist on the pre-step position, then for the acceleration task the previous action in the vehicle
// frame (quat_rotate with the FULL orientation, as written there) and the incoming action's first three components doubled
// in the caller's tensor.  A lane touches only its own row: `before` aliasing `actions` is read before it is written.
__global__ void __launch_bounds__(256) k_sim2real_pre_step(int kind, AgxEnvBuffers B, int n, const float *__restrict__ target,
                                                            const float *before, float *actions, float *__restrict__ prev_actions,
                                                            float *__restrict__ prev_dist, float *__restrict__ prev_actions_vehicle) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 pa = *reinterpret_cast<const float4 *>(before + (size_t)i * 4);
  *reinterpret_cast<float4 *>(prev_actions + (size_t)i * 4) = pa;
  const V3 d = task_vec(target, 0, n, i) - task_vec(B.state, 0, n, i);
  prev_dist[i] = norm(d);
  if (kind == AGX_SIM2REAL_ACCELERATION) {
    const V3 r = quat_rotate(task_quat(B.state, 3, n, i), V3{pa.x, pa.y, pa.z});
    *reinterpret_cast<float4 *>(prev_actions_vehicle + (size_t)i * 4) = make_float4(r.x, r.y, r.z, pa.w);
    float4 a = *reinterpret_cast<const float4 *>(actions + (size_t)i * 4);
    a.x = 2.0f * a.x; a.y = 2.0f * a.y; a.z = 2.0f * a.z;
    *reinterpret_cast<float4 *>(actions + (size_t)i * 4) = a;
  }
}

// compute_reward of the velocity task (position_setpoint_task_sim2real.py:286-339)
AGX_DEV float s2r_reward_velocity(float dist, float prev_dist, float yaw_error, float speed, float4 a, float4 p) {
  const float pos_reward = (gain_exp(dist, 2.0f, 1.0f) + gain_exp(dist, 3.0f, 10.0f)) + gain_abs_exp(dist, 3.0f, 50.0f);
  const float speed_reward = gain_exp(speed, 1.0f, 3.0f);
  const float dist_reward = (20.0f - dist) / 40.0f;
  const float action_penalty = sum4(gain_abs_exp_penalty(a.x, 0.2f, 4.0f), gain_abs_exp_penalty(a.y, 0.2f, 4.0f),
                                    gain_abs_exp_penalty(a.z, 0.2f, 4.0f), gain_abs_exp_penalty(a.w, 0.2f, 4.0f));
  const float diff_penalty = sum4(gain_abs_exp_penalty(a.x - p.x, 0.3f, 6.0f), gain_abs_exp_penalty(a.y - p.y, 0.3f, 6.0f),
                                  gain_abs_exp_penalty(a.z - p.z, 0.3f, 6.0f), gain_abs_exp_penalty(a.w - p.w, 0.3f, 6.0f));
  const float closer_reward = 400.0f * (prev_dist - dist);
  const float yaw_reward = gain_abs_exp(yaw_error, 2.0f, 3.0f);
  float total = (pos_reward + dist_reward) + pos_reward * ((speed_reward + action_penalty) + closer_reward / 10.0f);
  total = total + action_penalty;
  total = total + diff_penalty;
  total = total + closer_reward;
  total = total + yaw_reward;
  return 1.0f * total;
}

// compute_reward of the acceleration task (position_setpoint_task_acceleration_sim2real.py:300-356): other constants, the
// two-sided closer_reward, actions in the vehicle frame
AGX_DEV float s2r_reward_acceleration(float dist, float prev_dist, float yaw_error, float speed, float4 a, float4 p) {
  const float pos_reward = (gain_exp(dist, 2.0f, 1.0f) + gain_exp(dist, 3.0f, 10.0f)) + gain_abs_exp(dist, 3.0f, 50.0f);
  const float close_pos_reward = gain_exp(dist, 2.0f, 1.0f);
  const float speed_reward = gain_exp(speed, 2.0f, 2.5f);
  const float action_penalty = sum4(gain_abs_exp_penalty(a.x, 0.3f, 4.0f), gain_abs_exp_penalty(a.y, 0.3f, 4.0f),
                                    gain_abs_exp_penalty(a.z, 0.3f, 4.0f), gain_abs_exp_penalty(a.w, 0.3f, 4.0f));
  const float diff_penalty = sum4(gain_abs_exp_penalty(a.x - p.x, 0.4f, 6.0f), gain_abs_exp_penalty(a.y - p.y, 0.4f, 6.0f),
                                  gain_abs_exp_penalty(a.z - p.z, 0.4f, 6.0f), gain_abs_exp_penalty(a.w - p.w, 0.4f, 6.0f));
  const float closer = prev_dist - dist;
  const float closer_reward = (dist < prev_dist) ? 400.0f * closer : 1200.0f * closer;
  const float yaw_reward = gain_abs_exp(yaw_error, 3.0f, 5.0f);
  float total = pos_reward + pos_reward * ((closer_reward / 9.0f + action_penalty / 3.0f) + speed_reward / 1.5f);
  total = total + action_penalty;
  total = total + diff_penalty;
  total = total + closer_reward;
  total = total + yaw_reward;
  total = total + close_pos_reward;
  total = total + speed_reward * 0.2f;
  return 1.0f * total;
}

// compute_rewards_and_crashes (:230-259 / :239-273) + `truncations = sim_steps > episode_len` (:180-182 / :189-191) + the reset
// set of EnvManager.reset_terminated_and_truncated_envs, left exactly as k_reward_position leaves it.  The body-frame
// velocity and the vehicle-frame quaternion are the dict's tensors as EnvManager.step left them (B.derived).
__global__ void __launch_bounds__(256) k_sim2real_reward(int kind, AgxEnvBuffers B, int n, const float *__restrict__ target,
                                                          const float *__restrict__ actions, const float *__restrict__ prev_actions,
                                                          const float *__restrict__ prev_dist, float *__restrict__ actions_vehicle,
                                                          const float *__restrict__ prev_actions_vehicle, int episode_len,
                                                          int reset_on_collision, float *__restrict__ reward) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool reset = false;
  if (i < n) {
    const V3 p = task_vec(B.state, 0, n, i);
    const Q4 q = task_quat(B.state, 3, n, i);
    const Q4 qveh = task_quat(B.derived, 3, n, i);
    const V3 vbody = task_vec(B.derived, 10, n, i);
    const V3 err = task_vec(target, 0, n, i) - p;
    const float4 a = *reinterpret_cast<const float4 *>(actions + (size_t)i * 4);
    const float yaw_error = 0.0f - ssa(yaw_0_2pi(q));
    const float speed = norm(vbody);
    const float pd = prev_dist[i];
    float total, dist;
    if (kind == AGX_SIM2REAL_ACCELERATION) {
      dist = norm(quat_apply(conj(q), err));
      const V3 r = quat_rotate(qveh, V3{a.x, a.y, a.z});
      const float4 av = make_float4(r.x, r.y, r.z, a.w);
      *reinterpret_cast<float4 *>(actions_vehicle + (size_t)i * 4) = av;
      const float4 pv = *reinterpret_cast<const float4 *>(prev_actions_vehicle + (size_t)i * 4);
      total = s2r_reward_acceleration(dist, pd, yaw_error, speed, av, pv);
    } else {
      dist = norm(quat_apply(conj(qveh), err));
      const float4 pa = *reinterpret_cast<const float4 *>(prev_actions + (size_t)i * 4);
      total = s2r_reward_velocity(dist, pd, yaw_error, speed, a, pa);
    }
    bool crash = B.crashes[i] != 0;
    if (dist > 10.0f) crash = true;
    if (crash) total = -50.0f;
    reward[i] = total;
    B.crashes[i] = crash ? 1 : 0;
    reset = reset_set_truncate(B, i, crash, episode_len, reset_on_collision);
  }
  reset_flag_raise(B, reset);
}

// process_obs_for_task (:202-228 / :211-237, the same in both tasks): the state quaternion times sign(w), STORED BACK into
// the robot state like the reference's in-place write (torch.sign is 0 at +-0 and at NaN: the quaternion becomes zeros
// there); Euler angles -> ssa -> + 0.02 z_e -> quaternion; position error + 0.03 z_p; body velocities + 0.02 z_v / z_w;
// robot_actions behind them.  z: standard normals [4][N][3] in the reference's randn_like order (euler, position, linvel,
// angvel).  Launched behind the reset launch: state, derived and actions are the post-reset tensors.
__global__ void __launch_bounds__(256) k_sim2real_obs(AgxEnvBuffers B, int n, const float *__restrict__ target,
                                                       const float *__restrict__ z, float *__restrict__ obs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const V3 err = task_vec(target, 0, n, i) - task_vec(B.state, 0, n, i);
  Q4 q = task_quat(B.state, 3, n, i);
  const float s = (float)(q.w > 0.0f) - (float)(q.w < 0.0f);
  q = Q4{s * q.x, s * q.y, s * q.z, s * q.w};
  float *st = const_cast<float *>(B.state);
  AGX_TASK_AT(st, 3) = q.x; AGX_TASK_AT(st, 4) = q.y; AGX_TASK_AT(st, 5) = q.z; AGX_TASK_AT(st, 6) = q.w;
  const float *ze = z + (size_t)i * 3, *zp = ze + (size_t)n * 3, *zv = zp + (size_t)n * 3, *zw = zv + (size_t)n * 3;
  const V3 e = euler_xyz_0_2pi(q);
  const Q4 qn = quat_from_euler(ssa(e.x) + ze[0] * 0.02f, ssa(e.y) + ze[1] * 0.02f, ssa(e.z) + ze[2] * 0.02f);
  const V3 vb = task_vec(B.derived, 10, n, i), wb = task_vec(B.derived, 13, n, i);
  float *of = obs + (size_t)i * 17;  // rows of 17 floats: 4-byte aligned only
  of[0] = err.x + zp[0] * 0.03f; of[1] = err.y + zp[1] * 0.03f; of[2] = err.z + zp[2] * 0.03f;
  of[3] = qn.x; of[4] = qn.y; of[5] = qn.z; of[6] = qn.w;
  of[7] = vb.x + zv[0] * 0.02f; of[8] = vb.y + zv[1] * 0.02f; of[9] = vb.z + zv[2] * 0.02f;
  of[10] = wb.x + zw[0] * 0.02f; of[11] = wb.y + zw[1] * 0.02f; of[12] = wb.z + zw[2] * 0.02f;
  of[13] = AGX_TASK_AT(B.actions, 0); of[14] = AGX_TASK_AT(B.actions, 1); of[15] = AGX_TASK_AT(B.actions, 2); of[16] = AGX_TASK_AT(B.actions, 3);
}

}  // namespace agx

using namespace agx;

static int s2r_check(const char *what, int kind, const AgxEnvBuffers *B, int n, bool publishes_reset_set = false) {
  AGX_REQUIRE(kind == AGX_SIM2REAL_VELOCITY || kind == AGX_SIM2REAL_ACCELERATION, "%s: kind %d", what, kind);
  return task_check(what, B, n, publishes_reset_set);
}

extern "C" int agx_sim2real_pre_step(int kind, const AgxEnvBuffers *B, int n, const float *target, const float *actions_before,
                                     float *actions, float *prev_actions, float *prev_dist, float *prev_actions_vehicle_frame,
                                     void *stream) {
  if (int e = s2r_check("agx_sim2real_pre_step", kind, B, n)) return e;
  AGX_REQUIRE(target && actions_before && actions && prev_actions && prev_dist, "agx_sim2real_pre_step: null buffer");
  AGX_REQUIRE(kind != AGX_SIM2REAL_ACCELERATION || prev_actions_vehicle_frame,
              "agx_sim2real_pre_step: the acceleration task needs prev_actions_vehicle_frame");
  AGX_REQUIRE(aligned16(actions_before) && aligned16(actions) && aligned16(prev_actions) &&
                  aligned16(prev_actions_vehicle_frame),
              "agx_sim2real_pre_step: the [N][4] action tensors must be 16-byte aligned");
  const int block = pick_block(n);
  hipLaunchKernelGGL(k_sim2real_pre_step, dim3(blocks_for(n, block)), dim3(block), 0, (hipStream_t)stream, kind, *B, n, target,
                     actions_before, actions, prev_actions, prev_dist, prev_actions_vehicle_frame);
  return check_launch("agx_sim2real_pre_step");
}

extern "C" int agx_sim2real_reward(int kind, const AgxEnvBuffers *B, int n, const float *target, const float *actions,
                                   const float *prev_actions, const float *prev_dist, float *actions_vehicle_frame,
                                   const float *prev_actions_vehicle_frame, int episode_len, int reset_on_collision, float *reward,
                                   void *stream) {
  if (int e = s2r_check("agx_sim2real_reward", kind, B, n, true)) return e;
  AGX_REQUIRE(target && actions && prev_actions && prev_dist && reward && B->derived && B->crashes && B->truncations &&
                  B->sim_steps && B->reset_mask && B->reset_flag,
              "agx_sim2real_reward: null buffer");
  AGX_REQUIRE(kind != AGX_SIM2REAL_ACCELERATION || (actions_vehicle_frame && prev_actions_vehicle_frame),
              "agx_sim2real_reward: the acceleration task needs both vehicle-frame action tensors");
  AGX_REQUIRE(aligned16(actions) && aligned16(prev_actions) && aligned16(actions_vehicle_frame) &&
                  aligned16(prev_actions_vehicle_frame),
              "agx_sim2real_reward: the [N][4] action tensors must be 16-byte aligned");
  const int block = pick_block(n);
  hipLaunchKernelGGL(k_sim2real_reward, dim3(blocks_for(n, block)), dim3(block), 0, (hipStream_t)stream, kind, *B, n, target, actions,
                     prev_actions, prev_dist, actions_vehicle_frame, prev_actions_vehicle_frame, episode_len, reset_on_collision,
                     reward);
  return check_launch("agx_sim2real_reward");
}

extern "C" int agx_sim2real_obs(const AgxEnvBuffers *B, int n, const float *target, const float *noise, float *obs, void *stream) {
  if (int e = task_check("agx_sim2real_obs", B, n)) return e;
  AGX_REQUIRE(target && noise && obs && B->derived && B->actions, "agx_sim2real_obs: null buffer");
  AGX_REQUIRE(!B->step_rows[0] && !B->step_rows[1], "agx_sim2real_obs: exchange rows (step_rows) are not written for the 17-D observation");
  const int block = pick_block(n);
  hipLaunchKernelGGL(k_sim2real_obs, dim3(blocks_for(n, block)), dim3(block), 0, (hipStream_t)stream, *B, n, target, noise, obs);
  return check_launch("agx_sim2real_obs");
}
