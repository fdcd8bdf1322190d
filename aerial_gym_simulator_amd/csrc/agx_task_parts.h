// Parts the stand-alone task kernels and their entry points share: the reset set of a step and its device flag, the two exponential
// reward families, the left-to-right sums, the Box-Muller pair, the plain [C][N] accessor, the tail of an exchange row, and the host
// checks of a task entry.  Included by agx_dynamics.hip (in front of agx_dyn_task.h), agx_sim2real.hip, agx_lidar_nav.hip,
// agx_task_glue.hip and agx_imu.hip.  The fused step kernels (agx_dyn_env_step_body.h, agx_dyn_quad.h, agx_dyn_position_step.h,
// agx_dyn_reset.h) interleave the reset set with their other stores and keep their own lines.
#pragma once
#include "agx_common.h"
#include "agx_device_math.h"
#include "agx_step_signal.h"

namespace agx {

// ---- the reset set of EnvManager.reset_terminated_and_truncated_envs (env_manager.py:364-371) ----
// one env: reset = crashes * reset_on_collision + truncations, stored into reset_mask
AGX_DEV bool reset_set_store(const AgxEnvBuffers &B, int i, bool crash, bool trunc, int reset_on_collision) {
  const bool reset = (crash && reset_on_collision) || trunc;
  B.reset_mask[i] = reset ? 1 : 0;
  return reset;
}
// ... behind the tasks' `truncations = sim_steps > episode_len`, stored as well
AGX_DEV bool reset_set_truncate(const AgxEnvBuffers &B, int i, bool crash, int episode_len, int reset_on_collision) {
  const bool trunc = B.sim_steps[i] > episode_len;
  B.truncations[i] = trunc ? 1 : 0;
  return reset_set_store(B, i, crash, trunc, reset_on_collision);
}
// the step's device flag: some env of the wave resets.  Must be reached by every lane of the wave (reset = false past the batch).
AGX_DEV void reset_flag_raise(const AgxEnvBuffers &B, bool reset) {
  if (__ballot(reset) != 0ull && (threadIdx.x & 63) == 0) atomicOr(B.reset_flag + B.flag_parity, 1);
}

// ---- reward terms.  The two families round differently (the square is taken first in one, last in the other): not interchangeable ----
// navigation tasks: mag * exp(-(v * v) * ex) and its penalty form
AGX_DEV float exp_reward(float mag, float ex, float v) { return mag * exp_cw(-(v * v) * ex); }
AGX_DEV float exp_penalty(float mag, float ex, float v) { return mag * (exp_cw(-(v * v) * ex) - 1.0f); }
// set-point tasks (exp_func / exp_penalty_func / abs_exp_func / abs_exp_penalty_func): gain * exp((-e * x) * x), gain * exp(-e * |x|)
AGX_DEV float gain_exp(float x, float gain, float e) { return gain * exp_cw((-e * x) * x); }
AGX_DEV float gain_exp_penalty(float x, float gain, float e) { return gain * (exp_cw((-e * x) * x) - 1.0f); }
AGX_DEV float gain_abs_exp(float x, float gain, float e) { return gain * exp_cw(-e * fabsf(x)); }
AGX_DEV float gain_abs_exp_penalty(float x, float gain, float e) { return gain * (exp_cw(-e * fabsf(x)) - 1.0f); }
// torch.sum(x, dim=1) of three / four columns, left to right
AGX_DEV float sum3(float a, float b, float c) { return (a + b) + c; }
AGX_DEV float sum4(float a, float b, float c, float d) { return ((a + b) + c) + d; }

// two standard normals from two uniforms (Box-Muller); 1 - u keeps the log argument in (0, 1]
AGX_DEV void normal_pair(float u1, float u2, float &z0, float &z1) {
  const float r = sqrtf(-2.0f * logf(1.0f - u1));
  float sn, cs;
  sincos_bounded(kTwoPi * u2, sn, cs);
  z0 = r * cs;
  z1 = r * sn;
}

// ---- component c of env i in a component-major [C][N] tensor, plain 64-bit indexing (n and i of the caller's scope; not the
// buffer addressing of the env-step kernels, AGX_AT) ----
#define AGX_TASK_AT(p, c) (p)[(size_t)(c) * (size_t)n + (size_t)i]
AGX_DEV V3 task_vec(const float *__restrict__ p, int c0, int n, int i) {
  return V3{AGX_TASK_AT(p, c0), AGX_TASK_AT(p, c0 + 1), AGX_TASK_AT(p, c0 + 2)};
}
AGX_DEV Q4 task_quat(const float *__restrict__ p, int c0, int n, int i) {
  return Q4{AGX_TASK_AT(p, c0), AGX_TASK_AT(p, c0 + 1), AGX_TASK_AT(p, c0 + 2), AGX_TASK_AT(p, c0 + 3)};
}

// reward | terminated | truncated behind the observation in the exchange row (header: step_rows)
AGX_DEV void write_step_row_tail(const AgxEnvBuffers &B, int i, float *__restrict__ row, int obs_dim) {
  row_store(B, row + obs_dim, B.step_reward[i]);
  row_store(B, row + obs_dim + 1, B.crashes[i] ? 1.0f : 0.0f);
  row_store(B, row + obs_dim + 2, B.truncations[i] ? 1.0f : 0.0f);
}

}  // namespace agx

// ---- host side of a task entry ----
static int task_check(const char *what, const AgxEnvBuffers *B, int n, bool publishes_reset_set = false) {
  AGX_REQUIRE(B != nullptr, "%s: null buffers", what);
  AGX_REQUIRE(n > 0, "%s: num_envs must be > 0 (got %d)", what, n);
  AGX_REQUIRE(n <= (1 << 26), "%s: num_envs %d above 2^26 per GPU: shard the job", what, n);
  AGX_REQUIRE(B->state != nullptr, "%s: buf->state is not set", what);
  AGX_REQUIRE(!publishes_reset_set || B->flag_parity == 0 || B->flag_parity == 1, "%s: flag_parity must be 0 or 1", what);
  return AGX_OK;
}
// the [N][4] action tensors are moved as one 16-byte access per env
static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
