#pragma once
// Open-loop rollouts: k_env_step_rollout<M, CTRL, WIDE> runs T env steps of the task-free multirotor step in ONE launch, one lane per
// env, and agx_env_rollout launches it.  What a lane holds in registers from the first load to the last store: the 13 state
// floats, the 16 derived floats (one sub-step stale, as k_env_step leaves them), M motor thrusts and their 3 M constants, the 12
// gains, robot_actions / robot_prev_actions, the step counter, the last crash flag and the first crashing step.  Per step it
// reads one action row (requested one step ahead) and, with obstacles, the boxes; it writes only the recorded channels.
// The sub-step arithmetic IS that of k_env_step: agx_dyn_env_substep.h, the text the three k_env_step kinds include, is included
// here a fourth time -- the same statements under the same contraction setting, so T steps of this kernel leave the bits that T
// launches of k_env_step (or of the lane-quad kernels, which are pinned to the same bits) leave.  What surrounds that text below
// mirrors agx_dyn_env_step_body.h: the loads of its lines 23-75, the epilogue of its lines 179-224 with T.kind == AGX_TASK_NONE,
// launch_flags == 0, no peer push.
// Part of the one translation unit agx_dynamics.hip, which alone includes it (after agx_dyn_env_step.h).

namespace agx {
// flattened record sources: AGX_REC_STATE 0..12, AGX_REC_DERIVED 13..28, AGX_REC_THRUST 29..36, AGX_REC_CRASH 37
constexpr int kRecState = 0, kRecDerived = 13, kRecThrust = 29, kRecCrash = 37, kRecSources = 38;
struct RolloutArgs {
  const float *actions;       // [N][A] held, or [T][N][A]
  unsigned action_stride;     // floats between two steps' blocks: 0 (held) or N A
  int steps;                  // T >= 1
  int k_max;                  // the scalar sub-step count, or the largest of k_steps (the LDS rows a lane owns)
  const int *k_steps;         // device [T], or null
  float *out;                 // [T][C][N], or null
  int channels;               // C
  int *first_crash;           // [N], or null
  signed char slot[kRecSources + 2];  // channel a source is recorded to, or -1
};

// Both widths are compiled for ONE wave per SIMD.  Next to everything a k-loop step instance holds, this kernel carries the derived
// tensors, both action histories and two action rows across the steps: at the step loop's two waves per SIMD (256 VGPRs) the
// 256-thread instances spilled 21-93 VGPRs inside the T x k loop.  What a second wave would hide is memory latency, and the loop
// has almost none: one action row per step.  (Reasoned from the register counts, not measured above 65536 envs.)
// Named k_env_step_*: it is the env-step text, with the frame slots the SGPR spiller reserves for that text's float64 coefficients.
template <int M, int CTRL, bool WIDE>
__global__ void __launch_bounds__(WIDE ? 64 : 256, 1)
    k_env_step_rollout(AgxRobotParams P, AgxEnvBuffers B, int n, RolloutArgs R) {
  static_assert(CTRL != AGX_CTRL_WRENCH, "built-in laws only: an external controller runs on the host between sub-steps");
  constexpr bool ROV = false, COM = false, EXT = false, lean = false;
  constexpr bool kLawReadsNoAngles = CTRL == AGX_CTRL_POSITION || CTRL == AGX_CTRL_FULLY_ACTUATED || CTRL == AGX_CTRL_NONE;
  const V3 com{0.0f, 0.0f, 0.0f};
  extern __shared__ float traj[];  // [k_max][3][blockDim] sub-step positions of the step in flight (only with obstacles)
  const int tid = threadIdx.x, bd = blockDim.x;
  const int i = blockIdx.x * bd + tid;
  if (i >= n) return;  // (no barrier below: a lane reads back only its own LDS entries)
  // what the host entry refuses stays out of the instance: host-drawn disturbance, the IMU's force row, the device step counter
  B.disturb = nullptr;
  B.body_force = nullptr;
  B.step_counter_dev = nullptr;
  const int step0 = B.step_counter;
  const int A = P.num_actions;
  EnvState s = load_state(B.state, n, i);
  float u[M], kT[M], tinc[M], tdec[M];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    u[j] = AGX_AT(B.motor_thrust, j);
    kT[j] = P.use_rps ? AGX_AT(B.motor_kT, j) : 1.0f;
    tinc[j] = B.motor_tau_inc ? AGX_AT(B.motor_tau_inc, j) : P.tau_inc_uniform;
    tdec[j] = B.motor_tau_dec ? AGX_AT(B.motor_tau_dec, j) : P.tau_dec_uniform;
  }
  // (the row index in 32 bits, as in the step body: n x 8 actions < 2^32; the step's block is a 64-bit scalar offset)
  const unsigned arow = (unsigned)i * (unsigned)A;
  float a_in[AGX_MAX_ACTIONS], a_next[AGX_MAX_ACTIONS], a_cur[AGX_MAX_ACTIONS], a_prev[AGX_MAX_ACTIONS];
#pragma unroll
  for (int c = 0; c < AGX_MAX_ACTIONS; ++c) {
    a_next[c] = c < A ? R.actions[arow + (unsigned)c] : 0.0f;
    a_cur[c] = c < A ? AGX_AT(B.actions, c) : 0.0f;
    a_prev[c] = c < A ? AGX_AT(B.prev_actions, c) : 0.0f;
    a_in[c] = 0.0f;
  }
  // a step of zero sub-steps leaves the derived tensors as they are, and the record shows them: they start from memory
  Derived d = load_derived(B.derived, n, i);
  const int steps_in = B.sim_steps[i];
  // the gains LAST (agx_dyn_env_step_body.h: behind the last load the wait in front of the uniform arm's moves costs nothing)
  Gains g{};
  if (CTRL != AGX_CTRL_NONE) g = B.gains ? load_gains(B.gains, n, i) : uniform_gains(P);
  Wrench wc{V3{0, 0, 0}, V3{0, 0, 0}};
  const bool root_link = P.root_link_mode != 0;
  constexpr int sub_base = 0;
  bool has_drag = false;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    has_drag = has_drag || P.lin_drag_linear[c] != 0.0f || P.lin_drag_quadratic[c] != 0.0f || P.ang_drag_linear[c] != 0.0f ||
               P.ang_drag_quadratic[c] != 0.0f;
  V3 tlo = s.p, thi = s.p;
  bool crashed = false, stepped = false;
  int first = -1;
  const size_t rec_step = (size_t)R.channels * (size_t)n;  // floats of one step's record
  // One step's record: a plain store per recorded source into out[(t C + c) N + i].  Issued at the top of the NEXT step (and once
  // behind the loop), in front of that step's action request: the wait for an action row then has no store in front of it
  // (loads and stores share one counter), and nothing ever waits for a record store.
#define AGX_REC(src_, val_)                                  \
  {                                                          \
    const int sl_ = R.slot[src_];                            \
    if (sl_ >= 0) rec_[(size_t)sl_ * (size_t)n] = (val_);    \
  }
#define AGX_RECORD_STEP(t_)                                                                                                   \
  if (R.out) {                                                                                                                \
    float *rec_ = R.out + (size_t)(t_) * rec_step + i;                                                                        \
    AGX_REC(kRecState + 0, s.p.x) AGX_REC(kRecState + 1, s.p.y) AGX_REC(kRecState + 2, s.p.z)                                 \
    AGX_REC(kRecState + 3, s.q.x) AGX_REC(kRecState + 4, s.q.y) AGX_REC(kRecState + 5, s.q.z) AGX_REC(kRecState + 6, s.q.w)   \
    AGX_REC(kRecState + 7, s.v.x) AGX_REC(kRecState + 8, s.v.y) AGX_REC(kRecState + 9, s.v.z)                                 \
    AGX_REC(kRecState + 10, s.w.x) AGX_REC(kRecState + 11, s.w.y) AGX_REC(kRecState + 12, s.w.z)                              \
    AGX_REC(kRecDerived + 0, d.euler.x) AGX_REC(kRecDerived + 1, d.euler.y) AGX_REC(kRecDerived + 2, d.euler.z)               \
    AGX_REC(kRecDerived + 3, d.qveh.x) AGX_REC(kRecDerived + 4, d.qveh.y) AGX_REC(kRecDerived + 5, d.qveh.z)                  \
    AGX_REC(kRecDerived + 6, d.qveh.w)                                                                                        \
    AGX_REC(kRecDerived + 7, d.vveh.x) AGX_REC(kRecDerived + 8, d.vveh.y) AGX_REC(kRecDerived + 9, d.vveh.z)                  \
    AGX_REC(kRecDerived + 10, d.vbody.x) AGX_REC(kRecDerived + 11, d.vbody.y) AGX_REC(kRecDerived + 12, d.vbody.z)            \
    AGX_REC(kRecDerived + 13, d.wbody.x) AGX_REC(kRecDerived + 14, d.wbody.y) AGX_REC(kRecDerived + 15, d.wbody.z)            \
    _Pragma("unroll") for (int j = 0; j < M; ++j) AGX_REC(kRecThrust + j, u[j])                                               \
    AGX_REC(kRecCrash, crashed ? 1.0f : 0.0f)                                                                                 \
  }
  for (int t = 0; t < R.steps; ++t) {
#pragma unroll
    for (int c = 0; c < AGX_MAX_ACTIONS; ++c) a_in[c] = a_next[c];
    if (t > 0) AGX_RECORD_STEP(t - 1)
    // the action row of step t + 1, requested before step t's sub-steps start (a held tensor was loaded once, above)
    if (R.action_stride != 0u && t + 1 < R.steps) {
      const float *next = R.actions + (size_t)(t + 1) * (size_t)R.action_stride;
#pragma unroll
      for (int c = 0; c < AGX_MAX_ACTIONS; ++c) a_next[c] = c < A ? next[arow + (unsigned)c] : 0.0f;
    }
    // the count stays inside the LDS rows the launch asked for, whatever the array holds
    const int k = R.k_steps ? min(max(R.k_steps[t], 0), R.k_max) : R.k_max;
    B.step_counter = (step0 + t) & 0x7FFFFFFF;  // the stream index the t-th separate step would have used (EnvManager._begin_step)
    for (int sub = 0; sub < k; ++sub) {
#include "agx_dyn_env_substep.h"
    }
    // EnvManager.reset_tensors + compute_observations: the flag is this step's alone, and a step without sub-steps clears it
    crashed = false;
    if (B.boxes && k > 0) crashed = collide_trajectory(B.boxes, B.num_boxes, n, i, traj, k, bd, tid, tlo, thi, P.collision_radius);
    if (crashed && first < 0) first = t;
    // RobotManagerIGE.pre_physics_step runs every sub-step: prev <- cur, cur <- action
    if (k > 0) {
      stepped = true;
#pragma unroll
      for (int c = 0; c < AGX_MAX_ACTIONS; ++c) {
        a_prev[c] = k >= 2 ? a_in[c] : a_cur[c];
        a_cur[c] = a_in[c];
      }
    }
  }
  AGX_RECORD_STEP(R.steps - 1)
#undef AGX_RECORD_STEP
#undef AGX_REC
  store_state(B.state, n, i, s);
  store_derived(B.derived, n, i, d);
#pragma unroll
  for (int j = 0; j < M; ++j) AGX_AT(B.motor_thrust, j) = u[j];
  if (B.wrench_cmd && stepped) {
    AGX_AT(B.wrench_cmd, 0) = wc.f.x; AGX_AT(B.wrench_cmd, 1) = wc.f.y; AGX_AT(B.wrench_cmd, 2) = wc.f.z;
    AGX_AT(B.wrench_cmd, 3) = wc.t.x; AGX_AT(B.wrench_cmd, 4) = wc.t.y; AGX_AT(B.wrench_cmd, 5) = wc.t.z;
  }
#pragma unroll
  for (int c = 0; c < AGX_MAX_ACTIONS; ++c) {
    if (c < A) {
      AGX_AT(B.prev_actions, c) = a_prev[c];
      AGX_AT(B.actions, c) = a_cur[c];
    }
  }
  B.sim_steps[i] = steps_in + R.steps;
  B.crashes[i] = crashed ? 1 : 0;
  B.truncations[i] = 0;
  if (R.first_crash) R.first_crash[i] = first;
}
}  // namespace agx

// ---- host entry ----
template <int M, int CTRL>
static int launch_env_rollout(bool wide, int grid, int block, size_t lds, hipStream_t stream, const AgxRobotParams &P, const AgxEnvBuffers &B,
                              int n, const agx::RolloutArgs &R) {
  const auto kernel = wide ? k_env_step_rollout<M, CTRL, true> : k_env_step_rollout<M, CTRL, false>;
  if (lds > kLdsDefaultMax) {  // 256-thread workgroups with obstacles and k >= 22 sub-steps (as launch_env_step)
    hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEnvStepLdsMax);
    AGX_REQUIRE(e == hipSuccess, "hipFuncSetAttribute(k_env_step_rollout, %zu bytes of LDS): %s", lds, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, stream, P, B, n, R);
  return AGX_OK;
}

extern "C" int agx_env_rollout(const AgxRobotParams *P, const AgxEnvBuffers *B, int n, const float *actions, int actions_per_step, int steps,
                               int substeps, const int *substeps_per_step, const AgxRolloutRecord *record, int *first_crash_step,
                               void *stream) {
  if (int e = check_common(P, B, n)) return e;
  AGX_REQUIRE(P != nullptr, "agx_env_rollout: null params");
  AGX_REQUIRE(actions != nullptr, "agx_env_rollout: null actions");
  AGX_REQUIRE(actions_per_step == 0 || actions_per_step == 1, "agx_env_rollout: actions_per_step is 0 (one [N][A] block held) or 1 (one block per step), got %d",
              actions_per_step);
  AGX_REQUIRE(steps >= 1, "agx_env_rollout: steps must be >= 1 (got %d)", steps);
  AGX_REQUIRE(substeps >= 0 && substeps <= AGX_MAX_SUBSTEPS, "agx_env_rollout: substeps out of range: %d", substeps);
  AGX_REQUIRE(P->controller != AGX_CTRL_WRENCH, "agx_env_rollout: AGX_CTRL_WRENCH -- an external controller or robot is evaluated by the host between sub-steps");
  AGX_REQUIRE(B->launch_flags == 0, "agx_env_rollout: launch_flags must be 0 (no split step, no AGX_LAUNCH_LEAN, no AGX_LAUNCH_ROV: got 0x%x)",
              (unsigned)B->launch_flags);
  AGX_REQUIRE(B->disturb == nullptr, "agx_env_rollout: buf->disturb is set -- host-drawn disturbance (strict_rng) is drawn per step");
  AGX_REQUIRE(B->body_force == nullptr, "agx_env_rollout: buf->body_force is set -- the IMU is updated by a launch of its own after every step");
  AGX_REQUIRE(B->step_counter_dev == nullptr, "agx_env_rollout: buf->step_counter_dev is set -- a captured step advances that word itself");
  AGX_REQUIRE(!B->step_rows[0] && !B->step_rows[1] && B->push_world <= 0, "agx_env_rollout: exchange rows / peer push are bound");
  AGX_REQUIRE(B->state && B->derived && B->actions && B->prev_actions && B->motor_thrust && B->crashes && B->truncations && B->sim_steps,
              "agx_env_rollout: null env buffer");
  AGX_REQUIRE(!P->use_rps || B->motor_kT, "agx_env_rollout: null motor_kT with use_rps");
  // (every step block of the actions is addressed with the 32-bit row offset of the step body plus a 64-bit scalar offset)
  AGX_REQUIRE((unsigned long long)n * (unsigned long long)P->num_actions < (1ull << 32), "agx_env_rollout: num_envs x num_actions must stay below 2^32");
  agx::RolloutArgs R{};
  R.actions = actions;
  R.action_stride = actions_per_step ? (unsigned)n * (unsigned)P->num_actions : 0u;
  R.steps = steps;
  R.k_max = substeps;
  R.k_steps = substeps_per_step;
  R.first_crash = first_crash_step;
  for (int c = 0; c < agx::kRecSources + 2; ++c) R.slot[c] = -1;
  if (record) {
    AGX_REQUIRE(record->out != nullptr, "agx_env_rollout: record->out is null");
    AGX_REQUIRE(record->channels >= 1 && record->channels <= AGX_ROLLOUT_MAX_CHANNELS, "agx_env_rollout: record->channels %d outside 1..%d",
                record->channels, AGX_ROLLOUT_MAX_CHANNELS);
    for (int c = 0; c < record->channels; ++c) {
      const int src = record->source[c], comp = record->component[c];
      const int rows = src == AGX_REC_STATE ? 13 : src == AGX_REC_DERIVED ? 16 : src == AGX_REC_THRUST ? P->num_motors : src == AGX_REC_CRASH ? 1 : 0;
      AGX_REQUIRE(rows > 0, "agx_env_rollout: record channel %d: unknown source %d", c, src);
      AGX_REQUIRE(comp >= 0 && comp < rows, "agx_env_rollout: record channel %d: component %d outside 0..%d of source %d", c, comp, rows - 1, src);
      const int flat = (src == AGX_REC_STATE ? agx::kRecState : src == AGX_REC_DERIVED ? agx::kRecDerived : src == AGX_REC_THRUST ? agx::kRecThrust : agx::kRecCrash) + comp;
      AGX_REQUIRE(R.slot[flat] < 0, "agx_env_rollout: record channels %d and %d name the same (source, component)", (int)R.slot[flat], c);
      R.slot[flat] = (signed char)c;
    }
    R.out = record->out;
    R.channels = record->channels;
  }
  const int block = pick_block(n), grid = blocks_for(n, block);
  const size_t lds = B->boxes ? (size_t)substeps * 3 * block * sizeof(float) : 0;
  AGX_REQUIRE(lds <= kEnvStepLdsMax, "agx_env_rollout needs %zu bytes of LDS (> %zu)", lds, kEnvStepLdsMax);
#define AGX_ROLLOUT_CTRL(M_)                                                                                                              \
  switch (P->controller) {                                                                                                                \
    case AGX_CTRL_NONE: if (int e = launch_env_rollout<M_, AGX_CTRL_NONE>(block == 64, grid, block, lds, (hipStream_t)stream, *P, *B, n, R)) return e; break; \
    case AGX_CTRL_POSITION: if (int e = launch_env_rollout<M_, AGX_CTRL_POSITION>(block == 64, grid, block, lds, (hipStream_t)stream, *P, *B, n, R)) return e; break; \
    case AGX_CTRL_VELOCITY: if (int e = launch_env_rollout<M_, AGX_CTRL_VELOCITY>(block == 64, grid, block, lds, (hipStream_t)stream, *P, *B, n, R)) return e; break; \
    case AGX_CTRL_ATTITUDE: if (int e = launch_env_rollout<M_, AGX_CTRL_ATTITUDE>(block == 64, grid, block, lds, (hipStream_t)stream, *P, *B, n, R)) return e; break; \
    case AGX_CTRL_RATES: if (int e = launch_env_rollout<M_, AGX_CTRL_RATES>(block == 64, grid, block, lds, (hipStream_t)stream, *P, *B, n, R)) return e; break; \
    case AGX_CTRL_ACCELERATION: if (int e = launch_env_rollout<M_, AGX_CTRL_ACCELERATION>(block == 64, grid, block, lds, (hipStream_t)stream, *P, *B, n, R)) return e; break; \
    case AGX_CTRL_VEL_STEERING: if (int e = launch_env_rollout<M_, AGX_CTRL_VEL_STEERING>(block == 64, grid, block, lds, (hipStream_t)stream, *P, *B, n, R)) return e; break; \
    default: if (int e = launch_env_rollout<M_, AGX_CTRL_FULLY_ACTUATED>(block == 64, grid, block, lds, (hipStream_t)stream, *P, *B, n, R)) return e; break; \
  }
  AGX_DISPATCH_M(P->num_motors, AGX_ROLLOUT_CTRL(kM))
#undef AGX_ROLLOUT_CTRL
  return check_launch("agx_env_rollout");
}
