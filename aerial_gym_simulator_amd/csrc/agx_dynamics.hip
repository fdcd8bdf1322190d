// Fused per-env dynamics for gfx950: update_states -> Lee controller -> allocation ->
// motor model -> drag / disturbance -> rigid-body integration -> collision flag,
// k physics sub-steps per launch, one lane per env, SoA loads/stores (coalesced: lane i
// touches X[c*N + i], i.e. 256 contiguous bytes per wave instruction).
//
// The reference runs this as ~590 tiny torch ops per sub-step plus PhysX
// (SURVEY.md section 2.1 C/D); here the whole env step is one kernel whose HBM traffic
// is the state itself: 13 floats in/out, M thrusts in/out, A actions, 16 derived
// floats out, 3M motor parameters and 12 gains in.
//
// No MFMA: there is no dense contraction in this path (the 6xM allocation products are
// per-env matrix-vector products with constant matrices held in SGPRs).
#include "agx_common.h"
// Arithmetic of the state path (controller, motor model, integrator, rewards).  Default: every + - * / sqrt is one
// correctly rounded IEEE operation (no fma contraction) and the elementary functions are the explicit kernels of
// agx_device_math.h, i.e. exactly the sequence the CPU restatement of the parity tests evaluates: the whole env step is
// BIT-IDENTICAL to that restatement (tests assert array_equal), which in turn is pinned to the reference's own outputs on the
// CPU.  Measured cost of exactness on MI355X (profiles/r02_parity_variants.json): k_env_step 10.3 -> 11.2 us at 8192 envs,
// 138 -> 154 us at 2^21 envs.  The two switches below re-enable the faster, ~1e-6-accurate arithmetic for A/B runs:
//   AGX_DYN_CONTRACT=1  let the compiler contract a*b+c into v_fma_f32
//   AGX_DYN_FAST_RCP=1  hardware v_rcp / v_rsq / v_sqrt (+ one Newton step) instead of correctly rounded division / sqrt
#ifndef AGX_DYN_CONTRACT
#define AGX_DYN_CONTRACT 0
#endif
#ifndef AGX_DYN_WAVES
// waves per SIMD the straight-line env-step kernels are compiled for.  With the scalar-base SoA addressing (soa_at) they
// need <= 168 VGPRs and fit 3; a limit of 4 (128 VGPRs) spills.  Measured (profiles/r01_soa_addressing.txt).
#define AGX_DYN_WAVES 3
#endif
#ifndef AGX_DYN_WAVES_LEAN_LAWS
#define AGX_DYN_WAVES_LEAN_LAWS 4  // env_step_single_waves
#endif
#ifndef AGX_DYN_WAVES_LOOP
// the k-loop variants (k > 1 sub-steps per launch) keep the loop-carried motor / action state next to everything the
// straight-line kernel needs: at 3 waves per SIMD (168 VGPRs) they spilled 24-136 VGPRs to scratch; 2 waves (256) fit.
#define AGX_DYN_WAVES_LOOP 2
#endif
#if AGX_DYN_CONTRACT
#pragma clang fp contract(fast)
#else
#pragma clang fp contract(off)
#endif
#include "agx_device_math.h"
#include "agx_nav_parts.h"
#include "agx_quad_math.h"
#include "agx_rng.h"
#include "agx_step_signal.h"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#ifndef AGX_DYN_FAST_RCP
#define AGX_DYN_FAST_RCP 0
#endif

// ---- host-side checks the entry points of every family share (the family headers below use them) ----
using namespace agx;

// instantiate the step kernel for every (motor count, controller) pair in use by the reference's
// multirotor configs: 4 (quad, lmf*, x500, magpie), 6, 8 (octarotor) motors
#define AGX_DISPATCH_M(M_, ...)                                       \
  switch (M_) {                                                       \
    case 4: { constexpr int kM = 4; __VA_ARGS__; } break;             \
    case 6: { constexpr int kM = 6; __VA_ARGS__; } break;             \
    case 8: { constexpr int kM = 8; __VA_ARGS__; } break;             \
    default: return fail(AGX_E_UNSUPPORTED, "num_motors %d: kernels are built for 4, 6 and 8 motors", M_); \
  }
#define AGX_DISPATCH_CTRL(C_, ...)                                                         \
  switch (C_) {                                                                            \
    case AGX_CTRL_NONE: { constexpr int kC = AGX_CTRL_NONE; __VA_ARGS__; } break;          \
    case AGX_CTRL_POSITION: { constexpr int kC = AGX_CTRL_POSITION; __VA_ARGS__; } break;  \
    case AGX_CTRL_VELOCITY: { constexpr int kC = AGX_CTRL_VELOCITY; __VA_ARGS__; } break;  \
    case AGX_CTRL_ATTITUDE: { constexpr int kC = AGX_CTRL_ATTITUDE; __VA_ARGS__; } break;  \
    case AGX_CTRL_RATES: { constexpr int kC = AGX_CTRL_RATES; __VA_ARGS__; } break;        \
    case AGX_CTRL_ACCELERATION: { constexpr int kC = AGX_CTRL_ACCELERATION; __VA_ARGS__; } break; \
    case AGX_CTRL_VEL_STEERING: { constexpr int kC = AGX_CTRL_VEL_STEERING; __VA_ARGS__; } break; \
    case AGX_CTRL_FULLY_ACTUATED: { constexpr int kC = AGX_CTRL_FULLY_ACTUATED; __VA_ARGS__; } break; \
    case AGX_CTRL_WRENCH: { constexpr int kC = AGX_CTRL_WRENCH; __VA_ARGS__; } break;      \
    default: return fail(AGX_E_ARG, "unknown controller id %d", C_);                       \
  }

static int check_common(const AgxRobotParams *P, const AgxEnvBuffers *B, int n) {
  AGX_REQUIRE(B != nullptr, "null buffers");
  AGX_REQUIRE(n > 0, "num_envs must be > 0 (got %d)", n);
  // (SoaRef: a tensor's [<= 16][N] floats are addressed with 32-bit byte offsets from its base)
  AGX_REQUIRE(n <= (1 << 26), "num_envs %d above 2^26 = 67 108 864 per GPU: shard the job (the SoA accesses use 32-bit byte offsets)", n);
  AGX_REQUIRE(B->flag_parity == 0 || B->flag_parity == 1, "flag_parity must be 0 or 1");
  AGX_REQUIRE((!B->step_rows[0] && !B->step_rows[1]) ||
                  (B->step_rows[0] && B->step_rows[1] && B->step_reward && B->crashes && B->truncations),
              "step_rows needs both parity buffers, step_reward, crashes and truncations");
  if (P) {
    AGX_REQUIRE(P->num_motors >= 1 && P->num_motors <= AGX_MAX_MOTORS, "num_motors out of range");
    AGX_REQUIRE(P->num_actions >= 1 && P->num_actions <= AGX_MAX_ACTIONS, "num_actions out of range");
    AGX_REQUIRE(P->controller >= 0 && P->controller <= AGX_CTRL_WRENCH, "unknown controller id %d", P->controller);
    AGX_REQUIRE(P->controller != AGX_CTRL_FULLY_ACTUATED || P->num_actions == 7, "fully actuated controller needs 7 actions");
    AGX_REQUIRE(P->controller != AGX_CTRL_NONE || P->num_actions == P->num_motors, "no_control needs num_actions == num_motors");
    AGX_REQUIRE(P->controller == AGX_CTRL_NONE || P->controller == AGX_CTRL_FULLY_ACTUATED || P->controller == AGX_CTRL_WRENCH ||
                    P->num_actions == 4,
                "Lee controllers take 4 actions");
  }
  return AGX_OK;
}

// AGX_LAUNCH_ROV (the robot kind BaseROV): the kernels of that kind exist for eight thrusters under the laws that read no Euler
// angles -- the ROV's are not wrapped to (-pi, pi], which the Lee laws with Euler-angle feedback assume
static int check_rov(const AgxRobotParams *P, const char *entry) {
  AGX_REQUIRE(P->num_motors == 8, "%s: AGX_LAUNCH_ROV needs num_motors == 8 (got %d)", entry, P->num_motors);
  AGX_REQUIRE(P->controller == AGX_CTRL_FULLY_ACTUATED || P->controller == AGX_CTRL_NONE || P->controller == AGX_CTRL_WRENCH,
              "%s: AGX_LAUNCH_ROV runs the fully actuated law, no_control or an external wrench, not the Lee controller id %d", entry,
              P->controller);
  return AGX_OK;
}

// the lane-quad kernels leave the drag terms out: any non-zero coefficient keeps k_env_step
static bool has_drag(const AgxRobotParams *P) {
  for (int c = 0; c < 3; ++c)
    if (P->lin_drag_linear[c] != 0.0f || P->lin_drag_quadratic[c] != 0.0f || P->ang_drag_linear[c] != 0.0f ||
        P->ang_drag_quadratic[c] != 0.0f)
      return true;
  return false;
}

// The four-lanes-per-env kernel covers the plain quadrotor position step; agx_set_option("env_step_quad", 0) keeps k_env_step (A/B runs).
static bool quad_kernel_usable(const AgxRobotParams *P, const AgxEnvBuffers *B, const AgxTaskArgs *T) {
  if (!option_env_step_quad() || B->boxes || B->launch_flags != 0 || B->disturb || B->disturb_prob > 0.0f || P->num_actions != 4) return false;
  if (T->kind != AGX_TASK_NONE && T->kind != AGX_TASK_POSITION) return false;
  return !has_drag(P);
}

// ... and the sub-step loop of the velocity / acceleration controlled quadrotors (navigation tasks)
static bool quad_loop_kernel_usable(const AgxRobotParams *P, const AgxEnvBuffers *B, int n, int k) {
  if (!option_env_step_quad() || pick_block(n) != 64 || k < 1 || B->launch_flags != 0) return false;
  const bool lee_quad = P->num_motors == 4 && P->num_actions == 4 && P->controller >= AGX_CTRL_POSITION &&
                        P->controller <= AGX_CTRL_VEL_STEERING;
  const bool fa_octa = P->num_motors == 8 && P->num_actions == 7 && P->controller == AGX_CTRL_FULLY_ACTUATED;
  const bool lee_octa = P->num_motors == 8 && P->num_actions == 4 && (P->controller == AGX_CTRL_POSITION || P->controller == AGX_CTRL_VELOCITY);
  if (!lee_quad && !fa_octa && !lee_octa) return false;
  return !has_drag(P);
}

#include "agx_dyn_state.h"
#include "agx_dyn_physics.h"
#include "agx_task_parts.h"
#include "agx_dyn_task.h"
#include "agx_dyn_env_step.h"
#include "agx_dyn_quad.h"
#include "agx_dyn_robot.h"
#include "agx_dyn_reset.h"
#include "agx_dyn_end_to_end.h"
#include "agx_dyn_position_step.h"

// Which env-step kernel a launch runs, decided ONCE: agx_env_step switches on it and agx_env_step_kernel prints it (bench.py and the
// GPU tests trust that name).  On the per-step launch path: no allocation, no formatting.
enum EnvStepFamily { ENV_STEP_QUAD_POSITION, ENV_STEP_QUAD_LOOP, ENV_STEP_ONE_LANE };
struct EnvStepChoice {
  EnvStepFamily family;
  int M, ctrl;        // template arguments of k_env_step_quad_loop<M, CTRL> and k_env_step<M, CTRL, SINGLE, WIDE>
  bool single, wide;  // ... of k_env_step only
  int block, grid;    // threads per workgroup; workgroups that carry envs (the proof-slot launch adds its folding workgroup)
  bool rov;           // AGX_LAUNCH_ROV: k_env_step_rov<CTRL, SINGLE, WIDE> (one-lane family only: the lane-quad kernels need launch_flags == 0)
};
// com: agx_env_step_com -- k_env_step_com<M, CTRL, SINGLE, WIDE>, of the one-lane family at every batch size (the lane-quad kernels do not carry the offset)
static EnvStepChoice choose_env_step(const AgxRobotParams *P, const AgxEnvBuffers *B, int n, int k, const AgxTaskArgs &T, bool com = false) {
  const int block = pick_block(n);
  if (com) return EnvStepChoice{ENV_STEP_ONE_LANE, P->num_motors, P->controller, k == 1, block == 64, block, blocks_for(n, block), false};
  if (k == 1 && block == 64 && P->num_motors == 4 && P->controller == AGX_CTRL_POSITION && quad_kernel_usable(P, B, &T))
    return EnvStepChoice{ENV_STEP_QUAD_POSITION, 4, AGX_CTRL_POSITION, true, true, 64, blocks_for(n, 16), false};
  if (quad_loop_kernel_usable(P, B, n, k))
    return EnvStepChoice{ENV_STEP_QUAD_LOOP, P->num_motors, P->controller, false, true, 64, blocks_for(n, 16), false};
  return EnvStepChoice{ENV_STEP_ONE_LANE, P->num_motors, P->controller, k == 1, block == 64, block, blocks_for(n, block),
                       (B->launch_flags & AGX_LAUNCH_ROV) != 0};
}

// Dynamic LDS one launch may ask for without saying so first, and the most the 256-thread instance can ask for (obstacles, k = 32).
constexpr size_t kLdsDefaultMax = 64 * 1024;
constexpr size_t kEnvStepLdsMax = (size_t)AGX_MAX_SUBSTEPS * 3 * 256 * sizeof(float);
static_assert(kEnvStepLdsMax <= 160 * 1024, "the sub-step positions of a 256-thread workgroup must fit the CU's 160 KiB of LDS");

template <int M, int CTRL>
static int launch_env_step(const EnvStepChoice &c, size_t lds, hipStream_t stream, const AgxRobotParams &P, const AgxEnvBuffers &B, int n,
                           const float *actions_in, int k, const AgxTaskArgs &T) {
  const auto kernel = c.single ? (c.wide ? k_env_step<M, CTRL, true, true> : k_env_step<M, CTRL, true, false>)
                               : (c.wide ? k_env_step<M, CTRL, false, true> : k_env_step<M, CTRL, false, false>);
  if (lds > kLdsDefaultMax) {
    // 256-thread workgroups with obstacles and k >= 22 sub-steps: opted in as the LBVH build is (agx_scene.hip).  Off the hot
    // path: every other launch stays below the default and does not come here.
    hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEnvStepLdsMax);
    AGX_REQUIRE(e == hipSuccess, "hipFuncSetAttribute(k_env_step, %zu bytes of LDS): %s", lds, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kernel, dim3(c.grid), dim3(c.block), lds, stream, P, B, n, actions_in, k, T);
  return AGX_OK;
}

template <int CTRL>
static int launch_env_step_rov(const EnvStepChoice &c, size_t lds, hipStream_t stream, const AgxRobotParams &P, const AgxEnvBuffers &B, int n,
                               const float *actions_in, int k, const AgxTaskArgs &T) {
  const auto kernel = c.single ? (c.wide ? k_env_step_rov<CTRL, true, true> : k_env_step_rov<CTRL, true, false>)
                               : (c.wide ? k_env_step_rov<CTRL, false, true> : k_env_step_rov<CTRL, false, false>);
  if (lds > kLdsDefaultMax) {
    hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEnvStepLdsMax);
    AGX_REQUIRE(e == hipSuccess, "hipFuncSetAttribute(k_env_step_rov, %zu bytes of LDS): %s", lds, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kernel, dim3(c.grid), dim3(c.block), lds, stream, P, B, n, actions_in, k, T);
  return AGX_OK;
}

template <int M, int CTRL>
static int launch_env_step_com(const EnvStepChoice &c, size_t lds, hipStream_t stream, const AgxRobotParams &P, const AgxEnvBuffers &B, int n,
                               const float *actions_in, int k, const AgxTaskArgs &T, const AgxComOffset &com) {
  const auto kernel = c.single ? (c.wide ? k_env_step_com<M, CTRL, true, true> : k_env_step_com<M, CTRL, true, false>)
                               : (c.wide ? k_env_step_com<M, CTRL, false, true> : k_env_step_com<M, CTRL, false, false>);
  if (lds > kLdsDefaultMax) {
    hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEnvStepLdsMax);
    AGX_REQUIRE(e == hipSuccess, "hipFuncSetAttribute(k_env_step_com, %zu bytes of LDS): %s", lds, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kernel, dim3(c.grid), dim3(c.block), lds, stream, P, B, n, actions_in, k, T, com);
  return AGX_OK;
}

// agx_env_step_com: the kernels of that kind exist for four and eight motors and write no IMU force
static int check_com(const AgxRobotParams *P, const AgxEnvBuffers *B) {
  AGX_REQUIRE((B->launch_flags & AGX_LAUNCH_ROV) == 0, "agx_env_step_com: AGX_LAUNCH_ROV -- the ROV kind carries no centre-of-mass offset");
  AGX_REQUIRE(P->num_motors == 4 || P->num_motors == 8, "agx_env_step_com needs num_motors == 4 or 8 (got %d)", P->num_motors);
  AGX_REQUIRE(B->body_force == nullptr,
              "agx_env_step_com: buf->body_force is set -- an IMU on an airframe with an off-centre mass is not modelled (no lever-arm terms)");
  AGX_REQUIRE((B->launch_flags & AGX_LAUNCH_LEAN) == 0, "agx_env_step_com: AGX_LAUNCH_LEAN is not available with a centre-of-mass offset");
  return AGX_OK;
}

// agx_env_step and agx_env_step_com (com != NULL): the same checks, the same launch geometry
static int env_step(const char *entry, const AgxRobotParams *P, const AgxEnvBuffers *B, int n, const float *actions_in, int k,
                    const AgxTaskArgs *task, const AgxComOffset *com, void *stream) {
  if (int e = check_common(P, B, n)) return e;
  AGX_REQUIRE(P != nullptr, "null params");
  if (com)
    if (int e = check_com(P, B)) return e;
  AGX_REQUIRE(actions_in != nullptr, "null actions");
  AGX_REQUIRE(k >= 0 && k <= AGX_MAX_SUBSTEPS, "k_substeps out of range: %d", k);
  AGX_REQUIRE(P->controller != AGX_CTRL_WRENCH || k <= 1,
              "external controller (AGX_CTRL_WRENCH): one launch per physics sub-step, the host re-evaluates the controller in between");
  AGX_REQUIRE((B->launch_flags & ~(0xFF0F | AGX_LAUNCH_ROV)) == 0, "launch_flags: bits 0-3, the sub-step index in bits 8-15 and AGX_LAUNCH_ROV");
  if (B->launch_flags & AGX_LAUNCH_ROV)
    if (int e = check_rov(P, "agx_env_step")) return e;
  AGX_REQUIRE((B->launch_flags & AGX_LAUNCH_BODY_WRENCH) == 0 || P->controller == AGX_CTRL_WRENCH,
              "AGX_LAUNCH_BODY_WRENCH (external robot) goes with AGX_CTRL_WRENCH: actions_in is a wrench [N][6]");
  AGX_REQUIRE((B->launch_flags & 4) == 0 || ((B->launch_flags & 3) == 0 && P->controller != AGX_CTRL_WRENCH &&
                                             (!task || task->kind != AGX_TASK_NAVIGATION)),
              "AGX_LAUNCH_LEAN needs the fused step of a built-in controller without the navigation reward (it reads the action history)");
  AGX_REQUIRE(B->state && B->derived && B->actions && B->prev_actions && B->motor_thrust && B->crashes && B->truncations &&
                  B->sim_steps,
              "null env buffer");
  AGX_REQUIRE(!P->use_rps || B->motor_kT, "null motor_kT with use_rps");
  AgxTaskArgs T{};
  if (task) T = *task;
  AGX_REQUIRE(T.kind >= AGX_TASK_NONE && T.kind <= AGX_TASK_NAVIGATION, "bad task kind %d", T.kind);
  if (T.kind != AGX_TASK_NONE) {
    AGX_REQUIRE(T.target && T.reward && B->reset_mask && B->reset_flag, "null task buffer");
    AGX_REQUIRE(T.kind != AGX_TASK_NAVIGATION || (T.pos_err && T.prev_pos_err && P->num_actions >= 4), "null navigation buffer");
    AGX_REQUIRE((!T.successes && !T.timeouts && !T.counters) || (T.successes && T.timeouts && T.counters && T.kind == AGX_TASK_NAVIGATION),
                "navigation bookkeeping in the epilogue needs successes, timeouts and counters, and the navigation task kind");
  }
  const EnvStepChoice c = choose_env_step(P, B, n, k, T, com != nullptr);
  const dim3 grid(c.grid), block(c.block);
  if (c.family == ENV_STEP_QUAD_POSITION) {
    // (with proof slots: one more workgroup, the first, folds the previous launch's slots into the host record)
    hipLaunchKernelGGL(k_env_step_quad_position, dim3(c.grid + (T.proof_slots ? 1 : 0)), block, 0, (hipStream_t)stream, *P, *B, n,
                       actions_in, T);
    return check_launch("agx_env_step");
  }
  AGX_REQUIRE(!T.proof_slots && T.proof_mode == AGX_STEP_TWO, "AgxTaskArgs.proof_*: the four-lanes-per-env position kernel only");
  // the sub-step positions of a workgroup's envs (only with obstacles): 16 envs per wave in the lane-quad loop, one per lane otherwise
  const size_t lds = B->boxes ? (size_t)k * 3 * (c.family == ENV_STEP_QUAD_LOOP ? 16 : c.block) * sizeof(float) : 0;
  if (c.family == ENV_STEP_QUAD_LOOP) {
#define AGX_QUAD_LOOP(M_, C_)                                                                                                          \
  if (c.M == M_ && c.ctrl == C_)                                                                                                       \
    hipLaunchKernelGGL((k_env_step_quad_loop<M_, C_>), grid, block, lds, (hipStream_t)stream, *P, *B, n, actions_in, k, T);
    AGX_QUAD_LOOP(4, AGX_CTRL_POSITION)
    AGX_QUAD_LOOP(4, AGX_CTRL_VELOCITY)
    AGX_QUAD_LOOP(4, AGX_CTRL_ATTITUDE)
    AGX_QUAD_LOOP(4, AGX_CTRL_RATES)
    AGX_QUAD_LOOP(4, AGX_CTRL_ACCELERATION)
    AGX_QUAD_LOOP(4, AGX_CTRL_VEL_STEERING)
    AGX_QUAD_LOOP(8, AGX_CTRL_POSITION)
    AGX_QUAD_LOOP(8, AGX_CTRL_VELOCITY)
    AGX_QUAD_LOOP(8, AGX_CTRL_FULLY_ACTUATED)
#undef AGX_QUAD_LOOP
    return check_launch("agx_env_step");
  }
  AGX_REQUIRE(lds <= kEnvStepLdsMax, "agx_env_step needs %zu bytes of LDS (> %zu)", lds, kEnvStepLdsMax);
  if (c.rov) {  // (check_rov above: eight motors, one of these three laws)
    int e = c.ctrl == AGX_CTRL_FULLY_ACTUATED ? launch_env_step_rov<AGX_CTRL_FULLY_ACTUATED>(c, lds, (hipStream_t)stream, *P, *B, n, actions_in, k, T)
            : c.ctrl == AGX_CTRL_NONE         ? launch_env_step_rov<AGX_CTRL_NONE>(c, lds, (hipStream_t)stream, *P, *B, n, actions_in, k, T)
                                              : launch_env_step_rov<AGX_CTRL_WRENCH>(c, lds, (hipStream_t)stream, *P, *B, n, actions_in, k, T);
    if (e) return e;
    return check_launch("agx_env_step");
  }
  if (com) {  // (check_com above: four or eight motors)
    if (c.M == 4) {
      AGX_DISPATCH_CTRL(c.ctrl, if (int e = launch_env_step_com<4, kC>(c, lds, (hipStream_t)stream, *P, *B, n, actions_in, k, T, *com)) return e);
    } else {
      AGX_DISPATCH_CTRL(c.ctrl, if (int e = launch_env_step_com<8, kC>(c, lds, (hipStream_t)stream, *P, *B, n, actions_in, k, T, *com)) return e);
    }
    return check_launch(entry);
  }
  AGX_DISPATCH_M(c.M, AGX_DISPATCH_CTRL(c.ctrl, if (int e = launch_env_step<kM, kC>(c, lds, (hipStream_t)stream, *P, *B, n, actions_in, k, T)) return e));
  return check_launch("agx_env_step");
}

extern "C" int agx_env_step(const AgxRobotParams *P, const AgxEnvBuffers *B, int n, const float *actions_in, int k,
                            const AgxTaskArgs *task, void *stream) {
  return env_step("agx_env_step", P, B, n, actions_in, k, task, nullptr, stream);
}

extern "C" int agx_env_step_com(const AgxRobotParams *P, const AgxEnvBuffers *B, int n, const float *actions_in, int k,
                                const AgxTaskArgs *task, const AgxComOffset *com, void *stream) {
  AGX_REQUIRE(com != nullptr, "agx_env_step_com: null centre-of-mass offset");
  return env_step("agx_env_step_com", P, B, n, actions_in, k, task, com, stream);
}

// T task-free env steps in one launch (k_env_step_rollout, agx_env_rollout): uses check_common, pick_block and the LDS bounds above
#include "agx_dyn_rollout.h"

extern "C" int agx_env_step_kernel(const AgxRobotParams *P, const AgxEnvBuffers *B, int n, int k, const AgxTaskArgs *task, char *out,
                                   int cap) {
  AGX_REQUIRE(P && B && out && cap > 0 && n > 0, "bad arguments");
  AgxTaskArgs T{};
  if (task) T = *task;
  const EnvStepChoice c = choose_env_step(P, B, n, k, T);
  const int threads = c.grid * c.block;
  if (c.family == ENV_STEP_QUAD_POSITION)
    snprintf(out, (size_t)cap, "k_env_step_quad_position_%d", threads);
  else if (c.family == ENV_STEP_QUAD_LOOP)
    snprintf(out, (size_t)cap, "k_env_step_quad_loop<%d,%d>_%d", c.M, c.ctrl, threads);
  else if (c.rov)
    snprintf(out, (size_t)cap, "k_env_step_rov<%d,%s,%s>_%d", c.ctrl, c.single ? "true" : "false", c.wide ? "true" : "false", threads);
  else
    snprintf(out, (size_t)cap, "k_env_step<%d,%d,%s,%s>_%d", c.M, c.ctrl, c.single ? "true" : "false", c.wide ? "true" : "false", threads);
  return AGX_OK;
}

extern "C" int agx_dynamics_substeps(const AgxRobotParams *P, const AgxEnvBuffers *B, int n, const float *actions_in,
                                     int k, void *stream) {
  return agx_env_step(P, B, n, actions_in, k, nullptr, stream);
}

extern "C" int agx_push_advance(AgxEnvBuffers *b) {
  AGX_REQUIRE(b && b->push_world > 0 && b->push_world <= 8 && b->push_slots >= 5 && b->push_base && b->push_slice_bytes > 0,
              "agx_push_advance: peer push is not bound (or fewer than 5 receive slots)");
  b->push_pub_seq = b->push_seq;  // the rows of the step before are announced by the first kernel of this one
  b->push_pub_index = b->push_flag_index;
  const uint32_t seq = ++b->push_seq;
  const int slot = (int)((seq - 1u) % (uint32_t)b->push_slots);
  b->push_flag_index = slot * b->push_world + b->push_rank;
  b->step_rows[0] = b->step_rows[1] = (float *)(b->push_base + ((size_t)slot * b->push_world + b->push_rank) * (size_t)b->push_slice_bytes);
  if (seq > 2u) {
    b->push_wait_seq = seq - 2u;
    b->push_wait_index = (int)((seq - 3u) % (uint32_t)b->push_slots) * b->push_world;
  } else {
    b->push_wait_seq = 0u;
  }
  return AGX_OK;
}
