#pragma once
// The one-lane-per-env step kernel k_env_step<M, CTRL, SINGLE, WIDE> (108 instances), its ROV kind k_env_step_rov<CTRL, SINGLE, WIDE>
// (12 instances), its off-centre-mass kind k_env_step_com<M, CTRL, SINGLE, WIDE> (72 instances) and the occupancy they are compiled for.
// Part of the one translation unit agx_dynamics.hip, which alone includes it (after the AGX_DYN_* switches).

namespace agx {
// ---------------------------------------------------------------------------------------
// The env step: k fused physics sub-steps + (optionally) the task's reward / crash /
// truncation / reset set as an epilogue on the same registers.
// ---------------------------------------------------------------------------------------
// SINGLE: exactly one sub-step (empty_env, BASELINE config 1/2): straight-line code, no loop-
// carried copies of the loop invariants.
// WIDE: the launch uses one-wave workgroups (n <= 65536 envs: at most one wave per SIMD is resident anyway), so the
// kernel is compiled for ONE wave per SIMD and may use the whole 512-entry register file: no spill in any variant.
// !WIDE: 256-thread workgroups at AGX_DYN_WAVES waves per SIMD for batches that fill the chip several times over.
// Waves per SIMD a straight-line (SINGLE, 256-thread) instance is compiled for.  With the SoA accesses as buffer accesses (SoaRef)
// the laws without Euler-angle feedback fit 128 VGPRs without a spill (position: 113; was 148 with 64-bit address pairs): 4 waves.
constexpr int env_step_single_waves(int M, int CTRL) {
  return (M <= 6 && (CTRL == AGX_CTRL_NONE || CTRL == AGX_CTRL_POSITION || CTRL == AGX_CTRL_FULLY_ACTUATED || CTRL == AGX_CTRL_WRENCH))
             ? AGX_DYN_WAVES_LEAN_LAWS
             : (CTRL == AGX_CTRL_ACCELERATION ? 2 : AGX_DYN_WAVES);  // (the acceleration law: 168-181 VGPRs, spills at 3 waves)
}
// (the body: agx_dyn_env_step_body.h, shared as text with k_env_step_rov below)
template <int M, int CTRL, bool SINGLE, bool WIDE>
__global__ void __launch_bounds__(WIDE ? 64 : 256, WIDE ? 1 : (SINGLE ? env_step_single_waves(M, CTRL) : AGX_DYN_WAVES_LOOP))
    k_env_step(AgxRobotParams P, AgxEnvBuffers B, int n, const float *__restrict__ actions_in, int k_arg, AgxTaskArgs T) {
  constexpr bool ROV = false;
  constexpr bool COM = false;
  const V3 com{0.0f, 0.0f, 0.0f};
#include "agx_dyn_env_step_body.h"
}

// The ROV kind of the same step (AGX_LAUNCH_ROV): eight thrusters under the fully actuated law, no_control or the external wrench --
// the combinations an ROV can occur in (12 instances), compiled for the occupancy of the eight-motor multirotor instances.
template <int CTRL, bool SINGLE, bool WIDE>
__global__ void __launch_bounds__(WIDE ? 64 : 256, WIDE ? 1 : (SINGLE ? env_step_single_waves(8, CTRL) : AGX_DYN_WAVES_LOOP))
    k_env_step_rov(AgxRobotParams P, AgxEnvBuffers B, int n, const float *__restrict__ actions_in, int k_arg, AgxTaskArgs T) {
  static_assert(CTRL == AGX_CTRL_FULLY_ACTUATED || CTRL == AGX_CTRL_NONE || CTRL == AGX_CTRL_WRENCH, "the laws that read no Euler angles");
  constexpr int M = 8;
  constexpr bool ROV = true;
  constexpr bool COM = false;
  const V3 com{0.0f, 0.0f, 0.0f};
#include "agx_dyn_env_step_body.h"
}

// The kind of a multirotor whose centre of mass is not the base-link origin (agx_env_step_com): four or eight motors under every law
// k_env_step is compiled for (72 instances), at the occupancy of the k_env_step instance of the same arguments.  The offset travels
// as a trailing kernel argument: AgxRobotParams, AgxEnvBuffers and AgxTaskArgs stay what the other kernels receive.
template <int M, int CTRL, bool SINGLE, bool WIDE>
__global__ void __launch_bounds__(WIDE ? 64 : 256, WIDE ? 1 : (SINGLE ? env_step_single_waves(M, CTRL) : AGX_DYN_WAVES_LOOP))
    k_env_step_com(AgxRobotParams P, AgxEnvBuffers B, int n, const float *__restrict__ actions_in, int k_arg, AgxTaskArgs T, AgxComOffset C) {
  static_assert(M == 4 || M == 8, "compiled for four and eight motors");
  constexpr bool ROV = false;
  constexpr bool COM = true;
  const V3 com{C.c[0], C.c[1], C.c[2]};
#include "agx_dyn_env_step_body.h"
}
}  // namespace agx
