#pragma once
// Stand-alone robot plug-in kernels, k_update_states through k_net_body_wrench, with their entry points: the pieces of the env step
// a host-side robot or controller class calls one at a time.  None of them is on the hot path.
// Part of the one translation unit agx_dynamics.hip, which alone includes it (after the AGX_DYN_* switches).

namespace agx {
__global__ void __launch_bounds__(256) k_update_states(AgxEnvBuffers B, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  EnvState s = load_state(B.state, n, i);
  store_derived(B.derived, n, i, update_states(s));
}
__global__ void __launch_bounds__(256) k_update_states_rov(AgxEnvBuffers B, int n) {  // AGX_LAUNCH_ROV
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  EnvState s = load_state(B.state, n, i);
  store_derived(B.derived, n, i, update_states_rov(s));
}

// EnvManager.compute_observations (env_manager.py:358-362) on its own: crashes[i] |= the robot's collision sphere at its CURRENT
// position overlaps an obstacle box -- the predicate of the fused step (sphere_hits_box) without a trajectory.
__global__ void __launch_bounds__(256) k_collide_spheres_boxes(AgxEnvBuffers B, int n, float radius) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const V3 p = V3{AGX_AT(B.state, 0), AGX_AT(B.state, 1), AGX_AT(B.state, 2)};
  const float r2 = radius * radius;
  bool hit = false;
  for (int b = 0; b < B.num_boxes; ++b) {
    const float *bx = B.boxes + (size_t)b * 11 * n + i;
    const V3 c = V3{bx[0], bx[(size_t)n], bx[2 * (size_t)n]};
    const float reach = bx[10 * (size_t)n] + radius + 1.0e-3f;  // the box's bounding radius: conservative cull, the flag is exact
    const float dx = p.x - c.x, dy = p.y - c.y, dz = p.z - c.z;
    if (dx * dx + dy * dy + dz * dz > reach * reach) continue;
    const Q4 q = Q4{bx[3 * (size_t)n], bx[4 * (size_t)n], bx[5 * (size_t)n], bx[6 * (size_t)n]};
    const V3 h = V3{bx[7 * (size_t)n], bx[8 * (size_t)n], bx[9 * (size_t)n]};
    hit = hit || sphere_hits_box(p, c, q, h, r2);
  }
  if (hit) B.crashes[i] = 1;
}

__global__ void __launch_bounds__(256) k_controller_wrench(AgxRobotParams P, AgxEnvBuffers B, int n, const float *__restrict__ action) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  EnvState s = load_state(B.state, n, i);
  Derived d = load_derived(B.derived, n, i);
  Gains g = B.gains ? load_gains(B.gains, n, i) : uniform_gains(P);
  float a[AGX_MAX_ACTIONS];
#pragma unroll
  for (int c = 0; c < AGX_MAX_ACTIONS; ++c)
    a[c] = (c < P.num_actions) ? clamp_minmax(action[(size_t)i * P.num_actions + c], -10.0f, 10.0f) : 0.0f;
  store_wrench_cmd(B.wrench_cmd, n, i, run_controller_by_id(P, s, d, a, g));
}

// BaseMultirotor.step(action) of the reference as ONE launch (agx_robot_step; the robot plug-in's super().step()):
// update_states, clip, controller, allocation + motor model, the per-body force / torque tensors, drag, disturbance.
// One lane per env, runtime motor count and control law: a plug-in path evaluated between host calls, not a hot loop.
// ROV: BaseROV.step (base_rov.py:287-298) -- Euler angles without ssa(), per-axis quadratic drag on the linear velocity.
template <bool ROV>
__global__ void __launch_bounds__(256) k_robot_step(AgxRobotParams P, AgxEnvBuffers B, int n, const float *__restrict__ action,
                                                    AgxRobotStepArgs R) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int M = P.num_motors, A = P.num_actions, NB = R.num_bodies;
  EnvState s = load_state(B.state, n, i);
  const Derived d = ROV ? update_states_rov(s) : update_states(s);
  store_derived(B.derived, n, i, d);
  float a[AGX_MAX_ACTIONS];
#pragma unroll
  for (int c = 0; c < AGX_MAX_ACTIONS; ++c) a[c] = (c < A) ? clamp_minmax(action[(size_t)i * A + c], -10.0f, 10.0f) : 0.0f;  // clip_actions
  float u[AGX_MAX_MOTORS];
  Wrench wc{V3{0, 0, 0}, V3{0, 0, 0}};
  if (P.controller != AGX_CTRL_NONE) {
    Gains g = B.gains ? load_gains(B.gains, n, i) : uniform_gains(P);
    wc = run_controller_by_id(P, s, d, a, g);
  }
  const float w6[6] = {wc.f.x, wc.f.y, wc.f.z, wc.t.x, wc.t.y, wc.t.z};
#pragma unroll
  for (int j = 0; j < AGX_MAX_MOTORS; ++j) {
    u[j] = 0.0f;
    if (j < M) {
      float ref = a[j];  // no_control: the action IS the motor command
      if (P.controller != AGX_CTRL_NONE) {
        ref = 0.0f;
#pragma unroll
        for (int c = 0; c < 6; ++c) ref += P.alloc_pinv[6 * j + c] * w6[c];
      }
      const float kT = P.use_rps ? AGX_AT(B.motor_kT, j) : 1.0f;
      const float tinc = B.motor_tau_inc ? AGX_AT(B.motor_tau_inc, j) : P.tau_inc_uniform;
      const float tdec = B.motor_tau_dec ? AGX_AT(B.motor_tau_dec, j) : P.tau_dec_uniform;
      u[j] = motor_update(P, ref, AGX_AT(B.motor_thrust, j), kT, tinc, tdec);
      AGX_AT(B.motor_thrust, j) = u[j];
    }
  }
  if (B.wrench_cmd) store_wrench_cmd(B.wrench_cmd, n, i, wc);
  // call_controller (base_multirotor.py:246-258): output_forces / output_torques are zero outside the application mask
  float *F = R.force + (size_t)i * NB * 3, *T = R.torque + (size_t)i * NB * 3;
  for (int b = 0; b < NB * 3; ++b) { F[b] = 0.0f; T[b] = 0.0f; }
  if (P.root_link_mode) {  // control_allocation.py:67-79: output wrench = A u at the (single) masked body
    float w[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      float acc = 0.0f;
      for (int j = 0; j < M; ++j) acc += P.alloc[M * r + j] * u[j];
      w[r] = acc;
    }
    const int b = R.body_of_motor[0];
    F[3 * b] = w[0]; F[3 * b + 1] = w[1]; F[3 * b + 2] = w[2];
    T[3 * b] = w[3]; T[3 * b + 1] = w[4]; T[3 * b + 2] = w[5];
  } else {  // control_allocation.py:103-114: force (0, 0, u), torque cq * force * (-dir) at every motor link, in the LINK's frame
    for (int j = 0; j < M; ++j) {
      const int b = R.body_of_motor[j];
      F[3 * b + 2] = u[j];
      T[3 * b] = (P.cq * 0.0f) * (-P.motor_dir[j]);
      T[3 * b + 1] = (P.cq * 0.0f) * (-P.motor_dir[j]);
      T[3 * b + 2] = (P.cq * u[j]) * (-P.motor_dir[j]);
    }
  }
  // simulate_drag (:260-285), then apply_disturbance (:213-234): both `+=` into body 0
  // (the same drag and disturbance arithmetic as in k_env_step, agx_dyn_env_step.h: written out in both)
  {
    if (ROV) {  // base_rov.py:260-272: -c_q[k] |v_body[k]| v_body[k], per axis
      F[0] += (-P.lin_drag_linear[0] * d.vbody.x) + (-P.lin_drag_quadratic[0] * fabsf(d.vbody.x) * d.vbody.x);
      F[1] += (-P.lin_drag_linear[1] * d.vbody.y) + (-P.lin_drag_quadratic[1] * fabsf(d.vbody.y) * d.vbody.y);
      F[2] += (-P.lin_drag_linear[2] * d.vbody.z) + (-P.lin_drag_quadratic[2] * fabsf(d.vbody.z) * d.vbody.z);
    } else {
      const float vbn = norm(d.vbody);
      F[0] += (-P.lin_drag_linear[0] * d.vbody.x) + (-P.lin_drag_quadratic[0] * vbn * d.vbody.x);
      F[1] += (-P.lin_drag_linear[1] * d.vbody.y) + (-P.lin_drag_quadratic[1] * vbn * d.vbody.y);
      F[2] += (-P.lin_drag_linear[2] * d.vbody.z) + (-P.lin_drag_quadratic[2] * vbn * d.vbody.z);
    }
    T[0] += (-P.ang_drag_linear[0] * d.wbody.x) + (-P.ang_drag_quadratic[0] * fabsf(d.wbody.x) * d.wbody.x);
    T[1] += (-P.ang_drag_linear[1] * d.wbody.y) + (-P.ang_drag_quadratic[1] * fabsf(d.wbody.y) * d.wbody.y);
    T[2] += (-P.ang_drag_linear[2] * d.wbody.z) + (-P.ang_drag_quadratic[2] * fabsf(d.wbody.z) * d.wbody.z);
  }
  float di[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  bool any = false;
  if (B.disturb) {  // draws supplied by the host ([k][7][N] rows of this sub-step)
    const float *dd = B.disturb + (size_t)R.substep * 7 * n + i;
    const float occ = dd[0];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const float lo = -B.disturb_max[c], hi = B.disturb_max[c];
      di[c] = ((hi - lo) * dd[(size_t)(1 + c) * n] + lo) * occ;
    }
    any = true;
  } else if (B.disturb_prob > 0.0f) {  // the device stream of the fused step: same (env, step, sub-step) -> same draws
    float ud[7];
    rng_fill<7>(B.rng_seed, B.env_index_base + i, agx::step_index(B), RNG_DISTURB + R.substep, ud);
    const float occ = ud[0] < B.disturb_prob ? 1.0f : 0.0f;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const float lo = -B.disturb_max[c], hi = B.disturb_max[c];
      di[c] = ((hi - lo) * ud[1 + c] + lo) * occ;
    }
    any = true;
  }
  if (any) {
    F[0] += di[0]; F[1] += di[1]; F[2] += di[2];
    T[0] += di[3]; T[1] += di[4]; T[2] += di[5];
  }
}

// robot_force_tensor / robot_torque_tensor -> the net body-frame wrench on the rigid composite (agx_net_body_wrench)
__global__ void __launch_bounds__(256) k_net_body_wrench(int n, AgxLinkFrames L, const float *__restrict__ force,
                                                         const float *__restrict__ torque, float *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int NB = L.num_bodies;
  const float *F = force + (size_t)i * NB * 3, *T = torque + (size_t)i * NB * 3;
  float w[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int b = 0; b < NB; ++b) {
    const float *Rm = L.rot[b], *r = L.pos[b];
    const float f[3] = {F[3 * b], F[3 * b + 1], F[3 * b + 2]}, t[3] = {T[3 * b], T[3 * b + 1], T[3 * b + 2]};
    float fr[3], tr[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      fr[c] = (Rm[3 * c] * f[0] + Rm[3 * c + 1] * f[1]) + Rm[3 * c + 2] * f[2];
      tr[c] = (Rm[3 * c] * t[0] + Rm[3 * c + 1] * t[1]) + Rm[3 * c + 2] * t[2];
    }
    const float cx = r[1] * fr[2] - r[2] * fr[1], cy = r[2] * fr[0] - r[0] * fr[2], cz = r[0] * fr[1] - r[1] * fr[0];
    w[0] += fr[0]; w[1] += fr[1]; w[2] += fr[2];
    w[3] += cx + tr[0]; w[4] += cy + tr[1]; w[5] += cz + tr[2];
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) out[(size_t)i * 6 + c] = w[c];
}
}  // namespace agx

extern "C" int agx_update_states(const AgxEnvBuffers *B, int n, void *stream) {
  if (int e = check_common(nullptr, B, n)) return e;
  AGX_REQUIRE(B->state && B->derived, "null env buffer");
  const int block = pick_block(n);
  if (B->launch_flags & AGX_LAUNCH_ROV)
    hipLaunchKernelGGL(k_update_states_rov, dim3(blocks_for(n, block)), dim3(block), 0, (hipStream_t)stream, *B, n);
  else
    hipLaunchKernelGGL(k_update_states, dim3(blocks_for(n, block)), dim3(block), 0, (hipStream_t)stream, *B, n);
  return check_launch("agx_update_states");
}

extern "C" int agx_collide_spheres_boxes(const AgxRobotParams *P, const AgxEnvBuffers *B, int n, void *stream) {
  AGX_REQUIRE(P && B, "bad arguments");
  if (int e = check_common(P, B, n)) return e;  // the n <= 2^26 bound the 32-bit SoaRef offsets of the kernel depend on
  AGX_REQUIRE(B->state && B->crashes, "null env buffer");
  if (!B->boxes || B->num_boxes <= 0) return AGX_OK;  // no obstacles: nothing can be hit
  hipLaunchKernelGGL(k_collide_spheres_boxes, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, *B, n, P->collision_radius);
  return check_launch("agx_collide_spheres_boxes");
}

extern "C" int agx_controller_wrench(const AgxRobotParams *P, const AgxEnvBuffers *B, int n, const float *action,
                                     void *stream) {
  if (int e = check_common(P, B, n)) return e;
  AGX_REQUIRE(P && P->controller != AGX_CTRL_NONE, "controller required");
  AGX_REQUIRE(action && B->state && B->derived && B->wrench_cmd, "null buffer");
  const int block = pick_block(n);
  hipLaunchKernelGGL(k_controller_wrench, dim3(blocks_for(n, block)), dim3(block), 0, (hipStream_t)stream, *P, *B, n, action);
  return check_launch("agx_controller_wrench");
}

extern "C" int agx_robot_step(const AgxRobotParams *P, const AgxEnvBuffers *B, int n, const float *action, const AgxRobotStepArgs *R,
                              void *stream) {
  if (int e = check_common(P, B, n)) return e;
  AGX_REQUIRE(P && R && action, "null argument");
  AGX_REQUIRE(P->controller != AGX_CTRL_WRENCH, "agx_robot_step evaluates a BUILT-IN controller (an external controller class is called by the host)");
  AGX_REQUIRE(B->state && B->derived && B->motor_thrust && R->force && R->torque, "null buffer");
  AGX_REQUIRE(!P->use_rps || B->motor_kT, "null motor_kT with use_rps");
  AGX_REQUIRE(R->num_bodies >= 1 && R->num_bodies <= AGX_MAX_BODIES, "num_bodies %d outside [1, %d]", R->num_bodies, AGX_MAX_BODIES);
  AGX_REQUIRE(R->substep >= 0 && R->substep < AGX_MAX_SUBSTEPS, "substep out of range");
  AGX_REQUIRE((long long)n * R->num_bodies * 3 < (1ll << 31), "per-body tensors too large for this entry point");
  for (int j = 0; j < (P->root_link_mode ? 1 : P->num_motors); ++j)
    AGX_REQUIRE(R->body_of_motor[j] >= 0 && R->body_of_motor[j] < R->num_bodies, "application mask entry %d = %d outside [0, %d)", j,
                R->body_of_motor[j], R->num_bodies);
  if (B->launch_flags & AGX_LAUNCH_ROV) {
    if (int e = check_rov(P, "agx_robot_step")) return e;
    hipLaunchKernelGGL(k_robot_step<true>, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, *P, *B, n, action, *R);
  } else {
    hipLaunchKernelGGL(k_robot_step<false>, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, *P, *B, n, action, *R);
  }
  return check_launch("agx_robot_step");
}

extern "C" int agx_net_body_wrench(int n, const AgxLinkFrames *L, const float *force, const float *torque, float *out, void *stream) {
  AGX_REQUIRE(n > 0 && L && force && torque && out, "bad arguments");
  AGX_REQUIRE(L->num_bodies >= 1 && L->num_bodies <= AGX_MAX_BODIES, "num_bodies %d outside [1, %d]", L->num_bodies, AGX_MAX_BODIES);
  hipLaunchKernelGGL(k_net_body_wrench, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, n, *L, force, torque, out);
  return check_launch("agx_net_body_wrench");
}
