#pragma once
// The four-lanes-per-env (lane quad) device functions and the sub-step loop kernel built from them, k_env_step_quad_loop.
// Part of the one translation unit agx_dynamics.hip, which alone includes it (after the AGX_DYN_* switches).

namespace agx {
// ---------------------------------------------------------------------------------------
// The one-sub-step env step of the Lee position controller on a quadrotor (BASELINE configs 1/2) with FOUR lanes per
// env (agx_quad_math.h): a wave carries 16 envs, 8192 envs are 512 waves on the 1024 SIMDs instead of 128, and a wave
// issues about half the vector instructions of the one-lane-per-env kernel.  Every value is produced by the same IEEE
// operations in the same order as in k_env_step<4, AGX_CTRL_POSITION, true, .>; the GPU parity tests run against the
// CPU restatement through this kernel.  Not covered (the launcher falls back to k_env_step): obstacles, drag, disturbances,
// split launches, other controllers / motor counts.
// ---------------------------------------------------------------------------------------
namespace q4 = quad;
AGX_DEV unsigned long long vote(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// BaseMultirotor.update_states (base_multirotor.py:287-294) of one env on its lane quad
struct QuadDerived {
  float euler, qveh, vveh, vbody, wbody;
};
// `extra` / `esn`, `ecs`: the half-yaw's sine and cosine are needed in lanes 2 and 3 only, so lanes 0 and 1 of the same
// evaluation take another angle of the caller's (the position law's yaw set-point) and hand back its sine / cosine
AGX_DEV QuadDerived update_states_quad(float q, float v, float w, float extra, float &esn, float &ecs) {
  const int l = q4::lane_in_quad();
  QuadDerived d;
  const float e = q4::euler_xyz_0_2pi(q);
  d.euler = ssa(e);
  float sy, cy;
  const float half_yaw = (q4::bc<2>(e) * 1.0f) * 0.5f;  // vehicle_frame_quat_from_quat: quat_from_yaw
  sincos_bounded(l < 2 ? extra : half_yaw, sy, cy);
  esn = sy;
  ecs = cy;
  d.qveh = l == 2 ? sy : (l == 3 ? cy : 0.0f);
  d.vveh = q4::quat_rotate_inverse(d.qveh, v);
  d.vbody = q4::quat_rotate_inverse(q, v);
  d.wbody = q4::quat_rotate_inverse(q, w);
  return d;
}
AGX_DEV QuadDerived update_states_quad(float q, float v, float w) {
  float sn, cs;
  return update_states_quad(q, v, w, 0.0f, sn, cs);
}

// Per-lane constants of the quad kernels: component l of a vector, row l of a matrix, motors l (and l + 4 of an 8-motor robot)
// (indexed kernel-argument loads)
template <int M>
struct QuadConsts {
  float grav, in0, in1, in2, ii0, ii1, ii2, pinv[M / 4][6], mapf[M], mapt[M], mass, dt;
};
// (S: where the scalar fields come from -- the position-step kernels hand in their pinned copy, see arg_pin; the indexed
// loads must stay on the kernel argument itself)
template <int M>
AGX_DEV QuadConsts<M> load_quad_consts(const AgxRobotParams &P, const AgxRobotParams &S, int l, int l3) {
  QuadConsts<M> C;
  C.grav = P.gravity[l3];
  C.in0 = P.inertia[3 * l3 + 0]; C.in1 = P.inertia[3 * l3 + 1]; C.in2 = P.inertia[3 * l3 + 2];
  C.ii0 = P.inertia_inv[3 * l3 + 0]; C.ii1 = P.inertia_inv[3 * l3 + 1]; C.ii2 = P.inertia_inv[3 * l3 + 2];
#pragma unroll
  for (int h = 0; h < M / 4; ++h)
#pragma unroll
    for (int c = 0; c < 6; ++c) C.pinv[h][c] = P.alloc_pinv[6 * (l + 4 * h) + c];  // motor l + 4 h
  const float *wmap = S.root_link_mode != 0 ? P.alloc : P.wrench_map;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    C.mapf[j] = wmap[M * l3 + j];        // force row l
    C.mapt[j] = wmap[M * (3 + l3) + j];  // torque row l
  }
  C.mass = S.mass;
  C.dt = S.dt;
  return C;
}
template <int M>
AGX_DEV QuadConsts<M> load_quad_consts(const AgxRobotParams &P, int l, int l3) {
  return load_quad_consts<M>(P, P, l, l3);
}
// f . third column of quat_to_rotmat(q) = (2 (xz + yw), 2 (yz - xw), 1 - 2 (xx + yy)): the thrust command of the Lee laws
AGX_DEV float quad_thrust_along_body_z(float q, float f, int l) {
  const float t1 = q * q4::bc<2>(q), t2 = q4::perm<1, 0, 2, 3>(q) * q4::bc<3>(q);
  const float c2a = 2.0f * (l == 1 ? t1 - t2 : t1 + t2);
  const float sqq = q * q;
  const float m22 = 1.0f - 2.0f * (q4::bc<0>(sqq) + q4::bc<1>(sqq));
  return q4::dot3(f, l == 2 ? m22 : c2a);
}
// base_lee_controller.py:173-194 (desired_orientation_pos_vel)
// (sy, cy: sine and cosine of the yaw set-point, each valid in the lane that uses it -- cy in lane 0, sy in lane 1)
AGX_DEV float quad_desired_orientation_pos_vel_sc(float f, float sy, float cy, int l) {
  const float b3 = fdiv(f, q4::norm3(f));
  const float tmp = l == 0 ? cy : (l == 1 ? sy : 0.0f);
  const float cb = q4::cross3(b3, tmp);
  const float b2 = fdiv(cb, q4::norm3(cb));
  const float b1 = q4::cross3(b2, b3);
  return q4::rotmat_cols_to_quat(b1, b2, b3);
}
AGX_DEV float quad_desired_orientation_pos_vel(float f, float yaw, int l) {
  float sy, cy;
  sincos_bounded(yaw, sy, cy);
  return quad_desired_orientation_pos_vel_sc(f, sy, cy, l);
}
// base_lee_controller.py:136-154 (compute_body_torque); ZERO_RATE: the angular-velocity set-point is the constant 0
template <bool ZERO_RATE, int M>
AGX_DEV float quad_body_torque(const QuadConsts<M> &C, float q, float qd, float wb, float wsp, float kr, float kw, int l) {
  const float qe = q4::quat_mul(q4::conj(q), qd);
  const float pp = q4::rot1(qe) * q4::rot2(qe);  // (yz, zx, xy)
  const float pw = qe * q4::bc<3>(qe);           // (xw, yw, zw)
  const float mp = 2.0f * (pp + pw);             // (m21, m02, m10)
  const float mm = 2.0f * (pp - pw);             // (m12, m20, m01)
  const float rot_err = 0.5f * (l == 1 ? mm - mp : -(mp - mm));
  const float jw = (C.in0 * q4::bc<0>(wb) + C.in1 * q4::bc<1>(wb)) + C.in2 * q4::bc<2>(wb);
  const float ff = q4::cross3(wb, jw);
  const float we = ZERO_RATE ? wb : wb - q4::quat_rotate(qe, wsp);
  return ((-kr) * rot_err - kw * we) + ff;
}
// allocation (lane l = motors l, l + 4) + motor model + body wrench (lane l = row l of the force / of the torque);
// `force`: the commanded body force, (0, 0, thrust) for the Lee laws
template <int M>
AGX_DEV void quad_allocate(const AgxRobotParams &P, const QuadConsts<M> &C, float force, float torque, float (&u)[M / 4],
                           const float (&kT)[M / 4], const float (&tinc)[M / 4], const float (&tdec)[M / 4], float &fb, float &tb) {
  const float w0 = q4::bc<0>(force), w1 = q4::bc<1>(force), w2 = q4::bc<2>(force);
  const float w3 = q4::bc<0>(torque), w4 = q4::bc<1>(torque), w5 = q4::bc<2>(torque);
#pragma unroll
  for (int h = 0; h < M / 4; ++h) {
    float r = 0.0f;
    r += C.pinv[h][0] * w0;
    r += C.pinv[h][1] * w1;
    r += C.pinv[h][2] * w2;
    r += C.pinv[h][3] * w3;
    r += C.pinv[h][4] * w4;
    r += C.pinv[h][5] * w5;
    u[h] = motor_update(P, r, u[h], kT[h], tinc[h], tdec[h]);
  }
  fb = 0.0f;
  tb = 0.0f;
#pragma unroll
  for (int h = 0; h < M / 4; ++h) {
    const float u0 = q4::bc<0>(u[h]), u1 = q4::bc<1>(u[h]), u2 = q4::bc<2>(u[h]), u3 = q4::bc<3>(u[h]);
    fb += C.mapf[4 * h + 0] * u0; fb += C.mapf[4 * h + 1] * u1; fb += C.mapf[4 * h + 2] * u2; fb += C.mapf[4 * h + 3] * u3;
    tb += C.mapt[4 * h + 0] * u0; tb += C.mapt[4 * h + 1] * u1; tb += C.mapt[4 * h + 2] * u2; tb += C.mapt[4 * h + 3] * u3;
  }
}
// the rigid-body update (integrate(), DESIGN.md "integrator") on the quad
template <int M>
AGX_DEV void quad_integrate(const AgxRobotParams &P, const QuadConsts<M> &C, float &p, float &q, float &v, float &w, float fb, float tb,
                            int l) {
  const float dt = C.dt;
  const float fw = q4::quat_rotate(q, fb);
  const float wbi = q4::quat_rotate_inverse(q, w);
  const float jwi = (C.in0 * q4::bc<0>(wbi) + C.in1 * q4::bc<1>(wbi)) + C.in2 * q4::bc<2>(wbi);
  const float rhs = tb - q4::cross3(wbi, jwi);
  const float dwb = (C.ii0 * q4::bc<0>(rhs) + C.ii1 * q4::bc<1>(rhs)) + C.ii2 * q4::bc<2>(rhs);
  const float wb_new = wbi + dt * dwb;
  float w_new = q4::quat_rotate(q, wb_new);
  float v_new = v + dt * fdiv(fw, C.mass);
  v_new = v_new + C.grav * dt;
  const float ml = fmaxf(1.0f - P.linear_damping * dt, 0.0f);
  const float ma = fmaxf(1.0f - P.angular_damping * dt, 0.0f);
  v_new = v_new * ml;
  w_new = w_new * ma;
  const float v2 = q4::dot3(v_new, v_new), w2 = q4::dot3(w_new, w_new);
  if (v2 > P.max_linear_velocity * P.max_linear_velocity) v_new = v_new * fdiv(P.max_linear_velocity, fsqrt(v2));
  if (w2 > P.max_angular_velocity * P.max_angular_velocity) w_new = w_new * fdiv(P.max_angular_velocity, fsqrt(w2));
  p = p + v_new * dt;
  const float wm2 = q4::dot3(w_new, w_new);
  if (wm2 != 0.0f) {
    const float wm = fsqrt(wm2);
    const float half = dt * wm * 0.5f;
    float sn, cs;
    sincos_bounded(half, sn, cs);
    const float sc = fdiv(sn, wm);
    const float x1 = w_new * sc;  // (x1, y1, z1)
    // (x1 w + y1 z - z1 y, y1 w + z1 x - x1 z, z1 w + x1 y - y1 x, -(x1 x) - y1 y - z1 z)
    const float r3 = (x1 * q4::bc<3>(q) + q4::rot1(x1) * q4::rot2(q)) - q4::rot2(x1) * q4::rot1(q);
    const float xq = x1 * q;
    const float rw = (-q4::bc<0>(xq) - q4::bc<1>(xq)) - q4::bc<2>(xq);
    float rq = l == 3 ? rw : r3;
    rq += q * cs;
    const float nn = fsqrt(q4::dot4(rq, rq));
    q = fdiv(rq, nn);
  }
  v = v_new;
  w = w_new;
}

// ---------------------------------------------------------------------------------------
// Four lanes per env for the sub-step LOOP (BASELINE configs 2 / 4, the LiDAR navigation task, the reference's default
// attitude-controlled position task): quadrotor, any of the six Lee laws, k sub-steps, obstacles, device disturbance
// draws, task epilogue.  Same contract as k_env_step_quad_position: per component the IEEE operations of
// k_env_step<4, CTRL, false, .> in the same order.  The obstacle test splits the env's boxes over the four lanes (the flag
// is a boolean OR: any order).
// ---------------------------------------------------------------------------------------
// base_lee_controller.py:201-215 on the quad: (1 0 -sp; 0 cr sr cp; 0 -sr cr cp) (0, 0, rz)
AGX_DEV float euler_rates_to_body_rates_quad(float euler, float rz) {
  const int l = q4::lane_in_quad();
  float sn, cs;
  sincos_bounded(euler, sn, cs);  // lane 0: roll, lane 1: pitch
  const float sr = q4::bc<0>(sn), cr = q4::bc<0>(cs), sp = q4::bc<1>(sn), cp = q4::bc<1>(cs);
  const float m0 = q4::by_lane(l, 1.0f, 0.0f, 0.0f);
  const float m1 = q4::by_lane(l, 0.0f, cr, -sr);
  const float m2 = q4::by_lane(l, -sp, sr * cp, cr * cp);
  return (m0 * 0.0f + m1 * 0.0f) + m2 * rz;
}
// utils/math.py:156-172 (quat_from_euler_xyz) with (roll, pitch, yaw) in lanes 0..2 of `ang`
AGX_DEV float quat_from_euler_quad(float ang) {
  const int l = q4::lane_in_quad();
  float sn, cs;
  sincos_bounded(ang * 0.5f, sn, cs);
  const float sr = q4::bc<0>(sn), cr = q4::bc<0>(cs), sp = q4::bc<1>(sn), cp = q4::bc<1>(cs), sy = q4::bc<2>(sn), cy = q4::bc<2>(cs);
  // x: cy sr cp - sy cr sp   y: cy cr sp + sy sr cp   z: sy cr cp - cy sr sp   w: cy cr cp + sy sr sp
  const float a1 = l == 2 ? sy : cy, b1 = l == 0 ? sr : cr, c1 = l == 1 ? sp : cp;
  const float a2 = l == 2 ? cy : sy, b2 = l == 0 ? cr : sr, c2 = l == 1 ? cp : sp;
  const float t1 = a1 * b1 * c1, t2 = a2 * b2 * c2;
  return (l == 0 || l == 2) ? t1 - t2 : t1 + t2;
}

// One env's control law on its lane quad (control/controllers/*.py; run_controller<CTRL> above is the one-lane form):
// commanded body force ((0, 0, thrust) for the Lee laws) and body torque from the clipped action `a` (a0..a3 in lanes 0..3;
// the fully actuated law: position set-point in `a`, orientation set-point xyzw in `a2`).
template <int CTRL, int M>
AGX_DEV void quad_controller(const AgxRobotParams &P, const QuadConsts<M> &C, float p, float q, float v, const QuadDerived &d, float a,
                             float a2, float kp, float kv, float kr, float kw, int l, float &force, float &torque) {
  const float yaw = q4::bc<2>(d.euler);
  float fz = 0.0f;
  if (CTRL == AGX_CTRL_FULLY_ACTUATED) {  // fully_actuated_control.py:14-32
    float nq = sqrtf(q4::dot4(a2, a2));
    nq = nq < 1e-9f ? 1e-9f : nq;
    const float qd = a2 / nq;
    const float acc = kp * (a - p) + kv * (0.0f - v);
    const float f = (acc - C.grav) * C.mass;
    force = q4::quat_rotate_inverse(q, f);
    torque = quad_body_torque<true>(C, q, qd, d.wbody, 0.0f, kr, kw, l);
    return;
  }
  if (CTRL == AGX_CTRL_POSITION || CTRL == AGX_CTRL_VELOCITY || CTRL == AGX_CTRL_VEL_STEERING) {
    float acc;
    if (CTRL == AGX_CTRL_POSITION) {  // position_control.py:20-51: kp (sp - p) + kv (0 - v)
      acc = kp * (a - p) + kv * (0.0f - v);
    } else {  // velocity_control.py:18-51, velocity_steeing_angle_controller.py:15-45: set-point = the current position
      const float sp_vel_w = q4::quat_rotate(d.qveh, a);  // (a0, a1, a2) in the vehicle frame
      acc = kp * (p - p) + kv * (sp_vel_w - v);
    }
    const float f = (acc - C.grav) * C.mass;
    fz = quad_thrust_along_body_z(q, f, l);
    const float qd = quad_desired_orientation_pos_vel(f, CTRL == AGX_CTRL_VELOCITY ? yaw : q4::bc<3>(a), l);
    if (CTRL == AGX_CTRL_POSITION) {
      torque = quad_body_torque<true>(C, q, qd, d.wbody, 0.0f, kr, kw, l);
    } else {
      float wsp = euler_rates_to_body_rates_quad(d.euler, CTRL == AGX_CTRL_VELOCITY ? q4::bc<3>(a) : 0.0f);
      if (l == 2) wsp = fminf(fmaxf(wsp, -P.max_yaw_rate), P.max_yaw_rate);
      torque = quad_body_torque<false>(C, q, qd, d.wbody, wsp, kr, kw, l);
    }
  } else if (CTRL == AGX_CTRL_ACCELERATION) {  // acceleration_control.py:16-45
    const float f = (a - C.grav) * C.mass;
    fz = quad_thrust_along_body_z(q, f, l);
    // desired_orientation_forces_yaw(f, yaw): pitch = atan2(f.x, f.z), roll = atan2(-f.y, sqrt(f.z^2 + f.x^2))
    const float fx = q4::bc<0>(f), fy = q4::bc<1>(f), fzc = q4::bc<2>(f);
    const float num = q4::by_lane(l, -fy, fx, 0.0f);
    const float den = q4::by_lane(l, sqrtf(fzc * fzc + fx * fx), fzc, 1.0f);
    const float ang = atan2_cw(num, den);
    const float qd = quat_from_euler_quad(l == 2 ? yaw : ang);
    float wsp = euler_rates_to_body_rates_quad(d.euler, q4::bc<3>(a));
    if (l == 2) wsp = fminf(fmaxf(wsp, -P.max_yaw_rate), P.max_yaw_rate);
    torque = quad_body_torque<false>(C, q, qd, d.wbody, wsp, kr, kw, l);
  } else if (CTRL == AGX_CTRL_ATTITUDE) {  // attitude_control.py:16-43
    const float g0 = P.gravity[0], g1 = P.gravity[1], g2 = P.gravity[2];
    fz = (q4::bc<0>(a) + 1.0f) * C.mass * norm(V3{g0, g1, g2});  // torch.norm(gravity)
    float wsp = euler_rates_to_body_rates_quad(d.euler, q4::bc<3>(a));
    if (l == 2) wsp = fminf(fmaxf(wsp, -P.max_yaw_rate), P.max_yaw_rate);
    const float qd = quat_from_euler_quad(q4::by_lane(l, q4::bc<1>(a), q4::bc<2>(a), yaw));
    torque = quad_body_torque<false>(C, q, qd, d.wbody, wsp, kr, kw, l);
  } else {  // AGX_CTRL_RATES: rates_control.py:16-30 (line 25's broadcast bug -> z component)
    fz = (q4::bc<0>(a) - P.gravity[2]) * C.mass;
    float wsp = q4::perm<1, 2, 3, 3>(a);  // (a1, a2, a3)
    if (l == 2) wsp = fminf(fmaxf(wsp, -P.max_yaw_rate), P.max_yaw_rate);
    torque = quad_body_torque<false>(C, q, q, d.wbody, wsp, kr, kw, l);
  }
  force = l == 2 ? fz : 0.0f;
}

template <int M, int CTRL>
__global__ void __launch_bounds__(64, 1)
    k_env_step_quad_loop(AgxRobotParams P, AgxEnvBuffers B, int n, const float *__restrict__ actions_in, int k, AgxTaskArgs T) {
  static_assert((M == 4 && CTRL >= AGX_CTRL_POSITION && CTRL <= AGX_CTRL_VEL_STEERING) ||
                    (M == 8 && (CTRL == AGX_CTRL_FULLY_ACTUATED || CTRL == AGX_CTRL_POSITION || CTRL == AGX_CTRL_VELOCITY)),
                "the six Lee laws of the quadrotor; the octarotor (two motors per lane) under its three laws: fully actuated, Lee "
                "position, Lee velocity (control/__init__.py:94-96)");
  constexpr bool FA = CTRL == AGX_CTRL_FULLY_ACTUATED;  // 7 actions: position set-point (3) + orientation set-point xyzw (4)
  constexpr int A = FA ? 7 : 4;
  constexpr int MH = M / 4;
  extern __shared__ float traj[];  // [k][3][16] sub-step positions of the wave's 16 envs (only with obstacles)
  const int tid = threadIdx.x;
  const int l = tid & 3, l3 = l < 3 ? l : 2, slot = tid >> 2;
  const int i = blockIdx.x * 16 + slot;
  const unsigned ol = ((unsigned)l * (unsigned)n + (unsigned)i) * 4u, ol3 = ((unsigned)l3 * (unsigned)n + (unsigned)i) * 4u;  // AGX_QAT
  bool reset = false;
  if (blockIdx.x == 0) push_publish_previous(B);  // peer push: the previous step's rows have landed everywhere
  const uint32_t push_peek = blockIdx.x == 0 ? push_wait_peek(B) : 0u;  // ... and this step's slot: looked at when the kernel is done
  if (i < n) {
    float p = AGX_QAT(B.state, 0, ol3), q = AGX_QAT(B.state, 3, ol), v = AGX_QAT(B.state, 7, ol3), w = AGX_QAT(B.state, 10, ol3);
    float u[MH], kT[MH], tinc[MH], tdec[MH];
#pragma unroll
    for (int h = 0; h < MH; ++h) {  // motors l and l + 4
      u[h] = AGX_QAT(B.motor_thrust, 4 * h, ol);
      kT[h] = P.use_rps ? AGX_QAT(B.motor_kT, 4 * h, ol) : 1.0f;
      tinc[h] = B.motor_tau_inc ? AGX_QAT(B.motor_tau_inc, 4 * h, ol) : P.tau_inc_uniform;
      tdec[h] = B.motor_tau_dec ? AGX_QAT(B.motor_tau_dec, 4 * h, ol) : P.tau_dec_uniform;
    }
    const float a_in = actions_in[(size_t)i * A + l];  // (a0 .. a3); fully actuated: position set-point in lanes 0..2
    const float a_old = AGX_QAT(B.actions, 0, ol);
    const float a_in2 = FA ? actions_in[(size_t)i * A + 3 + l] : 0.0f;  // fully actuated: orientation set-point xyzw
    const float a_old2 = FA ? AGX_QAT(B.actions, 3, ol) : 0.0f;
    const float kp = B.gains ? AGX_QAT(B.gains, 0, ol3) : P.gains_uniform[0 + l3];
    const float kv = B.gains ? AGX_QAT(B.gains, 3, ol3) : P.gains_uniform[3 + l3];
    const float kr = B.gains ? AGX_QAT(B.gains, 6, ol3) : P.gains_uniform[6 + l3];
    const float kw = B.gains ? AGX_QAT(B.gains, 9, ol3) : P.gains_uniform[9 + l3];
    const QuadConsts<M> C = load_quad_consts<M>(P, l, l3);
    // what the epilogue reads, requested with the state (see k_env_step: a load behind the stores is a round trip of its own)
    const int steps_in = B.sim_steps[i];
    const float tgt = T.kind != AGX_TASK_NONE ? AGX_QAT(T.target, 0, ol3) : 0.0f;
    const float ppe = (T.kind != AGX_TASK_NONE && T.kind != AGX_TASK_POSITION) ? AGX_QAT(T.pos_err, 0, ol3) : 0.0f;
    const float a_prev_in = k == 0 ? AGX_QAT(B.prev_actions, 0, ol) : 0.0f;
    const float a_prev_in2 = (FA && k == 0) ? AGX_QAT(B.prev_actions, 3, ol) : 0.0f;
    const float dmax = B.disturb_max[l3], dmax_t = B.disturb_max[3 + l3];
    const float a = clamp_minmax(a_in, -10.0f, 10.0f);  // clip_actions (the same every sub-step)
    const float a2 = clamp_minmax(a_in2, -10.0f, 10.0f);
    // Obstacles: lane l tests boxes l, l + 4, ...  The cull data (centre, bounding radius) of kBoxBatch of them is requested in
    // ONE go -- a box per loop trip was a dependent memory round trip per trip (27 of them on BASELINE configs[2], with one wave
    // per SIMD and nothing to hide them behind) -- and the first batch before the sub-step loop, whose arithmetic covers it.
    constexpr int kBoxBatch = M == 8 ? 12 : 16;  // (4 x 16 registers held over the sub-step loop; the octarotor instances stay <= 256 VGPRs)
    struct BoxCull { float cx[kBoxBatch], cy[kBoxBatch], cz[kBoxBatch], rad[kBoxBatch]; };
    const int nb = (B.boxes && k > 0) ? B.num_boxes : 0;
    auto load_cull = [&](int b0, BoxCull &K) {
#pragma unroll
      for (int u = 0; u < kBoxBatch; ++u) {
        const int b = b0 + 4 * u;
        const float *bx = B.boxes + (size_t)(b < nb ? b : b0) * 11 * n + i;  // past the end: this lane's first box again, not used
        K.cx[u] = bx[0]; K.cy[u] = bx[(size_t)n]; K.cz[u] = bx[2 * (size_t)n]; K.rad[u] = bx[10 * (size_t)n];
      }
    };
    BoxCull cull0{};
    if (l < nb) load_cull(l, cull0);
    QuadDerived d{};
    float force = 0.0f, torque = 0.0f, fb = 0.0f;
    float tlo = p, thi = p;
    for (int sub = 0; sub < k; ++sub) {
      d = update_states_quad(q, v, w);
      quad_controller<CTRL>(P, C, p, q, v, d, a, a2, kp, kv, kr, kw, l, force, torque);
      // ---- allocation + motor model + body wrench
      float tb;
      quad_allocate<M>(P, C, force, torque, u, kT, tinc, tdec, fb, tb);
      if (B.disturb) {  // apply_disturbance (base_multirotor.py:213-234), draws supplied by the host
        const float *dd = B.disturb + (size_t)sub * 7 * n + i;
        const float occ = dd[0];
        fb += ((dmax - (-dmax)) * dd[(size_t)(1 + l3) * n] + (-dmax)) * occ;
        tb += ((dmax_t - (-dmax_t)) * dd[(size_t)(4 + l3) * n] + (-dmax_t)) * occ;
      } else if (B.disturb_prob > 0.0f) {  // same, drawn in place (every lane of the quad draws the env's 7 uniforms)
        float ud[7];
        rng_fill<7>(B.rng_seed, B.env_index_base + i, agx::step_index(B), RNG_DISTURB + sub, ud);
        const float occ = ud[0] < B.disturb_prob ? 1.0f : 0.0f;
        fb += ((dmax - (-dmax)) * q4::by_lane(l3, ud[1], ud[2], ud[3]) + (-dmax)) * occ;
        tb += ((dmax_t - (-dmax_t)) * q4::by_lane(l3, ud[4], ud[5], ud[6]) + (-dmax_t)) * occ;
      }
      quad_integrate(P, C, p, q, v, w, fb, tb, l);
      if (B.boxes) {
        if (l < 3) traj[(sub * 3 + l) * 16 + slot] = p;
        if (sub == 0) { tlo = p; thi = p; }
        tlo = fminf(tlo, p);
        thi = fmaxf(thi, p);
      }
    }
    if (B.body_force && l < 3 && k > 0) AGX_QAT(B.body_force, 0, ol) = fb;
    // ---- obstacles: the env's boxes over the four lanes
    bool crashed = false;
    if (B.boxes && k > 0) {
      const V3 lo = V3{q4::bc<0>(tlo), q4::bc<1>(tlo), q4::bc<2>(tlo)}, hi = V3{q4::bc<0>(thi), q4::bc<1>(thi), q4::bc<2>(thi)};
      const float rad = P.collision_radius, r2 = rad * rad;
      bool hit = false;
      auto test_batch = [&](int b0, const BoxCull &K) {
#pragma unroll
        for (int u = 0; u < kBoxBatch; ++u) {
          const int b = b0 + 4 * u;
          const V3 c = V3{K.cx[u], K.cy[u], K.cz[u]};
          const float reach = K.rad[u] + rad + 1.0e-3f;
          const float dx = fmaxf(fmaxf(lo.x - c.x, c.x - hi.x), 0.0f);
          const float dy = fmaxf(fmaxf(lo.y - c.y, c.y - hi.y), 0.0f);
          const float dz = fmaxf(fmaxf(lo.z - c.z, c.z - hi.z), 0.0f);
          if (b < nb && !(dx * dx + dy * dy + dz * dz > reach * reach)) {  // (rare: the boxes the trajectory's AABB reaches)
            const float *bx = B.boxes + (size_t)b * 11 * n + i;
            const Q4 bq = Q4{bx[3 * (size_t)n], bx[4 * (size_t)n], bx[5 * (size_t)n], bx[6 * (size_t)n]};
            const V3 bh = V3{bx[7 * (size_t)n], bx[8 * (size_t)n], bx[9 * (size_t)n]};
            for (int sub = 0; sub < k; ++sub) {
              const V3 ps = V3{traj[(sub * 3 + 0) * 16 + slot], traj[(sub * 3 + 1) * 16 + slot], traj[(sub * 3 + 2) * 16 + slot]};
              hit = hit || sphere_hits_box(ps, c, bq, bh, r2);
            }
          }
        }
      };
      if (l < nb) test_batch(l, cull0);
      for (int b0 = l + 4 * kBoxBatch; b0 < nb; b0 += 4 * kBoxBatch) {
        BoxCull K;
        load_cull(b0, K);
        test_batch(b0, K);
      }
      crashed = ((vote(hit) >> (tid & 60)) & 0xFull) != 0ull;
    }
    // ---- stores
    if (l < 3) AGX_QAT(B.state, 0, ol) = p;
    AGX_QAT(B.state, 3, ol) = q;
    if (l < 3) {
      AGX_QAT(B.state, 7, ol) = v;
      AGX_QAT(B.state, 10, ol) = w;
    }
    if (k > 0) {
      if (l < 3) {
        AGX_QAT(B.derived, 0, ol) = d.euler;
        AGX_QAT(B.derived, 7, ol) = d.vveh;
        AGX_QAT(B.derived, 10, ol) = d.vbody;
        AGX_QAT(B.derived, 13, ol) = d.wbody;
      }
      AGX_QAT(B.derived, 3, ol) = d.qveh;
#pragma unroll
      for (int h = 0; h < MH; ++h) AGX_QAT(B.motor_thrust, 4 * h, ol) = u[h];
      if (B.wrench_cmd && l < 3) {
        AGX_QAT(B.wrench_cmd, 0, ol) = force;
        AGX_QAT(B.wrench_cmd, 3, ol) = torque;
      }
      // RobotManagerIGE.pre_physics_step runs every sub-step: prev <- cur, cur <- action
      if (!FA || l < 3) {
        AGX_QAT(B.prev_actions, 0, ol) = k >= 2 ? a_in : a_old;
        AGX_QAT(B.actions, 0, ol) = a_in;
      }
      if (FA) {
        AGX_QAT(B.prev_actions, 3, ol) = k >= 2 ? a_in2 : a_old2;
        AGX_QAT(B.actions, 3, ol) = a_in2;
      }
    }
    // ---- EnvManager bookkeeping + task epilogue (scalar code, the same in the four lanes; lane 0 stores)
    const float acur = k > 0 ? a_in : a_old;
    const float aprev = k >= 2 ? a_in : (k == 1 ? a_old : a_prev_in);
    // action component 3 as the navigation reward reads it: a3, or the first orientation component of the 7-D command
    const float acur3 = FA ? q4::bc<0>(k > 0 ? a_in2 : a_old2) : q4::bc<3>(acur);
    const float aprev3 = FA ? q4::bc<0>(k >= 2 ? a_in2 : (k == 1 ? a_old2 : a_prev_in2)) : q4::bc<3>(aprev);
    const int steps = steps_in + 1;
    bool trunc = false;
    float rew = 0.0f;
    if (T.kind != AGX_TASK_NONE) {
      if (T.kind == AGX_TASK_POSITION) {
        EnvState s;
        s.p = V3{q4::bc<0>(p), q4::bc<1>(p), q4::bc<2>(p)};
        s.q = Q4{q4::bc<0>(q), q4::bc<1>(q), q4::bc<2>(q), q4::bc<3>(q)};
        s.v = V3{0, 0, 0};
        s.w = V3{0, 0, 0};
        rew = reward_position(s, Q4{q4::bc<0>(d.qveh), q4::bc<1>(d.qveh), q4::bc<2>(d.qveh), q4::bc<3>(d.qveh)},
                              V3{q4::bc<0>(d.wbody), q4::bc<1>(d.wbody), q4::bc<2>(d.wbody)},
                              V3{q4::bc<0>(tgt), q4::bc<1>(tgt), q4::bc<2>(tgt)}, crashed);
      } else {
        const float pe = q4::quat_rotate_inverse(d.qveh, tgt - p);
        if (l < 3) {
          AGX_QAT(T.prev_pos_err, 0, ol) = ppe;
          AGX_QAT(T.pos_err, 0, ol) = pe;
        }
        rew = reward_navigation(T.rp, T.curriculum_progress, V3{q4::bc<0>(pe), q4::bc<1>(pe), q4::bc<2>(pe)},
                                V3{q4::bc<0>(ppe), q4::bc<1>(ppe), q4::bc<2>(ppe)}, q4::bc<0>(acur), q4::bc<2>(acur), acur3,
                                q4::bc<0>(aprev), q4::bc<2>(aprev), aprev3, crashed);
      }
      trunc = steps > T.episode_len;
      reset = (crashed && T.reset_on_collision) || trunc;
      if (T.successes)  // (wave-uniform; lane 0 of the env's quad stores)
        nav_bookkeeping_epilogue(T, i, l == 0, V3{q4::bc<0>(tgt), q4::bc<1>(tgt), q4::bc<2>(tgt)}, V3{q4::bc<0>(p), q4::bc<1>(p), q4::bc<2>(p)},
                                 crashed, trunc);
    }
    if (l == 0) {
      B.sim_steps[i] = steps;
      if (T.kind != AGX_TASK_NONE) {
        T.reward[i] = rew;
        B.reset_mask[i] = reset ? 1 : 0;
      }
      B.crashes[i] = crashed ? 1 : 0;
      B.truncations[i] = trunc ? 1 : 0;
    }
  }
  if (T.kind != AGX_TASK_NONE && __ballot(reset) != 0ull && (tid & 63) == 0) atomicOr(B.reset_flag + B.flag_parity, 1);
  if (blockIdx.x == 0) push_wait_finish(B, push_peek);
}
}  // namespace agx
