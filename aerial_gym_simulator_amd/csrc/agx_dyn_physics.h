#pragma once
// Physics and controller device functions of one env on one lane: update_states, the Lee control laws and run_controller, the motor
// model, the rigid-body integrator, and the sphere / box collision predicate with its trajectory pass.
// Part of the one translation unit agx_dynamics.hip, which alone includes it (after the AGX_DYN_* switches).

namespace agx {
// BaseMultirotor.update_states, base_multirotor.py:287-294
AGX_DEV Derived update_states(const EnvState &s) {
  Derived d;
  V3 e = euler_xyz_0_2pi(s.q);
  d.euler = V3{ssa(e.x), ssa(e.y), ssa(e.z)};
  // vehicle_frame_quat_from_quat: euler * [0, 0, 1] (utils/math.py:176-180)
  d.qveh = quat_from_yaw(e.z * 1.0f);  // = quat_from_euler(e.x * 0, e.y * 0, e.z * 1), see agx_device_math.h
  d.vveh = quat_rotate_inverse(d.qveh, s.v);
  d.vbody = quat_rotate_inverse(s.q, s.v);
  d.wbody = quat_rotate_inverse(s.q, s.w);
  return d;
}

// BaseROV.update_states (base_rov.py:251-258; the robot kind AGX_LAUNCH_ROV): get_euler_xyz_tensor(q) is stored as it is, in
// [0, 2 pi), without ssa(); the rest is the same.  (The laws an ROV runs read no Euler angles: kLawReadsNoAngles in the env step.)
AGX_DEV Derived update_states_rov(const EnvState &s) {
  Derived d;
  V3 e = euler_xyz_0_2pi(s.q);
  d.euler = e;
  d.qveh = quat_from_yaw(e.z * 1.0f);
  d.vveh = quat_rotate_inverse(d.qveh, s.v);
  d.vbody = quat_rotate_inverse(s.q, s.v);
  d.wbody = quat_rotate_inverse(s.q, s.w);
  return d;
}

// The lean step (AGX_LAUNCH_LEAN) does not maintain Euler angles / vehicle-frame velocity, and under the laws that read neither
// (position, fully actuated; no controller) does not EVALUATE them either: roll and pitch are two of the three float64
// function evaluations of update_states.  What remains is what the task epilogue and the observation read, the same
// operations on the same operands: vehicle-frame quaternion (from the yaw), body-frame velocities.
AGX_DEV Derived update_states_lean(const EnvState &s) {
  Derived d{};
  d.qveh = quat_from_yaw(yaw_0_2pi(s.q) * 1.0f);
  d.vbody = quat_rotate_inverse(s.q, s.v);
  d.wbody = quat_rotate_inverse(s.q, s.w);
  return d;
}
// ... and the observation behind a reset reads the body-frame velocities only
AGX_DEV Derived update_states_body(const EnvState &s) {
  Derived d{};
  d.vbody = quat_rotate_inverse(s.q, s.v);
  d.wbody = quat_rotate_inverse(s.q, s.w);
  return d;
}

// base_lee_controller.py:120-134
// ZERO_VEL: the caller's velocity set-point is the constant 0 (position / fully actuated control): rotating it gives 0
template <bool ZERO_VEL = false>
AGX_DEV V3 compute_acceleration(const EnvState &s, Q4 qveh, V3 sp_pos, V3 sp_vel, const Gains &g) {
  V3 sp_vel_w = ZERO_VEL ? V3{0.0f, 0.0f, 0.0f} : quat_rotate(qveh, sp_vel);
  V3 pe = sp_pos - s.p;
  V3 ve = sp_vel_w - s.v;
  return V3{g.kp.x * pe.x + g.kv.x * ve.x, g.kp.y * pe.y + g.kv.y * ve.y, g.kp.z * pe.z + g.kv.z * ve.z};
}

// base_lee_controller.py:136-154 (sp_w.z is clamped in place by the caller-visible ref)
// ZERO_RATE: the caller's angular-velocity set-point is the constant 0
template <bool ZERO_RATE = false>
AGX_DEV V3 compute_body_torque(const AgxRobotParams &P, Q4 q, V3 wb, Q4 qd, V3 &sp_w, const Gains &g) {
  sp_w.z = fminf(fmaxf(sp_w.z, -P.max_yaw_rate), P.max_yaw_rate);
  Q4 qe = quat_mul(conj(q), qd);
  M33 R = quat_to_rotmat(qe);
  V3 rot_err = V3{0.5f * (-(R.m21 - R.m12)), 0.5f * (R.m20 - R.m02), 0.5f * (-(R.m10 - R.m01))};
  V3 wsp_b = ZERO_RATE ? V3{0.0f, 0.0f, 0.0f} : quat_rotate(qe, sp_w);
  V3 Jw = V3{P.inertia[0] * wb.x + P.inertia[1] * wb.y + P.inertia[2] * wb.z,
             P.inertia[3] * wb.x + P.inertia[4] * wb.y + P.inertia[5] * wb.z,
             P.inertia[6] * wb.x + P.inertia[7] * wb.y + P.inertia[8] * wb.z};
  V3 ff = cross(wb, Jw);
  V3 we = wb - wsp_b;
  return V3{-g.kr.x * rot_err.x - g.kw.x * we.x + ff.x, -g.kr.y * rot_err.y - g.kw.y * we.y + ff.y,
            -g.kr.z * rot_err.z - g.kw.z * we.z + ff.z};
}

// base_lee_controller.py:173-194
AGX_DEV Q4 desired_orientation_pos_vel(V3 f, float yaw) {
  V3 b3 = normalized(f);
  float sy, cy;
  sincos_bounded(yaw, sy, cy);
  V3 tmp = V3{cy, sy, 0.0f};
  V3 b2 = normalized(cross(b3, tmp));
  V3 b1 = cross(b2, b3);
  M33 R{b1.x, b2.x, b3.x, b1.y, b2.y, b3.y, b1.z, b2.z, b3.z};
  return rotmat_to_quat(R);
}

// base_lee_controller.py:158-169
AGX_DEV Q4 desired_orientation_forces_yaw(V3 f, float yaw) {
  float pitch = atan2_cw(f.x, f.z);
  float roll = atan2_cw(-f.y, sqrtf(f.z * f.z + f.x * f.x));
  return quat_from_euler(roll, pitch, yaw);
}

// base_lee_controller.py:201-215 (stale matrix entries only ever multiply zero rates)
AGX_DEV V3 euler_rates_to_body_rates(V3 euler, V3 r) {
  float sp, cp, sr, cr;
  sincos_bounded(euler.y, sp, cp);
  sincos_bounded(euler.x, sr, cr);
  return V3{1.0f * r.x + 0.0f * r.y + (-sp) * r.z, 0.0f * r.x + cr * r.y + (sr * cp) * r.z,
            0.0f * r.x + (-sr) * r.y + (cr * cp) * r.z};
}

// One env's controller (control/controllers/*.py).  a[] holds the +-10 clipped action and
// is mutated where the reference mutates it.
template <int CTRL>
AGX_DEV Wrench run_controller(const AgxRobotParams &P, const EnvState &s, const Derived &d, float (&a)[AGX_MAX_ACTIONS],
                              const Gains &g) {
  Wrench w{V3{0, 0, 0}, V3{0, 0, 0}};
  const V3 grav = V3{P.gravity[0], P.gravity[1], P.gravity[2]};
  const float m = P.mass;
  const V3 zero = V3{0, 0, 0};
  switch (CTRL) {
    case AGX_CTRL_POSITION: {  // position_control.py:20-51
      V3 acc = compute_acceleration<true>(s, d.qveh, V3{a[0], a[1], a[2]}, zero, g);
      V3 f = (acc - grav) * m;
      M33 R = quat_to_rotmat(s.q);
      w.f.z = f.x * R.m02 + f.y * R.m12 + f.z * R.m22;
      Q4 qd = desired_orientation_pos_vel(f, a[3]);
      V3 wsp = zero;
      w.t = compute_body_torque<true>(P, s.q, d.wbody, qd, wsp, g);
    } break;
    case AGX_CTRL_VELOCITY: {  // velocity_control.py:18-51
      V3 acc = compute_acceleration(s, d.qveh, s.p, V3{a[0], a[1], a[2]}, g);
      V3 f = (acc - grav) * m;
      M33 R = quat_to_rotmat(s.q);
      w.f.z = f.x * R.m02 + f.y * R.m12 + f.z * R.m22;
      Q4 qd = desired_orientation_pos_vel(f, d.euler.z);
      V3 wsp = euler_rates_to_body_rates(d.euler, V3{0, 0, a[3]});
      w.t = compute_body_torque(P, s.q, d.wbody, qd, wsp, g);
    } break;
    case AGX_CTRL_ATTITUDE: {  // attitude_control.py:16-43
      w.f.z = (a[0] + 1.0f) * m * norm(grav);
      V3 wsp = euler_rates_to_body_rates(d.euler, V3{0, 0, a[3]});
      Q4 qd = quat_from_euler(a[1], a[2], d.euler.z);
      w.t = compute_body_torque(P, s.q, d.wbody, qd, wsp, g);
    } break;
    case AGX_CTRL_RATES: {  // rates_control.py:16-30 (line 25's broadcast bug -> z component)
      w.f.z = (a[0] - grav.z) * m;
      V3 wsp = V3{a[1], a[2], a[3]};
      w.t = compute_body_torque(P, s.q, d.wbody, s.q, wsp, g);
      a[3] = wsp.z;  // in-place yaw-rate clamp
    } break;
    case AGX_CTRL_ACCELERATION: {  // acceleration_control.py:16-45
      V3 f = (V3{a[0], a[1], a[2]} - grav) * m;
      M33 R = quat_to_rotmat(s.q);
      w.f.z = f.x * R.m02 + f.y * R.m12 + f.z * R.m22;
      Q4 qd = desired_orientation_forces_yaw(f, d.euler.z);
      V3 wsp = euler_rates_to_body_rates(d.euler, V3{0, 0, a[3]});
      w.t = compute_body_torque(P, s.q, d.wbody, qd, wsp, g);
    } break;
    case AGX_CTRL_VEL_STEERING: {  // velocity_steeing_angle_controller.py:15-45
      V3 acc = compute_acceleration(s, d.qveh, s.p, V3{a[0], a[1], a[2]}, g);
      V3 f = (acc - grav) * m;
      M33 R = quat_to_rotmat(s.q);
      w.f.z = f.x * R.m02 + f.y * R.m12 + f.z * R.m22;
      Q4 qd = desired_orientation_pos_vel(f, a[3]);
      V3 wsp = euler_rates_to_body_rates(d.euler, zero);
      w.t = compute_body_torque(P, s.q, d.wbody, qd, wsp, g);
    } break;
    case AGX_CTRL_FULLY_ACTUATED: {  // fully_actuated_control.py:14-32
      float nq = sqrtf(a[3] * a[3] + a[4] * a[4] + a[5] * a[5] + a[6] * a[6]);
      nq = nq < 1e-9f ? 1e-9f : nq;
      a[3] = a[3] / nq; a[4] = a[4] / nq; a[5] = a[5] / nq; a[6] = a[6] / nq;
      V3 acc = compute_acceleration<true>(s, d.qveh, V3{a[0], a[1], a[2]}, zero, g);
      V3 f = (acc - grav) * m;
      w.f = quat_rotate_inverse(s.q, f);
      V3 wsp = zero;
      w.t = compute_body_torque<true>(P, s.q, d.wbody, Q4{a[3], a[4], a[5], a[6]}, wsp, g);
    } break;
    default: break;
  }
  return w;
}

// The control law as a run-time value: the plug-in kernels k_controller_wrench and k_robot_step only (none of them is hot; the env-step
// kernels are compiled per law).  No law for this id (none, external wrench): the zero wrench.
AGX_DEV Wrench run_controller_by_id(const AgxRobotParams &P, const EnvState &s, const Derived &d, float (&a)[AGX_MAX_ACTIONS],
                                    const Gains &g) {
  switch (P.controller) {
    case AGX_CTRL_POSITION: return run_controller<AGX_CTRL_POSITION>(P, s, d, a, g);
    case AGX_CTRL_VELOCITY: return run_controller<AGX_CTRL_VELOCITY>(P, s, d, a, g);
    case AGX_CTRL_ATTITUDE: return run_controller<AGX_CTRL_ATTITUDE>(P, s, d, a, g);
    case AGX_CTRL_RATES: return run_controller<AGX_CTRL_RATES>(P, s, d, a, g);
    case AGX_CTRL_ACCELERATION: return run_controller<AGX_CTRL_ACCELERATION>(P, s, d, a, g);
    case AGX_CTRL_VEL_STEERING: return run_controller<AGX_CTRL_VEL_STEERING>(P, s, d, a, g);
    case AGX_CTRL_FULLY_ACTUATED: return run_controller<AGX_CTRL_FULLY_ACTUATED>(P, s, d, a, g);
    default: return Wrench{V3{0, 0, 0}, V3{0, 0, 0}};
  }
}
// ... and its output as the env's six wrench_cmd columns
AGX_DEV void store_wrench_cmd(float *__restrict__ wrench_cmd, int n, int i, const Wrench &wc) {
  AGX_AT(wrench_cmd, 0) = wc.f.x; AGX_AT(wrench_cmd, 1) = wc.f.y; AGX_AT(wrench_cmd, 2) = wc.f.z;
  AGX_AT(wrench_cmd, 3) = wc.t.x; AGX_AT(wrench_cmd, 4) = wc.t.y; AGX_AT(wrench_cmd, 5) = wc.t.z;
}

// control/motor_model.py:88-250
AGX_DEV float clamp_minmax(float x, float lo, float hi) { return fmaxf(fminf(x, hi), lo); }
AGX_DEV float sgnf(float x) { return (x > 0.0f) ? 1.0f : ((x < 0.0f) ? -1.0f : 0.0f); }
AGX_DEV float motor_rate(float err, float mix, float max_rate) { return clamp_minmax(mix * err, -max_rate, max_rate); }
AGX_DEV float rk4_delta(float ref, float cur, float mix, float max_rate, float dt, float dt_over_6) {
  float k1 = motor_rate(ref - cur, mix, max_rate);
  float k2 = motor_rate(ref - (cur + 0.5f * dt * k1), mix, max_rate);
  float k3 = motor_rate(ref - (cur + 0.5f * dt * k2), mix, max_rate);
  float k4 = motor_rate(ref - (cur + dt * k3), mix, max_rate);
  return dt_over_6 * (k1 + 2.0f * k2 + 2.0f * k3 + k4);
}
AGX_DEV float motor_update(const AgxRobotParams &P, float ref, float cur, float kT, float tau_inc, float tau_dec) {
  const float dt = P.dt;
  ref = fminf(fmaxf(ref, P.min_thrust), P.max_thrust);
  float err = ref - cur;
  float tc = (sgnf(cur) * sgnf(err) < 0.0f) ? tau_dec : tau_inc;
  float mix = fdiv(1.0f, P.use_discrete_approximation ? dt + tc : tc);
  if (P.use_rps) {
    float cur_rpm = fsqrt(fdiv(cur, kT));
    float des_rpm = fsqrt(fdiv(ref, kT));
    if (P.integration_rk4)
      cur_rpm += rk4_delta(des_rpm, cur_rpm, mix, P.max_rate, dt, P.dt_over_6);
    else
      cur_rpm += motor_rate(des_rpm - cur_rpm, mix, P.max_rate) * dt;
    return kT * (cur_rpm * cur_rpm);
  }
  if (P.integration_rk4) return cur + rk4_delta(ref, cur, mix, P.max_rate, dt, P.dt_over_6);
  return cur + motor_rate(err, mix, P.max_rate) * dt;
}

// Rigid-body update replacing gym.simulate (PhysX): see DESIGN.md "integrator".
AGX_DEV void integrate(const AgxRobotParams &P, EnvState &s, V3 Fb, V3 Tb) {
  const float dt = P.dt;
  V3 Fw = quat_rotate(s.q, Fb);
  V3 wb = quat_rotate_inverse(s.q, s.w);
  V3 Jw = V3{P.inertia[0] * wb.x + P.inertia[1] * wb.y + P.inertia[2] * wb.z,
             P.inertia[3] * wb.x + P.inertia[4] * wb.y + P.inertia[5] * wb.z,
             P.inertia[6] * wb.x + P.inertia[7] * wb.y + P.inertia[8] * wb.z};
  V3 rhs = Tb - cross(wb, Jw);
  V3 dwb = V3{P.inertia_inv[0] * rhs.x + P.inertia_inv[1] * rhs.y + P.inertia_inv[2] * rhs.z,
              P.inertia_inv[3] * rhs.x + P.inertia_inv[4] * rhs.y + P.inertia_inv[5] * rhs.z,
              P.inertia_inv[6] * rhs.x + P.inertia_inv[7] * rhs.y + P.inertia_inv[8] * rhs.z};
  V3 wb_new = V3{wb.x + dt * dwb.x, wb.y + dt * dwb.y, wb.z + dt * dwb.z};
  V3 w_new = quat_rotate(s.q, wb_new);
  V3 v_new = V3{s.v.x + dt * fdiv(Fw.x, P.mass), s.v.y + dt * fdiv(Fw.y, P.mass), s.v.z + dt * fdiv(Fw.z, P.mass)};
  v_new = V3{v_new.x + P.gravity[0] * dt, v_new.y + P.gravity[1] * dt, v_new.z + P.gravity[2] * dt};
  float ml = fmaxf(1.0f - P.linear_damping * dt, 0.0f);
  float ma = fmaxf(1.0f - P.angular_damping * dt, 0.0f);
  v_new = v_new * ml;
  w_new = w_new * ma;
  float v2 = dot(v_new, v_new), w2 = dot(w_new, w_new);
  if (v2 > P.max_linear_velocity * P.max_linear_velocity) v_new = v_new * fdiv(P.max_linear_velocity, fsqrt(v2));
  if (w2 > P.max_angular_velocity * P.max_angular_velocity) w_new = w_new * fdiv(P.max_angular_velocity, fsqrt(w2));
  s.p = V3{s.p.x + v_new.x * dt, s.p.y + v_new.y * dt, s.p.z + v_new.z * dt};
  float wm2 = dot(w_new, w_new);
  if (wm2 != 0.0f) {
    float wm = fsqrt(wm2);
    float half = dt * wm * 0.5f;
    float sn, cs;
    sincos_bounded(half, sn, cs);  // |half| = dt |w| / 2 <= 0.5 (|w| <= 100 rad/s)
    float sc = fdiv(sn, wm);
    float x1 = w_new.x * sc, y1 = w_new.y * sc, z1 = w_new.z * sc;
    Q4 q = s.q;
    float rx = x1 * q.w + y1 * q.z - z1 * q.y;
    float ry = y1 * q.w + z1 * q.x - x1 * q.z;
    float rz = z1 * q.w + x1 * q.y - y1 * q.x;
    float rw = -(x1 * q.x) - y1 * q.y - z1 * q.z;
    rx += q.x * cs; ry += q.y * cs; rz += q.z * cs; rw += q.w * cs;
    float nn = fsqrt(rx * rx + ry * ry + rz * rz + rw * rw);
    s.q = Q4{fdiv(rx, nn), fdiv(ry, nn), fdiv(rz, nn), fdiv(rw, nn)};
  }
  s.v = v_new;
  s.w = w_new;
}

// ---- centre of mass off the base-link origin (k_env_step_com; DESIGN.md "integrator") ----
// The state keeps the reference's meaning: p, q the base-link frame, v the velocity of the mass centre, w the angular velocity.
// c: the composite's centre of mass in the base-link frame.
// The root body's entry of robot_force_tensor acts at the base-link origin, -c from the mass centre: about the mass centre its
// force F_root adds the torque (-c) x F_root = F_root x c.
AGX_DEV V3 com_root_torque(V3 F_root, V3 c) { return cross(F_root, c); }
// integrate() has moved the mass centre by v_new dt and turned the body about it from q0 to q1, and left p + v_new dt in p: the
// base-link origin is where the mass centre is minus R(q1) c, i.e. p + (R(q0) c - R(q1) c), component by component.
AGX_DEV V3 com_position_correction(V3 p, Q4 q0, Q4 q1, V3 c) {
  V3 a = quat_rotate(q0, c), b = quat_rotate(q1, c);
  return V3{p.x + (a.x - b.x), p.y + (a.y - b.y), p.z + (a.z - b.z)};
}

#pragma clang fp contract(off)  // everything below: one IEEE operation per + - * /

// sphere (robot collision sphere, quad.urdf:16) vs obstacle OBBs; replaces the PhysX
// contact-force test of env_manager.py:358-362.  The predicate uses only IEEE + - *
// (bit-reproducible, written out here so no contracted helper is inlined); the culling in
// front of it is conservative, so the flag is exact.
AGX_DEV bool sphere_hits_box(V3 p, V3 c, Q4 q, V3 h, float r2) {
  // quat_rotate_inverse(q, p - c), utils/math.py:340-347
  V3 v = V3{p.x - c.x, p.y - c.y, p.z - c.z};
  float s = 2.0f * (q.w * q.w) - 1.0f;
  V3 cr = V3{q.y * v.z - q.z * v.y, q.z * v.x - q.x * v.z, q.x * v.y - q.y * v.x};
  float d = q.x * v.x + q.y * v.y + q.z * v.z;
  V3 l = V3{v.x * s - cr.x * q.w * 2.0f + q.x * d * 2.0f, v.y * s - cr.y * q.w * 2.0f + q.y * d * 2.0f,
            v.z * s - cr.z * q.w * 2.0f + q.z * d * 2.0f};
  float ex = fabsf(l.x) - h.x, ey = fabsf(l.y) - h.y, ez = fabsf(l.z) - h.z;
  float d2 = 0.0f;
  if (ex > 0.0f) d2 += ex * ex;
  if (ey > 0.0f) d2 += ey * ey;
  if (ez > 0.0f) d2 += ez * ez;
  return d2 < r2;
}

// One pass over the env's K boxes for ALL k sub-step positions (kept in LDS,
// traj[(s*3+c)*bd + tid]): each box is fetched once per env step instead of once per sub-step,
// and boxes whose bounding sphere cannot reach the AABB of the k positions cost 4 loads.
AGX_DEV bool collide_trajectory(const float *__restrict__ boxes, int nb, int n, int i, const float *traj, int k, int bd,
                                int tid, V3 lo, V3 hi, float r) {
  bool hit = false;
  const float r2 = r * r;
  // the cull data (centre, bounding radius) of box b + 1 is fetched while box b is processed: with few envs the
  // loop is a chain of dependent HBM round trips otherwise (101 us at 256 envs x 106 boxes)
  const float *b0 = boxes + i;
  float ncx = 0.0f, ncy = 0.0f, ncz = 0.0f, nrad = 0.0f;
  if (nb > 0) { ncx = b0[0]; ncy = b0[(size_t)n]; ncz = b0[2 * (size_t)n]; nrad = b0[10 * (size_t)n]; }
  for (int b = 0; b < nb; ++b) {
    const float *bx = boxes + (size_t)b * 11 * n + i;
    V3 c = V3{ncx, ncy, ncz};
    float reach = nrad + r + 1.0e-3f;
    if (b + 1 < nb) {
      const float *bn = bx + (size_t)11 * n;
      ncx = bn[0]; ncy = bn[(size_t)n]; ncz = bn[2 * (size_t)n]; nrad = bn[10 * (size_t)n];
    }
    float dx = fmaxf(fmaxf(lo.x - c.x, c.x - hi.x), 0.0f);
    float dy = fmaxf(fmaxf(lo.y - c.y, c.y - hi.y), 0.0f);
    float dz = fmaxf(fmaxf(lo.z - c.z, c.z - hi.z), 0.0f);
    if (dx * dx + dy * dy + dz * dz > reach * reach) continue;
    Q4 q = Q4{bx[3 * (size_t)n], bx[4 * (size_t)n], bx[5 * (size_t)n], bx[6 * (size_t)n]};
    V3 h = V3{bx[7 * (size_t)n], bx[8 * (size_t)n], bx[9 * (size_t)n]};
    for (int s = 0; s < k; ++s) {
      V3 p = V3{traj[(s * 3 + 0) * bd + tid], traj[(s * 3 + 1) * bd + tid], traj[(s * 3 + 2) * bd + tid]};
      hit = hit || sphere_hits_box(p, c, q, h, r2);
    }
  }
  return hit;
}
}  // namespace agx
