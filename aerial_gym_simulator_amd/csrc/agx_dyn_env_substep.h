// ONE physics sub-step of the one-lane env-step kernels: the statements inside `for (int sub = 0; sub < k; ++sub) { ... }` of
// agx_dyn_env_step_body.h (k_env_step, k_env_step_rov, k_env_step_com) and of k_env_step_rollout (agx_dyn_rollout.h), included INSIDE
// that loop and nowhere else; no include guard on purpose.  Shared as text, not as a device function, for the reason the step body
// gives: every instance compiles from the statements it was compiled from before, to the same instructions.  The including loop
// provides P, B, n, i, k, sub, s, d, u / kT / tinc / tdec, a_in, g, wc, root_link, has_drag, sub_base, lean, traj / bd / tid,
// tlo / thi and the constants M, CTRL, EXT, ROV, COM, kLawReadsNoAngles and the vector `com`.
      d = (kLawReadsNoAngles && lean) ? update_states_lean(s) : (ROV ? update_states_rov(s) : update_states(s));
      float a[AGX_MAX_ACTIONS];
#pragma unroll
      for (int c = 0; c < AGX_MAX_ACTIONS; ++c) a[c] = clamp_minmax(a_in[c], -10.0f, 10.0f);  // clip_actions
      // EXTERNAL ROBOT (AGX_LAUNCH_BODY_WRENCH, host-evaluated robot.step()): actions_in is the net body wrench itself
      const bool body_wrench = EXT && (B.launch_flags & AGX_LAUNCH_BODY_WRENCH) != 0;  // wave-uniform
      if (CTRL == AGX_CTRL_NONE) {
#pragma unroll
        for (int j = 0; j < M; ++j) u[j] = motor_update(P, a[j], u[j], kT[j], tinc[j], tdec[j]);
      } else if (!body_wrench) {
        if (EXT) wc = Wrench{V3{a_in[0], a_in[1], a_in[2]}, V3{a_in[3], a_in[4], a_in[5]}};  // as handed in, not clipped
      else wc = run_controller<CTRL>(P, s, d, a, g);
        const float w6[6] = {wc.f.x, wc.f.y, wc.f.z, wc.t.x, wc.t.y, wc.t.z};
#pragma unroll
        for (int j = 0; j < M; ++j) {
          float r = 0.0f;
#pragma unroll
          for (int c = 0; c < 6; ++c) r += P.alloc_pinv[6 * j + c] * w6[c];
          u[j] = motor_update(P, r, u[j], kT[j], tinc[j], tdec[j]);
        }
      }
      float bw[6];
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < M; ++j) acc += (root_link ? P.alloc[M * r + j] : P.wrench_map[M * r + j]) * u[j];
        bw[r] = body_wrench ? a_in[r] : acc;
      }
      // The ROOT link's entry of robot_force / robot_torque_tensor: the allocator's wrench in root-link mode, else 0.
      // simulate_drag (base_multirotor.py:260-285; pre-physics body velocities) and apply_disturbance (:213-234) accumulate
      // into it with `+=`, in that order; the net wrench on the rigid composite is the motor links' sum plus that entry.  So
      // with forces at the motor links, drag AND disturbance are summed first and added to the links' sum once (`root`);
      // with one of the two, or in root-link mode, that is the running sum below.  All-zero drag coefficients (base
      // quadrotor) add +-0 to every component: skipped (a scalar test of kernel arguments).
      // (The same drag and disturbance arithmetic as in k_robot_step, agx_dyn_robot.h: written out in both)
      const bool any_dist = !body_wrench && (B.disturb != nullptr || B.disturb_prob > 0.0f);
      const bool split_root = !root_link && has_drag && any_dist;  // wave-uniform
      float dr[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, di[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      if (has_drag) {
        if (ROV) {  // base_rov.py:260-272: -c_q[k] |v_body[k]| v_body[k], per axis
          dr[0] = (-P.lin_drag_linear[0] * d.vbody.x) + (-P.lin_drag_quadratic[0] * fabsf(d.vbody.x) * d.vbody.x);
          dr[1] = (-P.lin_drag_linear[1] * d.vbody.y) + (-P.lin_drag_quadratic[1] * fabsf(d.vbody.y) * d.vbody.y);
          dr[2] = (-P.lin_drag_linear[2] * d.vbody.z) + (-P.lin_drag_quadratic[2] * fabsf(d.vbody.z) * d.vbody.z);
        } else {
          float vbn = norm(d.vbody);
          dr[0] = (-P.lin_drag_linear[0] * d.vbody.x) + (-P.lin_drag_quadratic[0] * vbn * d.vbody.x);
          dr[1] = (-P.lin_drag_linear[1] * d.vbody.y) + (-P.lin_drag_quadratic[1] * vbn * d.vbody.y);
          dr[2] = (-P.lin_drag_linear[2] * d.vbody.z) + (-P.lin_drag_quadratic[2] * vbn * d.vbody.z);
        }
        dr[3] = (-P.ang_drag_linear[0] * d.wbody.x) + (-P.ang_drag_quadratic[0] * fabsf(d.wbody.x) * d.wbody.x);
        dr[4] = (-P.ang_drag_linear[1] * d.wbody.y) + (-P.ang_drag_quadratic[1] * fabsf(d.wbody.y) * d.wbody.y);
        dr[5] = (-P.ang_drag_linear[2] * d.wbody.z) + (-P.ang_drag_quadratic[2] * fabsf(d.wbody.z) * d.wbody.z);
      }
      if (B.disturb) {  // draws supplied by the host
        const float *dd = B.disturb + (size_t)(sub_base + sub) * 7 * n + i;
        float occ = dd[0];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          float lo = -B.disturb_max[c], hi = B.disturb_max[c];
          di[c] = ((hi - lo) * dd[(size_t)(1 + c) * n] + lo) * occ;
        }
      } else if (B.disturb_prob > 0.0f) {  // same, drawn in place: 7 uniforms per env and sub-step
        float ud[7];
        rng_fill<7>(B.rng_seed, B.env_index_base + i, agx::step_index(B), RNG_DISTURB + sub_base + sub, ud);
        float occ = ud[0] < B.disturb_prob ? 1.0f : 0.0f;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          float lo = -B.disturb_max[c], hi = B.disturb_max[c];
          di[c] = ((hi - lo) * ud[1 + c] + lo) * occ;
        }
      }
      if (!body_wrench && (has_drag || any_dist)) {  // an absent term is +0: x + 0 = x
#pragma unroll
        for (int c = 0; c < 6; ++c) bw[c] = split_root ? bw[c] + (dr[c] + di[c]) : (bw[c] + dr[c]) + di[c];
      }
      if (COM && !body_wrench) {
        // the root body's entry acts at the base-link origin: the allocator's wrench in root-link mode (then bw IS that entry),
        // else drag + disturbance (0 `+=` the one, `+=` the other: an absent term is +0).  A body wrench handed in
        // (AGX_LAUNCH_BODY_WRENCH) is about the centre of mass already (agx_net_body_wrench).
        const V3 f_root = root_link ? V3{bw[0], bw[1], bw[2]} : V3{dr[0] + di[0], dr[1] + di[1], dr[2] + di[2]};
        const V3 lever = com_root_torque(f_root, com);
        bw[3] = bw[3] + lever.x; bw[4] = bw[4] + lever.y; bw[5] = bw[5] + lever.z;
      }
      if (B.body_force && sub == k - 1) {  // what the IMU's force sensor sees (agx_imu_update)
        AGX_AT(B.body_force, 0) = bw[0]; AGX_AT(B.body_force, 1) = bw[1]; AGX_AT(B.body_force, 2) = bw[2];
      }
      const Q4 q_before = s.q;
      integrate(P, s, V3{bw[0], bw[1], bw[2]}, V3{bw[3], bw[4], bw[5]});
      if (COM) s.p = com_position_correction(s.p, q_before, s.q, com);
      if (B.boxes) {
        traj[(sub * 3 + 0) * bd + tid] = s.p.x;
        traj[(sub * 3 + 1) * bd + tid] = s.p.y;
        traj[(sub * 3 + 2) * bd + tid] = s.p.z;
        if (sub == 0) { tlo = s.p; thi = s.p; }
        tlo = V3{fminf(tlo.x, s.p.x), fminf(tlo.y, s.p.y), fminf(tlo.z, s.p.z)};
        thi = V3{fmaxf(thi.x, s.p.x), fmaxf(thi.y, s.p.y), fmaxf(thi.z, s.p.z)};
      }
