// The body of the one-lane env-step kernels, included INSIDE k_env_step<M, CTRL, SINGLE, WIDE>, k_env_step_rov<CTRL, SINGLE, WIDE> and
// k_env_step_com<M, CTRL, SINGLE, WIDE> (agx_dyn_env_step.h, nowhere else; no include guard on purpose).  The including kernel provides
// the kernel parameters P, B, n, actions_in, k_arg, T and the compile-time constants M, CTRL, SINGLE, WIDE, ROV and COM, and the
// vector `com`.  ROV: the robot kind BaseROV of the reference (AGX_LAUNCH_ROV) -- per-axis quadratic drag on the linear velocity,
// Euler angles stored without ssa().  COM: the composite's centre of mass lies at `com` in the base-link frame, not at its origin
// (agx_env_step_com) -- the root body's force gets its lever arm, the base-link position follows the turning body.  Written as text
// the kernels share rather than as a device function they call: the multirotor instances then compile from the statements they
// were compiled from before the other kinds existed, to the same instructions.  (The sub-step itself is agx_dyn_env_substep.h,
// text again: k_env_step_rollout, agx_dyn_rollout.h, runs the same statements inside its own loop over env steps.)
  const int k = SINGLE ? 1 : k_arg;
  extern __shared__ float traj[];  // [k][3][blockDim] sub-step positions (only with obstacles)
  const int tid = threadIdx.x, bd = blockDim.x;
  const int i = blockIdx.x * bd + tid;
  bool reset = false;
  // peer push: one wave holds the step until the slot of its rows is free (flags loaded here, looked at when the kernel is done)
  if (blockIdx.x == 0 && tid < 64) push_publish_previous(B);
  const uint32_t push_peek = (blockIdx.x == 0 && tid < 64) ? push_wait_peek(B) : 0u;
  if (i < n) {
    const int A = P.num_actions;
    // AGX_LAUNCH_LEAN (launch_flags bit 2): the tensors that only exist to be LOOKED AT through the tensor dict are not
    // maintained -- Euler angles, vehicle-frame quaternion / velocity, robot_actions / robot_prev_actions (40 + 48 of the
    // 330 bytes an env moves per step); the body-frame velocities stay (the observation kernel reads them)
    const bool lean = (B.launch_flags & 4) != 0;
    EnvState s = load_state(B.state, n, i);
    float u[M], kT[M], tinc[M], tdec[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
      u[j] = AGX_AT(B.motor_thrust, j);
      kT[j] = P.use_rps ? AGX_AT(B.motor_kT, j) : 1.0f;
      tinc[j] = B.motor_tau_inc ? AGX_AT(B.motor_tau_inc, j) : P.tau_inc_uniform;
      tdec[j] = B.motor_tau_dec ? AGX_AT(B.motor_tau_dec, j) : P.tau_dec_uniform;
    }
    // EXTERNAL controller (a user class evaluated by the host between launches): actions_in is ITS OUTPUT, the body
    // wrench [N][6]; robot_actions / robot_prev_actions (A columns) are maintained by the host and only read here
    constexpr bool EXT = CTRL == AGX_CTRL_WRENCH;
    float a_in[AGX_MAX_ACTIONS], a_old[AGX_MAX_ACTIONS];
    // (the row index in 32 bits: n x 8 actions < 2^32.  The 64-bit multiply the compiler made of (size_t)i * A carried a
    // don't-care register into its high half -- one a state load was still writing -- and waited for that load first)
    const unsigned arow = (unsigned)i * (unsigned)(EXT ? 6 : A);
#pragma unroll
    for (int c = 0; c < AGX_MAX_ACTIONS; ++c) {
      a_in[c] = (c < (EXT ? 6 : A)) ? actions_in[arow + (unsigned)c] : 0.0f;
      a_old[c] = (c < A && !lean) ? AGX_AT(B.actions, c) : 0.0f;
    }
    Derived d{};
    if (k == 0 && T.kind != AGX_TASK_NONE) d = load_derived(B.derived, n, i);
    // What the bookkeeping / task epilogue reads is requested HERE, with the state.  Behind the stores of this kernel the
    // compiler cannot move a load up (the buffers may alias for all it knows), and each load issued down there is a memory
    // round trip of its own on the wave's critical path that also sits out every store in front of it (gfx9 counts loads and
    // stores in one vmcnt): step counter -> target -> previous error were three such trips per wave.
    const bool more_launches = (B.launch_flags & 2) != 0;  // (launch_flags: see below)
    const bool task_epilogue = T.kind != AGX_TASK_NONE && !more_launches;
    const int steps_in = B.sim_steps[i];
    const int crashed_in = (B.launch_flags & 1) ? B.crashes[i] : 0;
    V3 tgt{0, 0, 0}, ppe{0, 0, 0};
    if (task_epilogue) {
      tgt = V3{AGX_AT(T.target, 0), AGX_AT(T.target, 1), AGX_AT(T.target, 2)};
      if (T.kind != AGX_TASK_POSITION) ppe = V3{AGX_AT(T.pos_err, 0), AGX_AT(T.pos_err, 1), AGX_AT(T.pos_err, 2)};
    }
    float a_prev_in[AGX_MAX_ACTIONS];  // robot_prev_actions as the last step left them (a k = 0 launch or an external controller reads them)
#pragma unroll
    for (int c = 0; c < AGX_MAX_ACTIONS; ++c) a_prev_in[c] = ((k == 0 || EXT) && c < A && !lean) ? AGX_AT(B.prev_actions, c) : 0.0f;
    // the gains LAST: with uniform gains (B.gains null) the registers they are moved into are the ones the other arm loads into,
    // and the compiler waits for every load in flight before the move -- behind the last load that wait costs nothing
    Gains g{};
    if (CTRL != AGX_CTRL_NONE && CTRL != AGX_CTRL_WRENCH) g = B.gains ? load_gains(B.gains, n, i) : uniform_gains(P);
    Wrench wc{V3{0, 0, 0}, V3{0, 0, 0}};
    const bool root_link = P.root_link_mode != 0;
    const int sub_base = (B.launch_flags >> 8) & 0xFF;  // physics sub-step this launch starts at (split env steps)
    bool has_drag = false;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      has_drag = has_drag || P.lin_drag_linear[c] != 0.0f || P.lin_drag_quadratic[c] != 0.0f || P.ang_drag_linear[c] != 0.0f ||
                 P.ang_drag_quadratic[c] != 0.0f;
    V3 tlo = s.p, thi = s.p;
    constexpr bool kLawReadsNoAngles = CTRL == AGX_CTRL_POSITION || CTRL == AGX_CTRL_FULLY_ACTUATED || CTRL == AGX_CTRL_NONE || CTRL == AGX_CTRL_WRENCH;
    for (int sub = 0; sub < k; ++sub) {
#include "agx_dyn_env_substep.h"
    }
    // EnvManager.reset_tensors + compute_observations (env_manager.py:342-344, 358-362)
    // launch_flags (external controllers run ONE launch per physics sub-step): bit 0 = an earlier launch of this env
    // step already ran: accumulate its crash flag; bit 1 = more launches follow: no step counter / truncation / task epilogue
    bool crashed = crashed_in != 0;
    if (B.boxes && k > 0) crashed = collide_trajectory(B.boxes, B.num_boxes, n, i, traj, k, bd, tid, tlo, thi, P.collision_radius) || crashed;
    store_state(B.state, n, i, s);
    if (k > 0) {
      if (lean) store_body_velocities(B.derived, n, i, d);
      else store_derived(B.derived, n, i, d);
#pragma unroll
      for (int j = 0; j < M; ++j) AGX_AT(B.motor_thrust, j) = u[j];
      if (B.wrench_cmd) {
        AGX_AT(B.wrench_cmd, 0) = wc.f.x; AGX_AT(B.wrench_cmd, 1) = wc.f.y; AGX_AT(B.wrench_cmd, 2) = wc.f.z;
        AGX_AT(B.wrench_cmd, 3) = wc.t.x; AGX_AT(B.wrench_cmd, 4) = wc.t.y; AGX_AT(B.wrench_cmd, 5) = wc.t.z;
      }
    }
    // RobotManagerIGE.pre_physics_step runs every sub-step: prev <- cur, cur <- action
    float a_cur[AGX_MAX_ACTIONS], a_prev[AGX_MAX_ACTIONS];
#pragma unroll
    for (int c = 0; c < AGX_MAX_ACTIONS; ++c) {
      a_cur[c] = (k > 0 && !EXT) ? a_in[c] : a_old[c];
      a_prev[c] = (k >= 2 && !EXT) ? a_in[c] : ((k == 1 && !EXT) ? a_old[c] : a_prev_in[c]);
      if (c < A && k > 0 && !EXT && !lean) {
        AGX_AT(B.prev_actions, c) = a_prev[c];
        AGX_AT(B.actions, c) = a_cur[c];
      }
    }
    const int steps = steps_in + (more_launches ? 0 : 1);
    if (!more_launches) B.sim_steps[i] = steps;
    bool trunc = false;
    if (task_epilogue) {
      float rew;
      if (T.kind == AGX_TASK_POSITION) {
        rew = reward_position(s, d.qveh, d.wbody, tgt, crashed);
      } else {
        AGX_AT(T.prev_pos_err, 0) = ppe.x; AGX_AT(T.prev_pos_err, 1) = ppe.y; AGX_AT(T.prev_pos_err, 2) = ppe.z;
        V3 pe = quat_rotate_inverse(d.qveh, tgt - s.p);
        AGX_AT(T.pos_err, 0) = pe.x; AGX_AT(T.pos_err, 1) = pe.y; AGX_AT(T.pos_err, 2) = pe.z;
        rew = reward_navigation(T.rp, T.curriculum_progress, pe, ppe, a_cur[0], a_cur[2], a_cur[3], a_prev[0], a_prev[2],
                                a_prev[3], crashed);
      }
      T.reward[i] = rew;
      trunc = steps > T.episode_len;
      reset = (crashed && T.reset_on_collision) || trunc;
      B.reset_mask[i] = reset ? 1 : 0;
      if (T.successes) nav_bookkeeping_epilogue(T, i, true, tgt, s.p, crashed, trunc);  // (wave-uniform pointer test)
    }
    B.crashes[i] = crashed ? 1 : 0;
    if (!more_launches) B.truncations[i] = trunc ? 1 : 0;
  }
  if (T.kind != AGX_TASK_NONE && __ballot(reset) != 0ull && (tid & 63) == 0) atomicOr(B.reset_flag + B.flag_parity, 1);
  if (blockIdx.x == 0 && tid < 64) push_wait_finish(B, push_peek);
