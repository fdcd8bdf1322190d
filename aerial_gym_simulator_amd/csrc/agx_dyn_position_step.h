#pragma once
// The position step: the phase stamps of the probe build, the proof record on the device, the step wave and its helper wave,
// k_env_step_quad_position and the single-launch k_position_step_fused; then the host side of the plan (agx_position_task_step).
// Part of the one translation unit agx_dynamics.hip, which alone includes it (after the AGX_DYN_* switches).

namespace agx {
// -DAGX_STEP_STAMPS (profiles/step_phase_probe.py; never in the product build): lane 0 of every wave of a position-step launch
// stamps the shader clock at six points -- 0 wave start, 1 arguments there / first input load issued, 2 inputs arrived (the
// stamped build waits for them there), 3 barrier reached (NONE / TWO: the step is computed), 4 barrier passed, 5 last store
// issued -- and the 100 MHz wall clock at start and end ([6], [7]: cycles -> ns, and who finishes last), with plain vector stores.
#ifdef AGX_STEP_STAMPS
constexpr int kStampBlocks = 1024, kStampWords = 8;
__device__ unsigned long long g_step_stamps[kStampBlocks * 2 * kStampWords];
AGX_DEV void step_stamp(int k) {
  const unsigned long long t = k < 6 ? (unsigned long long)clock64() : (unsigned long long)wall_clock64();
  if ((threadIdx.x & 63u) == 0u && blockIdx.x < (unsigned)kStampBlocks)
    g_step_stamps[((size_t)blockIdx.x * 2 + (threadIdx.x >> 6)) * kStampWords + k] = t;
}
#define AGX_STAMP(k) step_stamp(k)
#define AGX_STAMP_ARRIVED(k) do { __builtin_amdgcn_s_waitcnt(0); step_stamp(k); } while (0)
#else
#define AGX_STAMP(k) do { } while (0)
#define AGX_STAMP_ARRIVED(k) do { } while (0)
#endif

// ---- single-launch position steps: the proof record (include/aerial_gym_hip.h, AgxPositionStepPlan) ---------------------------
// Every wave of a position-step launch of a plan leaves a slot about the END of its step, double-buffered by the step's parity
// (the folding workgroup of launch u reads bank (u - 1) & 1 while the waves of launch u write bank u & 1):
//   [0] tag = step_counter + 1 (31 bits)   [1] bit 0: some env of the wave reset, bit 1: the launch was AGX_STEP_ANY
//   [2] horizon: bit k = a witness env truncates in step t + k   [3] max sim_steps   [4] max dist bits   [5] max |v| bits
// dist and |v| are >= 0, so their bit patterns order like the values; NaN maps to 0x7FC00000, above every finite value and inf.
AGX_DEV unsigned proof_key(float x) { return x >= 0.0f ? __float_as_uint(x) : 0x7FC00000u; }

// env i is a witness for step t + k (k = episode_len - sim_steps + 1: it truncates then) if it did not reset in step t and cannot
// reset before: k = 1, or crashes do not reset, or it cannot get 8 m from its target in k - 1 steps, where m steps take it at
// most m dt min(v_max, |v| + m dv) (agx_step_proof_travel, per_env, margins included).  NaN distances or speeds: never witnesses.
// (host and device: agx_step_proof_witness_bit exports it to the CPU tests)
__host__ __device__ inline unsigned proof_witness_bit(int episode_len, int reset_on_collision, int steps, float dist, float speed, float dt,
                                                      float vmax, float dv) {
  const int k = episode_len - steps + 1;
  if (k < 1 || k > AGX_PROOF_HORIZON || !(dist == dist) || !(speed == speed)) return 0u;
  bool w = k == 1 || !reset_on_collision;
  if (!w) {
    const float m = (float)(k - 1);
    const float travel = m * dt * fminf(vmax, speed + m * dv);
    w = dist + (travel * 1.01f + 1.0e-3f) < 8.0f;
  }
  return w ? (1u << k) : 0u;
}

// OR (MAX = false) or unsigned max over the 64 lanes of a wave, as a wave-uniform value.  All 64 lanes must be active.
template <bool MAX>
AGX_DEV unsigned wave_reduce_dpp(unsigned x) {
#define AGX_RED(ctrl)                                                                        \
  {                                                                                           \
    const unsigned y_ = (unsigned)__builtin_amdgcn_mov_dpp((int)x, (ctrl), 0xF, 0xF, true);   \
    x = MAX ? max(x, y_) : (x | y_);                                                          \
  }
  AGX_RED(0xB1)   // quad_perm:[1,0,3,2]
  AGX_RED(0x4E)   // quad_perm:[2,3,0,1]
  AGX_RED(0x124)  // row_ror:4
  AGX_RED(0x128)  // row_ror:8
#undef AGX_RED
  const unsigned r0 = (unsigned)__builtin_amdgcn_readlane((int)x, 0), r1 = (unsigned)__builtin_amdgcn_readlane((int)x, 16);
  const unsigned r2 = (unsigned)__builtin_amdgcn_readlane((int)x, 32), r3 = (unsigned)__builtin_amdgcn_readlane((int)x, 48);
  return MAX ? max(max(r0, r1), max(r2, r3)) : ((r0 | r1) | (r2 | r3));
}

AGX_DEV void proof_store_slot(const AgxTaskArgs &T, const AgxEnvBuffers &B, int wb, int nb, bool reset, unsigned horizon, int steps,
                              float dist, float speed) {
  // only lane 0 stores: OR and max are idempotent, so four DPP stages leave every lane with its row's value and the four rows
  // meet in scalar registers -- no trip through the LDS crossbar (a __shfl_xor butterfly is six dependent ds_bpermute stages)
  const unsigned ar = wave_reduce_dpp<false>(reset ? 1u : 0u), hz = wave_reduce_dpp<false>(horizon);
  const unsigned ms = wave_reduce_dpp<true>((unsigned)max(steps, 0)), db = wave_reduce_dpp<true>(proof_key(dist));
  const unsigned vb = wave_reduce_dpp<true>(proof_key(speed));
  if ((threadIdx.x & 63u) == 0u) {
    uint4 *slot = reinterpret_cast<uint4 *>(T.proof_slots + ((size_t)(B.step_counter & 1) * nb + wb) * AGX_PROOF_SLOT_WORDS);
    slot[0] = make_uint4(((unsigned)B.step_counter + 1u) & 0x7FFFFFFFu, ar | (T.proof_mode == AGX_STEP_ANY ? 2u : 0u), hz, ms);
    slot[1] = make_uint4(db, vb, 0u, 0u);
  }
}

// workgroup 0 of a launch with slots: fold the `nb` slots of the launch before (complete: kernel boundary) and publish them to
// the host record -- begin tag, payload, end tag, each acknowledged before the next is stored (system-scope write-through stores
// to mapped host memory: acknowledged = visible to the host).  An AGX_STEP_ANY launch in which no env reset is a broken proof.
AGX_DEV void proof_fold_publish(const AgxTaskArgs &T, const AgxEnvBuffers &B, int nb) {
  const int lane = (int)(threadIdx.x & 63u);
  const uint32_t *bank = T.proof_slots + (size_t)((B.step_counter & 1) ^ 1) * nb * AGX_PROOF_SLOT_WORDS;
  unsigned t_and = 0x7FFFFFFFu, t_or = 0u, fl = 0u, hz = 0u, ms = 0u, db = 0u, vb = 0u;
  for (int b = lane; b < nb; b += 64) {
    const uint4 s0 = reinterpret_cast<const uint4 *>(bank + (size_t)b * AGX_PROOF_SLOT_WORDS)[0];
    const uint4 s1 = reinterpret_cast<const uint4 *>(bank + (size_t)b * AGX_PROOF_SLOT_WORDS)[1];
    t_and &= s0.x; t_or |= s0.x; fl |= s0.y; hz |= s0.z;
    ms = max(ms, s0.w); db = max(db, s1.x); vb = max(vb, s1.y);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    t_and &= (unsigned)__shfl_xor((int)t_and, off);
    t_or |= (unsigned)__shfl_xor((int)t_or, off);
    fl |= (unsigned)__shfl_xor((int)fl, off);
    hz |= (unsigned)__shfl_xor((int)hz, off);
    ms = max(ms, (unsigned)__shfl_xor((int)ms, off));
    db = max(db, (unsigned)__shfl_xor((int)db, off));
    vb = max(vb, (unsigned)__shfl_xor((int)vb, off));
  }
  if (lane != 0) return;
  const unsigned tag = t_and == t_or ? t_or : 0u;  // every slot written by the same launch, else: not a record
  if (tag != 0u && (fl & 2u) && !(fl & 1u)) atomicAdd(T.proof_violation, 1u);
  uint32_t *h = T.proof_record;
  __hip_atomic_store(h + 7, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (compiler: keep the order)
  __builtin_amdgcn_s_waitcnt(0);                          // (hardware: acknowledged)
  __hip_atomic_store(h + 1, hz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(h + 2, ms, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(h + 3, db, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(h + 4, vb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(h + 5, fl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_s_waitcnt(0);
  __hip_atomic_store(h + 0, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// One env step of the plain quadrotor position task, four lanes per env.  MODE:
//   AGX_STEP_TWO   the first of the two launches (k_env_step_quad_position): step, derived tensors of the pre-step state,
//                  task epilogue; k_reset_masked_quad_obs follows
//   AGX_STEP_ANY   the whole step when some env certainly resets: as TWO without the (dead) pre-step derived stores, then
//                  what k_reset_masked_quad_obs does with its flag set -- the reset of the env's own flagged envs, the refresh
//                  of every env from its post-step / post-reset state, the observation
//   AGX_STEP_NONE  the whole step when no env can reset: as TWO, then the observation from the pre-step derived tensors (what
//                  k_reset_masked_quad_obs reads back with its flag clear)
// Same IEEE operations in the same order in every mode (bit-identical); the fused modes write no address from two lanes (the
// sub-step's state, thrust and sim_steps stores are skipped for an env that reset_env rewrites) and carry no step exchange.
//
// ANY runs on two waves per workgroup.  A launch lasts as long as its slowest wave, a lone wave per SIMD issues one instruction
// after the other, and the reset, the refresh and the observation do not depend on most of what the step computes: they are
// position_step_helper's, on a SIMD of the same CU that would otherwise idle.  The step wave (this function, wave 0) hands the
// post-step state and the reset bits over through LDS at ONE workgroup barrier that every wave of an env workgroup reaches
// unconditionally, and goes on with the reward, the proof slot and its own stores.  NONE and TWO have no such tail and stay
// one-wave workgroups without an LDS segment.
struct StepHandoff {
  float p[64], q[64], v[64], w[64];  // per lane of the step wave: its component of the post-step state
  int reset[64];                     // the env resets (truncation or crash)
};
template <int MODE>
AGX_DEV void position_step_quad(const AgxRobotParams &P0, const AgxEnvBuffers &B0, int n, const float *actions_in,
                                const AgxTaskArgs &T0, float *obs, StepHandoff *H) {
  constexpr bool FUSED = MODE != AGX_STEP_TWO;
  const int tid = threadIdx.x;
  AGX_STAMP(0); AGX_STAMP(6);
  // ---- kernel arguments: every field this wave uses, one batch (arg_pin).  P / B / T are the pinned copies; P0 / B0 / T0 serve
  // only what indexes an argument array by lane (vector loads: load_quad_consts, the peer-push flag pointers) and the folding
  // workgroup
  AgxRobotParams P = P0;
  AgxEnvBuffers B = B0;
  AgxTaskArgs T = T0;
#define AGX_STEP_WAVE_ARGS(X)                                                                                                        \
  X(B, state) X(B, actions) X(B, prev_actions) X(B, motor_thrust) X(B, motor_kT) X(B, motor_tau_inc) X(B, motor_tau_dec)  \
  X(B, gains) X(B, wrench_cmd) X(B, crashes) X(B, truncations) X(B, sim_steps) X(B, reset_mask) X(B, reset_flag) X(B, flag_parity)    \
  X(B, step_counter) X(B, body_force)                                                                                                  \
  X(P, dt) X(P, dt_over_6) X(P, mass) X(P, min_thrust) X(P, max_thrust) X(P, max_rate) X(P, linear_damping) X(P, angular_damping)     \
  X(P, max_linear_velocity) X(P, max_angular_velocity) X(P, tau_inc_uniform) X(P, tau_dec_uniform)                                    \
  X(T, episode_len) X(T, target) X(T, reward) X(T, proof_slots) X(T, proof_violation) X(T, proof_dv)
  AGX_STEP_WAVE_ARGS(AGX_ARG_READ)
  AGX_ARG_READ(B, derived) AGX_ARG_READ(B, push_world)
  AGX_ARG_READ(P, root_link_mode) AGX_ARG_READ(P, use_rps) AGX_ARG_READ(P, use_discrete_approximation) AGX_ARG_READ(P, integration_rk4)
  AGX_ARG_READ(T, reset_on_collision) AGX_ARG_READ(T, kind) AGX_ARG_READ(T, proof_mode)
  const int grid_blocks = (int)gridDim.x;  // (an implicit argument: fetched with the rest, not in front of the proof slot's stores)
  // nothing crosses this line when the instructions are scheduled: every read above is issued before the first value is looked
  // at below (otherwise the scheduler defers some of the reads behind the first pin's wait: a second and a third round trip)
  __builtin_amdgcn_sched_barrier(0);
  int env_blocks = grid_blocks - 1;
  // the switches and the small enumerations share ONE register (the one-wave kernels have none to spare: 102, no spills)
  int sw = (P_root_link_mode != 0 ? 1 : 0) | (P_use_rps != 0 ? 2 : 0) | (P_use_discrete_approximation != 0 ? 4 : 0) |
           (P_integration_rk4 != 0 ? 8 : 0) | (T_reset_on_collision != 0 ? 16 : 0) | ((T_kind & 0xFF) << 8) | ((T_proof_mode & 0xFF) << 16);
  arg_pin(n); arg_pin(actions_in);
  if (MODE == AGX_STEP_NONE) arg_pin(obs);
  AGX_STEP_WAVE_ARGS(AGX_ARG_PIN)
  if (MODE != AGX_STEP_ANY) { AGX_ARG_PIN(B, derived) }
  if (!FUSED) { AGX_ARG_PIN(B, push_world) }
  arg_pin(env_blocks);
#undef AGX_STEP_WAVE_ARGS
  arg_pin(sw);
  P.root_link_mode = sw & 1; P.use_rps = sw & 2; P.use_discrete_approximation = sw & 4; P.integration_rk4 = sw & 8;
  T.reset_on_collision = sw & 16; T.kind = (sw >> 8) & 0xFF; T.proof_mode = (sw >> 16) & 0xFF;
  const bool proof = T.proof_slots != nullptr;
  if (proof && blockIdx.x == 0) {  // the extra workgroup of a launch with slots: no envs, only the host record
    proof_fold_publish(T0, B0, (int)gridDim.x - 1);
    AGX_STAMP(5); AGX_STAMP(7);
    return;
  }
  const int wb = (int)blockIdx.x - (proof ? 1 : 0);  // env block
  const int l = tid & 3, l3 = l < 3 ? l : 2;  // component of a 4-vector / of a 3-vector (lane 3 repeats z: don't care)
  const int i = wb * 16 + (tid >> 2);  // env
  const unsigned ol = ((unsigned)l * (unsigned)n + (unsigned)i) * 4u, ol3 = ((unsigned)l3 * (unsigned)n + (unsigned)i) * 4u;  // AGX_QAT
  const bool valid = i < n;
  bool reset = false;
  if (FUSED && wb == 0 && tid == 0) B.reset_flag[B.flag_parity ^ 1] = 0;  // (what the second launch does first)
  // peer push (one wave of the launch, sharded runs only: the unlikely side, laid out behind the kernel's own path), decided on
  // the pinned word: no argument fetch here without it
  const bool push = !FUSED && wb == 0 && B.push_world > 0;
  uint32_t push_peek = 0u;
  if (__builtin_expect(push, false)) {
    push_publish_previous(B0);        // the previous step's rows have landed everywhere
    push_peek = push_wait_peek(B0);  // ... and this step's slot: looked at when the kernel is done
  }
  float p = 0.0f, q = 0.0f, v = 0.0f, w = 0.0f, tgt = 0.0f, vbody = 0.0f, wbody = 0.0f;
  int steps = 0;
  float proof_dist = 0.0f, proof_speed = 0.0f;
  unsigned horizon = 0u;
  // what the second half of the step (behind ANY's hand-off) takes over from the first
  float u[1] = {0.0f}, a_in = 0.0f, a_old = 0.0f, fz = 0.0f, torque = 0.0f, dist = 0.0f;
  QuadDerived d{};
  bool crashed = false, trunc = false;
  AGX_STAMP(1);
  if (valid) {
    // ---- loads: one instruction per vector, all of them issued before any is looked at (one memory round trip).  A buffer
    // that may be absent is a branch on its wave-uniform pointer around a load that replaces the uniform value (the gains: the
    // lane's component, an indexed kernel-argument load issued in any case -- twelve scalar registers would not fit): a
    // `pointer ? global[...] : P.uniform[...]` select compiled to a FLAT load through a selected address, and flat loads count
    // on lgkmcnt too -- every later wait for a scalar load also sat out those vector loads' trip to memory
    p = AGX_QAT(B.state, 0, ol3); q = AGX_QAT(B.state, 3, ol); v = AGX_QAT(B.state, 7, ol3); w = AGX_QAT(B.state, 10, ol3);
    u[0] = AGX_QAT(B.motor_thrust, 0, ol);  // motor l
    float kT[1] = {1.0f}, tinc[1] = {P.tau_inc_uniform}, tdec[1] = {P.tau_dec_uniform};
    if (P.use_rps) kT[0] = AGX_QAT(B.motor_kT, 0, ol);
    if (B.motor_tau_inc) tinc[0] = AGX_QAT(B.motor_tau_inc, 0, ol);
    if (B.motor_tau_dec) tdec[0] = AGX_QAT(B.motor_tau_dec, 0, ol);
    a_in = actions_in[(size_t)i * 4 + l];
    a_old = AGX_QAT(B.actions, 0, ol);
    float kp = P0.gains_uniform[0 + l3], kv = P0.gains_uniform[3 + l3], kr = P0.gains_uniform[6 + l3], kw = P0.gains_uniform[9 + l3];
    if (B.gains) {  // (gain_load: not a load the compiler may fold with the one above into a flat load of a selected address)
      kp = gain_load(&AGX_QAT(B.gains, 0, ol3)); kv = gain_load(&AGX_QAT(B.gains, 3, ol3));
      kr = gain_load(&AGX_QAT(B.gains, 6, ol3)); kw = gain_load(&AGX_QAT(B.gains, 9, ol3));
    }
    // what the task epilogue reads is requested HERE, with the state: behind the stores below the compiler cannot move a load up
    // (the buffers may alias for all it knows), and a load issued there is a second memory round trip on the kernel's critical
    // path -- one that also waits for every store in front of it (gfx9 counts loads and stores in the same vmcnt)
    const int steps_in = B.sim_steps[i];
    tgt = T.kind == AGX_TASK_POSITION ? AGX_QAT(T.target, 0, ol3) : 0.0f;
    const QuadConsts<4> C = load_quad_consts<4>(P0, P, l, l3);
    AGX_STAMP_ARRIVED(2);

    // ---- update_states + controller (position_control.py:20-51)
    const float a = clamp_minmax(a_in, -10.0f, 10.0f);  // clip_actions
    float sy_sp, cy_sp;  // of the yaw set-point (lanes 0, 1), out of the evaluation that serves the vehicle-frame quaternion
    d = update_states_quad(q, v, w, q4::bc<3>(a), sy_sp, cy_sp);
    // compute_acceleration (velocity set-point 0): kp (sp - p) + kv (0 - v)
    const float pe = a - p;
    const float ve = 0.0f - v;
    const float acc = kp * pe + kv * ve;
    const float f = (acc - C.grav) * C.mass;
    fz = quad_thrust_along_body_z(q, f, l);
    const float qd = quad_desired_orientation_pos_vel_sc(f, sy_sp, cy_sp, l);
    torque = quad_body_torque<true>(C, q, qd, d.wbody, 0.0f, kr, kw, l);

    // ---- allocation + motor model + body wrench, rigid-body update
    float fb, tb;
    quad_allocate<4>(P, C, l == 2 ? fz : 0.0f, torque, u, kT, tinc, tdec, fb, tb);
    if (B.body_force && l < 3) AGX_QAT(B.body_force, 0, ol) = fb;
    quad_integrate(P, C, p, q, v, w, fb, tb, l);

    // ---- EnvManager bookkeeping + the reset set of the position task (position_setpoint_task.py:245-282)
    steps = steps_in + 1;
    if (T.kind == AGX_TASK_POSITION) {
      const float pe_t = q4::quat_apply(q4::conj(d.qveh), tgt - p);  // quat_apply_inverse
      dist = q4::norm3(pe_t);
      if (dist > 8.0f) crashed = true;
      trunc = steps > T.episode_len;
      reset = (crashed && T.reset_on_collision) || trunc;
    }
  }
  AGX_STAMP(3);
  if (MODE == AGX_STEP_ANY) {  // the hand-off to the helper wave: every lane of every env workgroup, whatever `valid` says
    H->p[tid] = p; H->q[tid] = q; H->v[tid] = v; H->w[tid] = w;
    H->reset[tid] = reset ? 1 : 0;
    __syncthreads();
  }
  AGX_STAMP(4);
  if (valid) {
    // ---- the position task's reward
    float rew = 0.0f;
    if (T.kind == AGX_TASK_POSITION) {
      // 3 exp(-8 d^2) + 2 exp(-4 d^2): both exponentials in one evaluation (lanes 0 / 1)
      const float ex = exp_cw((l == 0 ? -8.0f : -4.0f) * dist * dist);
      const float pos_reward = 3.0f * q4::bc<0>(ex) + 2.0f * q4::bc<1>(ex);
      const float dist_reward = (20.0f - dist) / 40.0f;
      const float axis_z = l == 2 ? 1.0f : 0.0f;
      const float up = q4::bc<2>(q4::quat_rotate(q, axis_z));  // quat_axis(q, 2).z
      const float tilt = fabsf(1.0f - up);
      const float spin = q4::norm3(d.wbody);
      // 0.2 / (0.1 + tilt^2) = reciprocal * 0.2 (torch's scalar / tensor) and (1 / (1 + spin^2)) * 3: one division (lanes 0 / 1)
      const float quo = (1.0f / (l == 0 ? 0.1f + tilt * tilt : 1.0f + spin * spin)) * (l == 0 ? 0.2f : 3.0f);
      const float up_reward = q4::bc<0>(quo);
      const float ang_reward = q4::bc<1>(quo);
      float total = pos_reward + dist_reward + pos_reward * (up_reward + ang_reward);
      total = 1.0f * total;
      if (crashed) total = -20.0f;
      rew = total;
      proof_dist = dist;
    }
    if (proof) {
      proof_speed = q4::norm3(v);  // the post-step linear speed
      if (l == 0 && !reset && T.kind == AGX_TASK_POSITION) horizon = proof_witness_bit(T.episode_len, T.reset_on_collision, steps, proof_dist, proof_speed, P.dt, P.max_linear_velocity,
                                    T.proof_dv);
    }

    // ---- stores: state, derived, motors, controller output, actions (reset_env rewrites state, thrust and sim_steps of an env
    // that resets in a fused launch: it alone stores them then)
    const bool own = MODE != AGX_STEP_ANY || !reset;
    if (own) {
      if (l < 3) AGX_QAT(B.state, 0, ol) = p;
      AGX_QAT(B.state, 3, ol) = q;
      if (l < 3) {
        AGX_QAT(B.state, 7, ol) = v;
        AGX_QAT(B.state, 10, ol) = w;
      }
      AGX_QAT(B.motor_thrust, 0, ol) = u[0];
    }
    if (MODE != AGX_STEP_ANY) {  // (ANY: the refresh below overwrites them)
      if (l < 3) {
        AGX_QAT(B.derived, 0, ol) = d.euler;
        AGX_QAT(B.derived, 7, ol) = d.vveh;
        AGX_QAT(B.derived, 10, ol) = d.vbody;
        AGX_QAT(B.derived, 13, ol) = d.wbody;
      }
      AGX_QAT(B.derived, 3, ol) = d.qveh;
    }
    vbody = d.vbody;
    wbody = d.wbody;
    if (B.wrench_cmd) {
      if (l < 3) {
        AGX_QAT(B.wrench_cmd, 0, ol) = l == 2 ? fz : 0.0f;
        AGX_QAT(B.wrench_cmd, 3, ol) = torque;
      }
    }
    AGX_QAT(B.prev_actions, 0, ol) = a_old;  // RobotManagerIGE.pre_physics_step: prev <- cur, cur <- action
    AGX_QAT(B.actions, 0, ol) = a_in;
    if (l == 0) {
      if (own) B.sim_steps[i] = steps;
      if (T.kind == AGX_TASK_POSITION) {
        T.reward[i] = rew;
        B.reset_mask[i] = reset ? 1 : 0;
      }
      B.crashes[i] = crashed ? 1 : 0;
      B.truncations[i] = trunc ? 1 : 0;
    }
  }
  const bool some = __ballot(reset) != 0ull;
  if (T.kind != AGX_TASK_NONE && some && (tid & 63) == 0) {
    atomicOr(B.reset_flag + B.flag_parity, 1);
    if (MODE == AGX_STEP_NONE) atomicAdd(T.proof_violation, 1u);  // cannot happen (the host proved it): tests watch this word
  }
  if (proof) proof_store_slot(T, B, wb, env_blocks, reset, horizon, steps, proof_dist, proof_speed);
  if (!FUSED) {
    if (__builtin_expect(push, false)) push_wait_finish(B0, push_peek);
    AGX_STAMP(5); AGX_STAMP(7);
    return;
  }
  if (MODE == AGX_STEP_ANY) {  // the reset, the refresh and the observation are the helper wave's
    AGX_STAMP(5); AGX_STAMP(7);
    return;
  }
  if (valid) {  // position_setpoint_task.py:194-203: target - p | q | v_body | w_body
    float *o = obs + (size_t)i * 13;
    const float e = tgt - p;
    if (l < 3) { o[l] = e; o[7 + l] = vbody; o[10 + l] = wbody; }
    o[3 + l] = q;
  }
  AGX_STAMP(5); AGX_STAMP(7);
}

// The helper wave (wave 1) of an env workgroup of k_position_step_fused<AGX_STEP_ANY>: what k_reset_masked_quad_obs does with
// its flag set (reset_masked_quad_obs_body<false>), same lane layout as the step wave, in two phases around the one barrier:
//   1  while the step wave computes: truncation is `sim_steps + 1 > episode_len`, known from a load, so the draws and the new
//      state of a truncating env are evaluated here -- into registers: reset_env's stores hit addresses the step wave loads at
//      its top, and nothing orders the two waves before the barrier;
//   2  behind the barrier: the envs that crashed (known only after the step) get their draws and values now, reset_env's
//      stores go out, then BaseMultirotor.reset_idx's un-indexed update_states() of every env and the observation.
// Every address stored here belongs to a resetting env (the step wave skips those: `own`) or is a derived tensor / the
// observation (the step wave writes neither in ANY).  Draws are keyed by (seed, global env, episode, stream, block): evaluating
// them for the truncating and the crashing envs in two calls gives the same values as one call for both.
AGX_DEV void position_step_helper(const AgxRobotParams &P0, const AgxEnvBuffers &B0, int n, const AgxTaskArgs &T0, const AgxResetArgs &R0,
                                  float *obs, const StepHandoff *H) {
  AGX_STAMP(0); AGX_STAMP(6);
  // ---- kernel arguments: every field this wave uses, one batch (arg_pin) -- the reset ranges included: behind the barrier this
  // wave is the launch's critical path, and a crash's values and every store of a resetting env otherwise start with a fetch
  AgxRobotParams P = P0;
  AgxEnvBuffers B = B0;
  AgxTaskArgs T = T0;
  AgxResetArgs R = R0;
#define AGX_HELPER_WAVE_ARGS(X, XN)                                                                                                  \
  X(B, sim_steps) X(B, episode_count) X(B, env_index_base) X(B, bounds_min) X(B, bounds_max) X(B, state) X(B, derived) X(B, gains)    \
  X(B, motor_tau_inc) X(B, motor_tau_dec) X(B, motor_thrust) X(B, motor_kT)                                                           \
  X(P, use_rps) X(P, min_thrust) X(P, max_thrust) X(T, kind) X(T, episode_len) X(T, target) X(T, proof_slots)                         \
  XN(R, lower_bound_min, 3) XN(R, lower_bound_max, 3) XN(R, upper_bound_min, 3) XN(R, upper_bound_max, 3) XN(R, min_state, 13)        \
  XN(R, max_state, 13) XN(R, gains_min, 12) XN(R, gains_max, 12) X(R, tau_inc_min) X(R, tau_inc_max) X(R, tau_dec_min)                \
  X(R, tau_dec_max) X(R, kT_min) X(R, kT_max) X(R, randomize_gains) X(R, seed)
  AGX_HELPER_WAVE_ARGS(AGX_ARG_READ, AGX_ARG_READ_N)
  arg_pin(n); arg_pin(obs);
  AGX_HELPER_WAVE_ARGS(AGX_ARG_PIN, AGX_ARG_PIN_N)
#undef AGX_HELPER_WAVE_ARGS
  const bool proof = T.proof_slots != nullptr;
  if (proof && blockIdx.x == 0) return;  // the folding workgroup: wave 0's, and no barrier in it
  const int lane = (int)(threadIdx.x & 63u);
  const int wb = (int)blockIdx.x - (proof ? 1 : 0);  // env block
  const int l = lane & 3, l3 = l < 3 ? l : 2;
  const int i = wb * 16 + (lane >> 2);  // env
  const unsigned ol = ((unsigned)l * (unsigned)n + (unsigned)i) * 4u, ol3 = ((unsigned)l3 * (unsigned)n + (unsigned)i) * 4u;  // AGX_QAT
  const bool valid = i < n;
  int steps_in = 0, ep = 0;
  float tgt = 0.0f;
  AGX_STAMP(1);
  if (valid) {
    steps_in = B.sim_steps[i];
    if (B.episode_count) ep = B.episode_count[i];  // (the reset's draws are keyed by it)
    tgt = T.kind == AGX_TASK_POSITION ? AGX_QAT(T.target, 0, ol3) : 0.0f;
  }
  AGX_STAMP_ARRIVED(2);
  // ---- phase 1: the step wave's own truncation predicate
  const bool early = valid && T.kind == AGX_TASK_POSITION && steps_in + 1 > T.episode_len;
  ResetValues<4> V{};
  if (vote(early) != 0ull) {
    ResetDraws<4> D{};
    wave_reset_draws<4>(R, B.env_index_base + i, ep, early && l == 0, D);  // draws are keyed by the GLOBAL env index
    V = reset_env_values<4>(P, R, D);
  }
  AGX_STAMP(3);
  __syncthreads();
  AGX_STAMP(4);
  // ---- phase 2
  float p = H->p[lane], q = H->q[lane], v = H->v[lane], w = H->w[lane];
  const bool mine = H->reset[lane] != 0;
  const bool late = mine && !early;  // a crash
  if (vote(late) != 0ull) {
    ResetDraws<4> D{};
    wave_reset_draws<4>(R, B.env_index_base + i, ep, late && l == 0, D);
    const ResetValues<4> V2 = reset_env_values<4>(P, R, D);
    if (late) V = V2;
  }
  if (vote(mine) != 0ull) {  // some env of this wave resets
    if (mine && l == 0) reset_env_store<4>(P, B, n, R, i, ep, V);
    // the quad takes the new state over from its first lane
    const EnvState &s = V.s;
    const float npv = q4::by_lane(l3, q4::bc<0>(s.p.x), q4::bc<0>(s.p.y), q4::bc<0>(s.p.z));
    const float nq = q4::by_lane(l, q4::bc<0>(s.q.x), q4::bc<0>(s.q.y), q4::bc<0>(s.q.z), q4::bc<0>(s.q.w));
    const float nv = q4::by_lane(l3, q4::bc<0>(s.v.x), q4::bc<0>(s.v.y), q4::bc<0>(s.v.z));
    const float nw = q4::by_lane(l3, q4::bc<0>(s.w.x), q4::bc<0>(s.w.y), q4::bc<0>(s.w.z));
    p = mine ? npv : p; q = mine ? nq : q; v = mine ? nv : v; w = mine ? nw : w;
  }
  // BaseMultirotor.reset_idx ends with an un-indexed update_states(): every env is refreshed
  const QuadDerived d2 = update_states_quad(q, v, w);
  if (valid) {
    if (l < 3) {
      AGX_QAT(B.derived, 0, ol) = d2.euler;
      AGX_QAT(B.derived, 7, ol) = d2.vveh;
      AGX_QAT(B.derived, 10, ol) = d2.vbody;
      AGX_QAT(B.derived, 13, ol) = d2.wbody;
    }
    AGX_QAT(B.derived, 3, ol) = d2.qveh;
    // position_setpoint_task.py:194-203: target - p | q | v_body | w_body
    float *o = obs + (size_t)i * 13;
    const float e = tgt - p;
    if (l < 3) { o[l] = e; o[7 + l] = d2.vbody; o[10 + l] = d2.wbody; }
    o[3 + l] = q;
  }
  AGX_STAMP(5); AGX_STAMP(7);
}

__global__ void __launch_bounds__(64, 1)
    k_env_step_quad_position(AgxRobotParams P, AgxEnvBuffers B, int n, const float *__restrict__ actions_in, AgxTaskArgs T) {
  position_step_quad<AGX_STEP_TWO>(P, B, n, actions_in, T, nullptr, nullptr);
}

// The whole position step as ONE launch (agx_position_task_step, when the host record proves the outcome of the batch-wide reset
// OR): AGX_STEP_ANY or AGX_STEP_NONE, always with the proof slots and the folding workgroup 0.  ANY: 128 threads, the step wave
// and its helper wave (position_step_quad); both waves of the folding workgroup return before any barrier.
template <int MODE>
__global__ void __launch_bounds__(MODE == AGX_STEP_ANY ? 128 : 64, 1)
    k_position_step_fused(AgxRobotParams P, AgxEnvBuffers B, int n, const float *__restrict__ actions_in, AgxTaskArgs T, AgxResetArgs R,
                          float *__restrict__ obs) {
  if constexpr (MODE == AGX_STEP_ANY) {
    __shared__ StepHandoff H;
    // (readfirstlane: a scalar branch -- each wave runs one side only and meets exactly one s_barrier)
    if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0) position_step_quad<MODE>(P, B, n, actions_in, T, obs, &H);
    else position_step_helper(P, B, n, T, R, obs, &H);
  } else {
    position_step_quad<MODE>(P, B, n, actions_in, T, obs, nullptr);
  }
}

#ifdef AGX_STEP_STAMPS
}  // namespace agx
// [blocks][2 waves][8] of the LAST position-step launch (blocks <= 1024); a wave that did not run leaves its words as they were
extern "C" int agx_debug_step_stamps(unsigned long long *out, int blocks) {
  if (blocks < 0 || blocks > agx::kStampBlocks) return -1;
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(agx::g_step_stamps), sizeof(unsigned long long) * 2 * agx::kStampWords * (size_t)blocks);
}
namespace agx {
#endif
}  // namespace agx

// ---- single-launch position steps: the host side (include/aerial_gym_hip.h, AgxPositionStepPlan) -------------------------------
extern "C" float agx_step_proof_dv(const AgxRobotParams *P) {
  if (!P || !(P->mass > 0.0f)) return INFINITY;
  const int M = P->num_motors;
  const float *wmap = P->root_link_mode != 0 ? P->alloc : P->wrench_map;  // (the map the kernels use: force rows 0..2 of [6][M])
  float col = 0.0f;  // sum over the motors of |force per unit thrust|: the body force is at most that times max |thrust|
  for (int j = 0; j < M; ++j) col += sqrtf(wmap[j] * wmap[j] + wmap[M + j] * wmap[M + j] + wmap[2 * M + j] * wmap[2 * M + j]);
  const float g = sqrtf(P->gravity[0] * P->gravity[0] + P->gravity[1] * P->gravity[1] + P->gravity[2] * P->gravity[2]);
  return (col * fmaxf(fabsf(P->max_thrust), fabsf(P->min_thrust)) / P->mass + g) * P->dt * 1.1f;
}

extern "C" float agx_step_proof_travel(int m, float speed, float dt, float vmax, float dv, int per_env) {
  if (m <= 0) return 0.0f;
  float travel = 0.0f;
  if (per_env) {
    travel = (float)m * dt * fminf(vmax, speed + (float)m * dv);  // (the device's proof_witness_bit, same expression)
  } else {
    float v = speed;
    for (int k = 0; k < m; ++k) {
      v = fminf(v + dv, vmax);
      travel += v * dt;
    }
  }
  return travel * 1.01f + 1.0e-3f;
}

extern "C" uint32_t agx_step_proof_witness_bit(int episode_len, int reset_on_collision, int steps, float dist, float speed, float dt,
                                               float max_linear_velocity, float dv) {
  return proof_witness_bit(episode_len, reset_on_collision, steps, dist, speed, dt, max_linear_velocity, dv);
}

extern "C" int agx_step_proof_decide(const uint32_t *record, const AgxStepProofQuery *q, int32_t *reason) {
  int32_t why = AGX_PROOF_PROVED;
  int mode = AGX_STEP_TWO;
  if (!record || !q) {
    why = AGX_PROOF_OFF;
  } else {
    // seqlock read: the writer stores [7] begin, the payload, [0] end, each acknowledged before the next
    volatile const uint32_t *h = record;
    const uint32_t end = h[0];
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    const uint32_t hz = h[1], ms = h[2], db = h[3], vb = h[4], fl = h[5];
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    const uint32_t begin = h[7];
    const uint32_t k = (q->now_tag - end) & 0x7FFFFFFFu;  // steps from the recorded step to this one
    float dist, speed;
    memcpy(&dist, &db, 4);
    memcpy(&speed, &vb, 4);
    if (end != begin) why = AGX_PROOF_TORN;
    else if (end == 0u) why = AGX_PROOF_NO_RECORD;
    else if (((end - q->min_tag) & 0x7FFFFFFFu) >= 0x40000000u) why = AGX_PROOF_VOID;  // recorded before the host's last interference
    else if (k == 0u || k > 64u) why = AGX_PROOF_TAG;
    else if (k <= AGX_PROOF_HORIZON && ((hz >> k) & 1u)) mode = AGX_STEP_ANY;  // a witness truncates in this step
    else if (fl & 1u) why = AGX_PROOF_RESET_NO_WITNESS;  // (the recorded maxima do not describe the envs that reset)
    else if ((int64_t)ms + (int64_t)k > (int64_t)q->episode_len) why = AGX_PROOF_MAY_TRUNCATE;
    else if (q->reset_on_collision && (!(speed == speed) ||  // (fminf would hide a NaN speed; a NaN distance fails the compare)
                                       !(dist + agx_step_proof_travel((int)k, speed, q->dt, q->max_linear_velocity, q->dv, 0) < 8.0f)))
      why = AGX_PROOF_MAY_CRASH;
    else mode = AGX_STEP_NONE;
  }
  if (reason) *reason = why;
  return mode;
}

extern "C" int agx_host_record_alloc(size_t bytes, void **out) {
  AGX_REQUIRE(out && bytes > 0 && bytes <= (1u << 20), "bad arguments");
  void *p = nullptr;
  const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent);
  if (e != hipSuccess) return fail(AGX_E_LAUNCH, "hipHostMalloc(%zu, mapped | coherent): %s", bytes, hipGetErrorString(e));
  memset(p, 0, bytes);
  *out = p;
  return AGX_OK;
}

extern "C" int agx_host_record_free(void *p) {
  if (p) (void)hipHostFree(p);
  return AGX_OK;
}

// Which form this step takes: the two launches without slots (not covered), the two launches with slots, or one launch.
static int position_step_mode(AgxPositionStepPlan *plan, const AgxTaskArgs &T, hipStream_t stream, bool *slots, int32_t *reason) {
  *slots = false;
  const AgxEnvBuffers *B = plan->buf;
  const AgxRobotParams *P = plan->params;
  if (!option_single_launch_step() || !plan->proof_slots || !plan->proof_record || !plan->proof_violation) {
    *reason = AGX_PROOF_OFF;
    return AGX_STEP_TWO;
  }
  const bool covered = plan->k_substeps == 1 && pick_block(plan->num_envs) == 64 && P->num_motors == 4 &&
                       P->controller == AGX_CTRL_POSITION && T.kind == AGX_TASK_POSITION && quad_kernel_usable(P, B, &T) &&
                       plan->reset->u_state == nullptr && B->episode_count && !B->step_rows[0] && !B->step_rows[1] &&
                       !B->step_signal && B->push_world <= 0 && !B->step_counter_dev && plan->obs && plan->target == T.target;
  if (!covered) {
    *reason = AGX_PROOF_NOT_COVERED;
    return AGX_STEP_TWO;
  }
  if (!plan->captured) {  // a step captured into a graph is replayed whatever the state is then, and the host does not see it
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) plan->captured = 1;
  }
  if (plan->captured) {
    *reason = AGX_PROOF_CAPTURE;
    return AGX_STEP_TWO;
  }
  *slots = true;
  const int max_lag = plan->max_lag > 0 ? plan->max_lag : 8;
  AgxStepProofQuery Q{};
  Q.now_tag = ((uint32_t)B->step_counter + 1u) & 0x7FFFFFFFu;
  Q.min_tag = plan->proof_min_tag;
  Q.episode_len = T.episode_len;
  Q.reset_on_collision = T.reset_on_collision;
  Q.dt = P->dt;
  Q.max_linear_velocity = P->max_linear_velocity;
  Q.dv = T.proof_dv;
  // Bounded run-ahead: a host that enqueues faster than the device executes gets ahead by the depth of the queue, and a record
  // from far back proves little.  More than max_lag steps ahead of the newest record, spin on it (no HIP call, at most 2 ms).
  // Only when the record can catch up: the last max_lag + 1 launches of this plan wrote slots.
  if (plan->slot_run > max_lag) {
    volatile const uint32_t *h = plan->proof_record;
    uint32_t k = (Q.now_tag - h[0]) & 0x7FFFFFFFu;
    if (h[0] != 0u && k > (uint32_t)max_lag && k <= 64u) {
      const auto t0 = std::chrono::steady_clock::now();
      // (lag_wait_ns / lag_waits: how much of the host's step time is this wait -- what is left is the host's own floor)
      const auto waited = [&] {
        plan->lag_waits += 1;
        plan->lag_wait_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
      };
      for (unsigned spin = 1;; ++spin) {
        k = (Q.now_tag - h[0]) & 0x7FFFFFFFu;
        if (k <= (uint32_t)max_lag || k > 64u) break;
        __builtin_ia32_pause();
        if ((spin & 255u) == 0u && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(2000)) {
          waited();
          *reason = AGX_PROOF_LAG;
          return AGX_STEP_TWO;
        }
      }
      waited();
    }
  }
  return agx_step_proof_decide(plan->proof_record, &Q, reason);
}

extern "C" int agx_position_task_step(AgxPositionStepPlan *plan, const float *actions_in, void *stream) {
  AGX_REQUIRE(plan && plan->params && plan->buf && plan->task && plan->reset, "null plan member");
  AGX_REQUIRE(plan->max_lag == 0 || (plan->max_lag >= 2 && plan->max_lag < AGX_PROOF_HORIZON), "max_lag %d outside 2 .. %d (0: 8)",
              plan->max_lag, AGX_PROOF_HORIZON - 1);
  plan->buf->flag_parity ^= 1;  // new env step: the flag the previous step's reset kernel cleared
  if (plan->buf->push_world > 0)
    if (int e = agx_push_advance(plan->buf)) return e;
  AgxTaskArgs T = *plan->task;
  T.proof_slots = nullptr;
  T.proof_record = nullptr;
  T.proof_violation = nullptr;
  T.proof_mode = AGX_STEP_TWO;
  T.proof_dv = agx_step_proof_dv(plan->params);
  bool slots = false;
  int32_t why = AGX_PROOF_OFF;
  const int mode = position_step_mode(plan, T, (hipStream_t)stream, &slots, &why);
  plan->last_mode = mode;
  plan->last_reason = why;
  plan->mode_count[mode] += 1;
  plan->reason_count[why] += 1;
  plan->slot_run = slots ? plan->slot_run + 1 : 0;
  if (slots) {
    T.proof_slots = plan->proof_slots;
    T.proof_record = plan->proof_record;
    T.proof_violation = plan->proof_violation;
    T.proof_mode = mode;
  }
  if (mode != AGX_STEP_TWO) {
    const AgxEnvBuffers *B = plan->buf;
    const int n = plan->num_envs;
    if (int e = check_reset(plan->params, B, n, plan->reset)) return e;
    AGX_REQUIRE(actions_in && B->state && B->derived && B->actions && B->prev_actions && B->motor_thrust && B->crashes && B->truncations &&
                    B->sim_steps && T.target && T.reward,
                "null buffer");
    const dim3 grid(blocks_for(n, 16) + 1);
    if (mode == AGX_STEP_ANY)
      hipLaunchKernelGGL(k_position_step_fused<AGX_STEP_ANY>, grid, dim3(128), 0, (hipStream_t)stream, *plan->params, *B, n, actions_in, T,
                         *plan->reset, plan->obs);  // (the step wave and its helper wave)
    else
      hipLaunchKernelGGL(k_position_step_fused<AGX_STEP_NONE>, grid, dim3(64), 0, (hipStream_t)stream, *plan->params, *B, n, actions_in, T,
                         *plan->reset, plan->obs);
    return check_launch("agx_position_task_step");
  }
  if (int e = agx_env_step(plan->params, plan->buf, plan->num_envs, actions_in, plan->k_substeps, &T, stream)) return e;
  // peer push: the env-step kernel has waited (one wave) until the slot of this step's rows was vacated; the observation
  // kernel behind it need not look again
  const uint32_t wait_seq = plan->buf->push_wait_seq;
  plan->buf->push_wait_seq = 0;
  const int rc = agx_post_step_position(plan->params, plan->buf, plan->num_envs, plan->reset, plan->target, plan->obs, stream);
  plan->buf->push_wait_seq = wait_seq;
  return rc;
}
