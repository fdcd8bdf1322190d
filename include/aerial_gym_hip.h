/*
 * aerial_gym_hip.h -- C ABI of libaerialgym_hip.so (gfx950 / MI355X).
 *
 * This is the drop-in boundary of the hot path.  The reference
 * (ntnu-arl/aerial_gym_simulator) has no FFI of its own: its "plugin API" is
 * Python (string registries + manager classes + one dict of aliasing tensors,
 * SURVEY.md section 8b).  Behind those Python classes the reference calls three
 * device back-ends -- PyTorch op chains, NVIDIA Warp kernels, and the Isaac Gym
 * (PhysX) C API.  Every entry point below replaces one such call site and cites
 * it.  The Python host (aerial_gym_simulator_amd/) binds them with ctypes, see
 * INTEGRATION.md for the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, sizes, a hipStream_t passed as void*;
 *     no torch / C++ types cross the boundary.
 *   - return 0 on success, negative on error (AGX_E_*); text via agx_last_error().
 *   - no allocation, no ownership transfer, stream-ordered, no host sync.
 *   - fp32 everywhere; quaternions are xyzw like the reference.
 *   - env state is SoA, component-major:  X[c * num_envs + env]
 *     (the reference is AoS [N, C]; the Python host exposes transposed views so
 *      `robot_position[N,3]` etc. keep their reference shapes).
 *   - images are [N, S, H, W] row-major exactly like the reference
 *     (warp_cam.py:134-149 writes pixels[env, cam, y, x]).
 */
#ifndef AERIAL_GYM_HIP_H
#define AERIAL_GYM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGX_ABI_VERSION 25  /* (agx_env_rollout / AgxRolloutRecord were ADDED under 25: a new symbol and a new struct, no existing
                               layout or signature changed, so a caller built against the earlier 25 header keeps working;
                               likewise the bf16 entries of the VAE encoder: new symbols and enums only) */
#define AGX_MAX_MOTORS 8
#define AGX_MAX_ACTIONS 8
#define AGX_MAX_SUBSTEPS 32
#define AGX_MAX_BODIES 24   /* rigid bodies (links) of one robot: base_quadrotor 9, base_octarotor 17 */

enum {
  AGX_OK = 0,
  AGX_E_ARG = -1,     /* bad argument (null pointer, size out of range)  */
  AGX_E_LAUNCH = -2,  /* hipLaunch / runtime error                       */
  AGX_E_UNSUPPORTED = -3
};

/* controller ids, one per class registered in aerial_gym/control/__init__.py:42-100 */
enum {
  AGX_CTRL_NONE = 0,          /* no_control                                            */
  AGX_CTRL_POSITION = 1,      /* LeePositionController     position_control.py:20      */
  AGX_CTRL_VELOCITY = 2,      /* LeeVelocityController     velocity_control.py:18      */
  AGX_CTRL_ATTITUDE = 3,      /* LeeAttitudeController     attitude_control.py:16      */
  AGX_CTRL_RATES = 4,         /* LeeRatesController        rates_control.py:16         */
  AGX_CTRL_ACCELERATION = 5,  /* LeeAccelerationController acceleration_control.py:16  */
  AGX_CTRL_VEL_STEERING = 6,  /* LeeVelocitySteeringAngleController  :15               */
  AGX_CTRL_FULLY_ACTUATED = 7,/* FullyActuatedController   fully_actuated_control.py:14 */
  AGX_CTRL_WRENCH = 8         /* EXTERNAL controller: any class registered through controller_registry.register_controller
                                 (registry/controller_registry.py:12-52) whose __call__(action) returns the body wrench
                                 [N, 6] (base_lee_controller.py:92-93).  The host evaluates it (torch) once per physics
                                 sub-step on freshly updated state tensors and hands its OUTPUT to agx_env_step as
                                 `actions_in` [N][6] with k_substeps = 1 and AgxEnvBuffers.launch_flags; allocation, motor
                                 model, drag, disturbance, integration, collision run in the kernel as usual.  num_actions
                                 stays the width of robot_actions (maintained by the host in this mode).               */
};

/* Constants shared by all envs.  Sources: config/robot_config/ *.py,
 * config/controller_config/ *.py, config/sim_config/base_sim_config.py,
 * resources/robots/<robot>/<robot>.urdf (composite mass/inertia computed as in
 * robots/robot_manager.py:295-435).                                          */
typedef struct AgxRobotParams {
  int32_t num_motors;
  int32_t num_actions;
  int32_t controller;
  int32_t root_link_mode;               /* force_application_level == "root_link" */
  float dt;
  float dt_over_6;                      /* float(dt / 6.0) with dt the config's double: the reference forms the RK4 weight
                                           from python scalars, `(dt / 6.0) * (k1 + ...)` (motor_model.py:198) -- not
                                           float(dt) / 6.0f, which is 1 ulp away for dt = 0.01                       */
  float gravity[3];
  float mass;
  float inertia[9];                     /* row-major, body frame, about COM       */
  float inertia_inv[9];
  float alloc[6 * AGX_MAX_MOTORS];      /* allocation_matrix, 6 x M row-major     */
  float alloc_pinv[AGX_MAX_MOTORS * 6]; /* pinv, M x 6 row-major                  */
  float wrench_map[6 * AGX_MAX_MOTORS]; /* body wrench per unit motor thrust when
                                           forces are applied at the motor links  */
  float motor_dir[AGX_MAX_MOTORS];
  float cq;
  int32_t use_rps;
  int32_t use_discrete_approximation;
  int32_t integration_rk4;
  float min_thrust, max_thrust, max_rate;
  float max_yaw_rate;
  float lin_drag_linear[3], lin_drag_quadratic[3];
  float ang_drag_linear[3], ang_drag_quadratic[3];
  float linear_damping, angular_damping;
  float max_linear_velocity, max_angular_velocity;
  float collision_radius;
  /* values used when the corresponding per-env buffer pointer in AgxEnvBuffers is NULL
   * (parameter not randomised: min == max in the config) -- saves the HBM reads          */
  float gains_uniform[12];              /* K_pos K_vel K_rot K_angvel                     */
  float tau_inc_uniform, tau_dec_uniform;
} AgxRobotParams;

/* Per-env device buffers of the dynamics path (all SoA, fp32 unless noted).
 * Keys in parentheses are the reference's global_tensor_dict names.          */
typedef struct AgxEnvBuffers {
  float *state;          /* [13][N] p q v w            (robot_state_tensor)            */
  float *derived;        /* [16][N] euler(3) qveh(4) vveh(3) vbody(3) wbody(3)
                            (robot_euler_angles, robot_vehicle_orientation,
                             robot_vehicle_linvel, robot_body_linvel, robot_body_angvel) */
  float *actions;        /* [A][N] (robot_actions)  -- written from actions_in        */
  float *prev_actions;   /* [A][N] (robot_prev_actions)                               */
  float *motor_thrust;   /* [M][N] MotorModel.current_motor_thrust                    */
  float *motor_kT;       /* [M][N] motor_thrust_constant (use_rps only)               */
  float *motor_tau_inc;  /* [M][N] motor_time_constants_increasing, or NULL (uniform)   */
  float *motor_tau_dec;  /* [M][N] motor_time_constants_decreasing, or NULL (uniform)   */
  float *gains;          /* [12][N] K_pos K_vel K_rot K_angvel (current values), or NULL (uniform) */
  float *wrench_cmd;     /* [6][N]  controller output of the LAST sub-step, or NULL     */
  uint8_t *crashes;      /* [N] bool (crashes)                                        */
  uint8_t *truncations;  /* [N] bool (truncations)                                    */
  int32_t *sim_steps;    /* [N]   EnvManager.sim_steps                                */
  uint8_t *reset_mask;   /* [N]   envs to reset = crashes*reset_on_collision | truncations
                            (env_manager.py:364-371), written by the task reward kernels          */
  int32_t *reset_flag;   /* [2]   device flags, double buffered by env-step parity: the task reward
                            (kernel or fused epilogue) ORs 1 into reset_flag[flag_parity] when any
                            env must reset; agx_reset_masked / agx_post_step_* read that entry and
                            clear the other one for the next step.  No host sync, no memset.     */
  int32_t flag_parity;   /* 0 / 1, toggled by the host once per env step                         */
  int32_t *episode_count;/* [N]   number of resets of each env (device RNG counter), or NULL     */
  float *bounds_min;     /* [3][N] (env_bounds_min)                                    */
  float *bounds_max;     /* [3][N] (env_bounds_max)                                    */
  /* optional inputs */
  const float *disturb;  /* [k][7][N] per sub-step (bernoulli outcome, 6 x U01), or NULL:
                            with disturb_prob > 0 the kernel then draws them itself (Philox,
                            counter = (env, step_counter, sub-step))                        */
  float disturb_max[6];
  float disturb_prob;    /* cfg.disturbance.prob_apply_disturbance, 0 = disabled           */
  int32_t step_counter;  /* env steps taken so far (host increments once per env step)      */
  uint64_t rng_seed;     /* key of the device generator                                     */
  const float *boxes;    /* [K][11][N] obstacle OBBs centre(3) quat(4) half(3) bounding radius(1), or NULL */
  int32_t num_boxes;
  /* optional multi-GPU exchange rows (ONE gather per env step).  When step_rows[p] is
     set, every kernel that writes the task observation (agx_post_step_position, agx_obs_position,
     agx_obs_navigation) also writes row i of step_rows[flag_parity] =
       obs(obs_dim) | reward | terminated (crashes) | truncated     ([N][obs_dim + 3] row-major)
     so the send buffer of the collective costs no extra launch.  Double buffered by step parity so
     the gather of step t may overlap step t+1.                                                 */
  float *step_rows[2];
  const float *step_reward; /* [N] the task's reward buffer (required when step_rows is set)     */
  /* optional, with step_rows: uint32 [4] in device memory, zero-initialised by the host.  The LAST
     wave of a row-writing kernel to finish stores step_signal[flag_parity] = step_counter + 1 (release,
     agent scope) after every row of that launch is visible device-wide ([2] is the kernel's own arrival
     counter).  The exchange's communication stream spins on it (agx_exchange_post, signal != NULL)
     instead of a cross-queue event: no host call per step for the producer side.                   */
  uint32_t *step_signal;
  /* optional PEER PUSH of the exchange rows (agx_exchange_create_push): step_rows[flag_parity] then points at THIS rank's own
     slice of a slot of its receive buffer, and every row store is repeated at the same offset in each peer's buffer
     (address + push_delta[j]: the peers' buffers are mapped into this process through hipIpcMemHandle) -- the rows of all
     ranks meet in every rank's buffer with no collective and no extra launch.  The last workgroup of a row-writing kernel
     then stores push_seq into entry push_flag_index of every rank's flag array (system-scope release).  Before its first
     row store such a kernel waits (device side, bounded) until entries push_wait_index .. + push_world of its OWN flag array
     have reached push_wait_seq: the slot it is about to overwrite has been vacated by every rank (0 = no wait).          */
  int64_t push_delta[7];       /* byte offsets own receive buffer -> peer j's, j < push_world - 1                           */
  uint32_t *push_flags[8];     /* flag arrays of ranks 0 .. push_world - 1 (own included), [slots][world] each             */
  int32_t push_world;          /* 0 = no peer push                                                                        */
  int32_t push_rank;
  int32_t push_flag_index;     /* slot * world + rank of this step                                                        */
  int32_t push_wait_index;     /* wait_slot * world                                                                       */
  int32_t push_pub_index;      /* flag entry of the PREVIOUS step's rows (published by the head of this step's first kernel) */
  uint32_t push_pub_seq;       /* ... and their sequence number (0 = nothing to publish)                                  */
  uint32_t push_seq;           /* sequence number of this step's rows (1, 2, ...)                                         */
  uint32_t push_wait_seq;
  uint32_t *push_timed_out;    /* device-visible host word: a wait that gave up stores the sequence number it waited for  */
  char *push_base;             /* this rank's receive buffer [push_slots][push_world][N][row]; with push_slice_bytes = N * row * 4
                                  and push_slots it lets agx_push_advance (called by agx_position_task_step) move to the next
                                  step without the host touching a field                                                  */
  int64_t push_slice_bytes;
  int32_t push_slots;
  float *body_force;     /* optional [3][N]: net applied (non-gravitational) force of the LAST sub-step in
                            the body frame = allocator output + drag + disturbance; read by agx_imu_update */
  const int32_t *step_counter_dev; /* optional, device memory: when set the kernels read the env-step index from here
                            instead of `step_counter` (whose value is frozen in a captured hipGraph); advance it with
                            agx_step_counter_advance as the last launch of the step                                    */
  int32_t env_index_base;/* global index of env 0 of these buffers (sharded runs: this rank owns global envs
                            [env_index_base, env_index_base + N)): first counter word of the device generator, so that
                            a draw is a function of (seed, GLOBAL env, episode | step, stream) whatever the sharding   */
  int32_t launch_flags;  /* 0 for the fused step.  An env step split over several agx_env_step launches (AGX_CTRL_WRENCH:
                            one per physics sub-step): bit 0 = not the first launch (crash flags accumulate, env_manager.py:
                            426-428), bit 1 = not the last launch (no sim_steps += 1, truncation or task epilogue yet),
                            bits 8-15 = index of the first physics sub-step of this launch (disturbance draws / rows).
                            bit 2 (AGX_LAUNCH_LEAN, fused step of a built-in controller, no navigation reward) = the tensors
                            that exist only to be looked at through the tensor dict are not maintained: derived[0..9]
                            (Euler angles, vehicle quaternion, vehicle-frame velocity), actions, prev_actions -- 88 of the
                            ~330 bytes an env moves per step; agx_update_states recomputes the derived tensors from the
                            current state on demand (the host mirror does that when a dict key is read).  The one-lane
                            kernels implement it (it is meant for batches far above 65 536 envs, where bytes matter).
                            bit 3 (AGX_LAUNCH_BODY_WRENCH, with AGX_CTRL_WRENCH only) = EXTERNAL ROBOT: `actions_in` [N][6] is
                            the NET body-frame wrench on the rigid composite about its centre of mass -- what the robot
                            object's step() left in robot_force_tensor / robot_torque_tensor, reduced by
                            agx_net_body_wrench -- and goes straight to the integrator: no allocation, motor model, drag or
                            disturbance in this launch (the robot's step() did whatever it does about them).
                            bit 16 (AGX_LAUNCH_ROV) = the robot is of the kind BaseROV (robots/base_rov.py of the reference): a
                            rigid body with eight fixed thrusters that differs from the multirotor in three places --
                            the quadratic drag on the linear velocity is per axis, -c_q[k] |v_body[k]| v_body[k]; the Euler
                            angles (derived[0..2]) are stored as get_euler_xyz returns them, in [0, 2 pi), not wrapped to
                            (-pi, pi]; a masked reset leaves motor_thrust, motor_kT, motor_tau_inc and motor_tau_dec of the
                            resetting envs as they are and consumes no motor draws (AgxResetArgs.u_tau_inc, u_tau_dec,
                            u_thrust, u_kT may be NULL).  Read by agx_env_step, agx_robot_step, agx_update_states,
                            agx_reset_masked and agx_post_step_position, which refuse it unless num_motors == 8 and the
                            controller is AGX_CTRL_FULLY_ACTUATED, AGX_CTRL_NONE or AGX_CTRL_WRENCH (the laws that read no
                            Euler angles); the other entry points that reset or refresh a robot refuse the flag.      */
} AgxEnvBuffers;
#define AGX_LAUNCH_LEAN 4
#define AGX_LAUNCH_BODY_WRENCH 8
#define AGX_LAUNCH_ROV 0x10000

const char *agx_last_error(void);
int agx_abi_version(void);
/* Identity of the BINARY: the hash (sha256[:16]) of the kernel sources, this header and the compile flags the library
 * was built from, embedded at compile time (aerial_gym_simulator_amd/_build.py).  Callers compare it with the hash of
 * the sources they see (`_build.source_hash()`): a stale library shipped next to newer sources is detected whatever its
 * file times say; bench.py stamps committed counter files with it.                                                     */
const char *agx_build_id(void);

/* Process-wide tuning / A-B options of the library (none changes a result: every setting is bit-identical, tests hold that).
 * They replace the environment variables rounds 1-5 read inside the launch paths (AGX_ENV_STEP_QUAD, AGX_RAY_SPLIT): the
 * library reads NO environment variable.
 *   "env_step_quad"  1 (default): the four-lanes-per-env kernels where they apply; 0: one lane per env everywhere
 *   "ray_split"      0 (default): workgroups per (env, sensor) image by the launch policy (csrc/agx_raycast.hip
 *                    ray_split_policy); n > 0: that many (clamped to the image's tiles)
 *   "single_launch_step"  1 (default): agx_position_task_step issues a step as ONE launch when its record proves the
 *                    outcome of the batch-wide reset OR; 0: always the two launches
 * agx_set_option returns AGX_E_ARG for an unknown name or a value out of range; agx_get_option reads the current value.  */
int agx_set_option(const char *name, int value);
int agx_get_option(const char *name, int *value);

/* ---- dynamics -------------------------------------------------------------------
 * agx_dynamics_substeps: `k` physics sub-steps of every env, fused in one launch.
 * Replaces, per sub-step: RobotManagerIGE.pre_physics_step (robot_manager.py:486-489),
 * BaseMultirotor.step (base_multirotor.py:296-307: update_states, clip, controller,
 * ControlAllocator.allocate_output control_allocation.py:52-114, MotorModel
 * motor_model.py:88-138, simulate_drag, apply_disturbance),
 * gym.apply_rigid_body_force_tensors + gym.simulate + refresh_* (IGE_env_manager.py:
 * 444-449,477,486-495) and EnvManager.compute_observations (env_manager.py:358-362);
 * plus reset_tensors / sim_steps += 1 of EnvManager.step (env_manager.py:399-432).
 * actions_in: [N][A] row-major, exactly the tensor the policy hands to task.step().  */
int agx_dynamics_substeps(const AgxRobotParams *params, const AgxEnvBuffers *buf, int num_envs,
                          const float *actions_in, int k_substeps, void *stream);

/* Task epilogue fused into the env step (same arithmetic as agx_reward_position /
 * agx_reward_navigation, evaluated on the registers of the dynamics kernel).             */
enum { AGX_TASK_NONE = 0, AGX_TASK_POSITION = 1, AGX_TASK_NAVIGATION = 2 };
typedef struct AgxTaskArgs {
  int32_t kind;               /* AGX_TASK_*                                                */
  int32_t episode_len;        /* truncations = sim_steps > episode_len                     */
  int32_t reset_on_collision; /* cfg.env.reset_on_collision                                */
  float curriculum_progress;  /* navigation only                                           */
  const float *target;        /* [3][N]                                                    */
  float *reward;              /* [N]                                                       */
  float *pos_err;             /* [3][N] navigation only (in/out)                           */
  float *prev_pos_err;        /* [3][N] navigation only (out)                              */
  float rp[18];               /* navigation reward parameters                              */
  /* navigation bookkeeping in the same epilogue (navigation_task.py:311-326; what agx_nav_bookkeeping does as a launch of its
   * own): all three NULL = not done here.  successes = truncated & |target - p| < success_radius & not crashed; timeouts =
   * truncated & not success & not crashed; counters[0..2] += number of (successes, crashes, timeouts) of this step.          */
  uint8_t *successes;         /* [N] */
  uint8_t *timeouts;          /* [N] */
  int32_t *counters;          /* [3] */
  float success_radius;
  int32_t reserved;
  /* Single-launch position steps (AgxPositionStepPlan.proof_*): set by agx_position_task_step on its own copy for the
   * four-lanes-per-env kernels; every other caller leaves them zero.                                                        */
  uint32_t *proof_slots;      /* device [2][blocks][AGX_PROOF_SLOT_WORDS]: what each wave saw at the END of its step       */
  uint32_t *proof_record;     /* mapped host [AGX_PROOF_RECORD_WORDS]: the previous launch's slots, folded (seqlock)         */
  uint32_t *proof_violation;  /* device [1]: +1 per broken proof (must stay 0)                                                */
  float proof_dv;             /* bound on the growth of |v| per env step: (M max|thrust| / mass + |g|) dt 1.1               */
  int32_t proof_mode;         /* AGX_STEP_TWO / AGX_STEP_ANY / AGX_STEP_NONE: what this launch is                           */
} AgxTaskArgs;

/* agx_env_step = agx_dynamics_substeps + the task's reward / crash / truncation / reset-set
 * in ONE launch (task may be NULL or kind NONE).                                           */
int agx_env_step(const AgxRobotParams *params, const AgxEnvBuffers *buf, int num_envs,
                 const float *actions_in, int k_substeps, const AgxTaskArgs *task, void *stream);

/* Which kernel instance agx_env_step launches for these arguments, as "<kernel name incl. template arguments>_<grid size
 * in threads>" (e.g. "k_env_step<4,2,false,true>_8192", "k_env_step_quad_position_32768"): the key under which profilers
 * list it (bench.py pairs its live launch time with the committed rocprofv3 counters of that instance).             */
int agx_env_step_kernel(const AgxRobotParams *params, const AgxEnvBuffers *buf, int num_envs, int k_substeps,
                        const AgxTaskArgs *task, char *out, int out_capacity);

/* agx_env_step for a multirotor whose centre of mass is NOT the base-link origin (an asymmetric payload; the reference's
 * base_random).  com->c: the composite's centre of mass in the base-link frame [m].  The state tensor keeps the reference's
 * meaning (the PhysX tensor convention): position and attitude are the base-link frame's, the linear velocity is the velocity
 * of the mass centre, the angular velocity the body's.  Against agx_env_step two things change, per physics sub-step:
 *   - the root body's entry of robot_force_tensor -- the allocator's wrench in root-link mode, plus drag, plus disturbance --
 *     acts at the base-link origin: its force F_root adds the torque cross(F_root, c) about the mass centre.  (The motor
 *     links' arms are in params->wrench_map, which is about the mass centre; a net body wrench handed in under
 *     AGX_LAUNCH_BODY_WRENCH is about the mass centre already, agx_net_body_wrench with pos = xyz - com.)
 *   - the integrator moves the mass centre and turns the body about it: behind its p' = p + v dt,
 *     p'' = p' + (quat_rotate(q, c) - quat_rotate(q', c)) with q, q' the attitude before and after the update.
 * Everything that reads the state -- controllers, rewards, observations, the collision sphere (centred at p), sensor poses --
 * reads it as before.  c = 0 is the ordinary dynamics.  Runs the one-lane kernels k_env_step_com<M, CTRL, SINGLE, WIDE> at every
 * batch size, for 4 and 8 motors under every controller id.  Refused (AGX_E_ARG): AGX_LAUNCH_ROV, AGX_LAUNCH_LEAN, another
 * motor count, a non-NULL buf->body_force (the IMU's lever-arm terms are not modelled).                                     */
typedef struct AgxComOffset {
  float c[3];
  float reserved;
} AgxComOffset;
int agx_env_step_com(const AgxRobotParams *params, const AgxEnvBuffers *buf, int num_envs, const float *actions_in, int k_substeps,
                     const AgxTaskArgs *task, const AgxComOffset *com, void *stream);

/* Open-loop rollout: `steps` env steps of the task-free multirotor step in ONE launch (k_env_step_rollout<M, CTRL, WIDE>), in place
 * of the reference's one-call-per-step loops under known actions -- EnvManager.step (env_manager.py:399-432) driven `steps`
 * times, as examples/sys_id.py:56-90 does 500 times per action axis with a host copy of one dict tensor after every step.
 * The buffers end where `steps` calls agx_env_step(params, buf, n, actions_t, k_t, NULL, stream) leave them, bit for bit, with
 * buf->step_counter advanced by one between the calls (step t draws its device-generator disturbance from stream index
 * (buf->step_counter + t) & 0x7FFFFFFF): state, derived (one sub-step stale), motor_thrust, actions / prev_actions, crashes and
 * truncations (the last step's), sim_steps (+ steps), wrench_cmd where bound.  The state stays in registers in between.
 *   actions            float [N][A] with actions_per_step == 0 (held for every step), [steps][N][A] with actions_per_step == 1
 *   substeps           physics sub-steps of every step, 0 .. AGX_MAX_SUBSTEPS; with substeps_per_step: the LARGEST count in it
 *                      (the launch sizes the sub-step positions in LDS by it; a larger entry is cut to it, a negative one to 0)
 *   substeps_per_step  device int32 [steps], or NULL.  A count of 0: the step only counts (sim_steps + 1, crashes = 0)
 *   record             NULL, or what to store after every step: channel c of step t goes to out[(t * channels + c) * N + env],
 *                      component-major, a plain store nothing waits for.  source[c] / component[c] name the value:
 *                        AGX_REC_STATE   0..12  position xyz, quaternion xyzw, linear velocity, angular velocity
 *                        AGX_REC_DERIVED 0..15  Euler angles, vehicle-frame quaternion xyzw, vehicle-frame linear velocity,
 *                                               body-frame linear velocity, body-frame angular velocity (buf->derived rows)
 *                        AGX_REC_THRUST  0..M-1 motor thrusts
 *                        AGX_REC_CRASH   0      this step's crash flag as 0.0f / 1.0f
 *                      each (source, component) at most once, at most AGX_ROLLOUT_MAX_CHANNELS channels
 *   first_crash_step   int32 [N] or NULL: the first step whose crash flag was set, or -1 (a crashed env keeps flying, as in
 *                      the separate calls)
 * Refused (AGX_E_ARG): AGX_CTRL_WRENCH, any launch_flags bit (split step, AGX_LAUNCH_LEAN, AGX_LAUNCH_ROV), buf->disturb,
 * buf->body_force, buf->step_counter_dev, bound exchange rows / peer push; AGX_E_UNSUPPORTED: a motor count other than 4, 6, 8.
 * No allocation, stream-ordered; one-wave workgroups up to 65536 envs, 256-thread workgroups above.                          */
#define AGX_ROLLOUT_MAX_CHANNELS 32
enum { AGX_REC_STATE = 0, AGX_REC_DERIVED = 1, AGX_REC_THRUST = 2, AGX_REC_CRASH = 3 };
typedef struct AgxRolloutRecord {
  float *out;                                   /* [steps][channels][N]                 */
  int32_t channels;                             /* 1 .. AGX_ROLLOUT_MAX_CHANNELS        */
  int32_t reserved;
  int32_t source[AGX_ROLLOUT_MAX_CHANNELS];     /* AGX_REC_*                            */
  int32_t component[AGX_ROLLOUT_MAX_CHANNELS];  /* row of that source                   */
} AgxRolloutRecord;
int agx_env_rollout(const AgxRobotParams *params, const AgxEnvBuffers *buf, int num_envs, const float *actions, int actions_per_step,
                    int steps, int substeps, const int *substeps_per_step, const AgxRolloutRecord *record, int *first_crash_step,
                    void *stream);

/* EnvManager.compute_observations alone (env_manager.py:358-362; SURVEY 8b's minimum export set): crashes[i] |= the robot's
 * collision sphere (params->collision_radius) at its CURRENT position overlaps one of the env's obstacle boxes (buf->boxes,
 * the layout agx_boxes_from_assets writes).  The fused step accumulates the same predicate over its sub-step positions; this
 * entry point is for callers that drive simulate() / compute_observations() themselves.  No boxes bound: no-op.            */
int agx_collide_spheres_boxes(const AgxRobotParams *params, const AgxEnvBuffers *buf, int num_envs, void *stream);

/* BaseMultirotor.update_states alone (base_multirotor.py:287-294). */
int agx_update_states(const AgxEnvBuffers *buf, int num_envs, void *stream);

/* The elementary functions the kernels evaluate in place of torch.sin / cos / atan2 / asin / exp (utils/math.py:124-172,
 * base_lee_controller.py:136-215, the reward functions' torch.exp), on device vectors: out[i] = f(x[i]) (atan2:
 * atan2(x[i], y[i]), x = the "y" argument).  float64 inside, rounded once: correctly rounded in practice.  Diagnostic
 * entry: the parity tests compare it bit for bit with the CPU restatement.                                          */
enum { AGX_MATH_SIN = 0, AGX_MATH_COS = 1, AGX_MATH_ATAN2 = 2, AGX_MATH_ASIN = 3, AGX_MATH_EXP = 4,
       AGX_MATH_EXPM1 = 5 /* expm1_cw: the negative branch of ELU (agx_vae.hip), where torch evaluates expm1 */,
       AGX_MATH_SIGMOID = 6, AGX_MATH_TANH = 7 /* sigmoid_cw, tanh_cw: the gates of the recurrent cell (agx_policy.hip) */ };
int agx_math_eval(int which, int n, const float *x, const float *y, float *out, void *stream);

/* Diagnostic: float4 streaming copy of `bytes` (multiple of 16) from src to dst -- the HBM rate a kernel of this library
 * reaches on the device at hand (bench.py's "achievable" HBM line next to the 8 TB/s of specification).            */
int agx_copy_f4(const void *src, void *dst, size_t bytes, void *stream);

/* Controller plug-in entry: BaseLeeController subclasses' update(), returning the wrench
 * [6][N] into buf->wrench_cmd (control/controllers/ *.py).  Uses buf->state/derived as is.
 * action: [N][A] row-major (clipped to +-10 like BaseMultirotor.clip_actions).          */
int agx_controller_wrench(const AgxRobotParams *params, const AgxEnvBuffers *buf, int num_envs,
                          const float *action, void *stream);

/* ---- robot plug-in (robots/base_robot.py:10-63, robot_manager.py:486-489) ------------------------------
 * A robot CLASS registered through robot_registry.register that overrides step(action) is called by the host once per
 * physics sub-step, like the reference's RobotManagerIGE.pre_physics_step does; what it leaves in robot_force_tensor /
 * robot_torque_tensor ([N][num_bodies][3], each body's wrench in that BODY's own frame: IGE_env_manager.py:444-449 applies
 * them with LOCAL_SPACE) is reduced to the net wrench on the rigid composite (agx_net_body_wrench) and integrated by
 * agx_env_step with AGX_CTRL_WRENCH + AGX_LAUNCH_BODY_WRENCH.
 *
 * agx_robot_step = the reference's BaseMultirotor.step(action) (base_multirotor.py:296-307) as ONE launch, for such a class
 * to call through super().step(action): update_states (derived tensors stored), clip_actions, the built-in controller,
 * ControlAllocator.allocate_output + MotorModel (motor thrusts stored; control_allocation.py:52-114), the per-body tensors
 * written like call_controller does (:246-258: every body zero, then motor link j <- force (0, 0, u_j), torque
 * (0, 0, -cq dir_j u_j); root-link mode: body_of_motor[0] <- the allocator's wrench), simulate_drag and apply_disturbance
 * accumulated into body 0 (:213-234, :260-285; buf->disturb rows of sub-step `substep`, or the device stream).          */
typedef struct AgxRobotStepArgs {
  float *force;                          /* [N][num_bodies][3] robot_force_tensor  (row-major, the reference's layout) */
  float *torque;                         /* [N][num_bodies][3] robot_torque_tensor                                      */
  int32_t num_bodies;                    /* 1 .. AGX_MAX_BODIES                                                         */
  int32_t substep;                       /* physics sub-step inside the env step (disturbance draws)                    */
  int32_t body_of_motor[AGX_MAX_MOTORS]; /* control_allocator_config.application_mask                                   */
} AgxRobotStepArgs;
int agx_robot_step(const AgxRobotParams *params, const AgxEnvBuffers *buf, int num_envs, const float *action /*[N][A]*/,
                   const AgxRobotStepArgs *args, void *stream);

/* Net body-frame wrench about the centre of mass of per-body wrenches given in each body's own frame:
 *   F = sum_b R_b f_b,   T = sum_b (r_b x (R_b f_b) + R_b t_b)     (b ascending, fp32, one IEEE operation per + - *)
 * rot / pos: pose of body b in the root-link frame (URDF joint origins), about the composite's centre of mass.
 * wrench_out: [N][6] row-major -- the `actions_in` of agx_env_step under AGX_LAUNCH_BODY_WRENCH.                        */
typedef struct AgxLinkFrames {
  int32_t num_bodies;
  int32_t reserved;
  float rot[AGX_MAX_BODIES][9];          /* row-major 3 x 3 */
  float pos[AGX_MAX_BODIES][3];
} AgxLinkFrames;
int agx_net_body_wrench(int num_envs, const AgxLinkFrames *frames, const float *force, const float *torque,
                        float *wrench_out, void *stream);

/* ---- tasks ----------------------------------------------------------------------
 * Position-setpoint task: compute_rewards_and_crashes + truncation test
 * (position_setpoint_task.py:205-229,245-282,172-174).  Writes reward[N], ORs the
 * distance crash into crashes, truncations = sim_steps > episode_len, and sets
 * *buf->reset_flag to 1 if any env is to be reset
 * (env_manager.py:364-371: crashes*reset_on_collision + truncations).            */
int agx_reward_position(const AgxEnvBuffers *buf, int num_envs, const float *target /*[3][N]*/,
                        int episode_len, int reset_on_collision, float *reward, void *stream);

/* process_obs_for_task (position_setpoint_task.py:194-203): obs [N][13] row-major. */
int agx_obs_position(const AgxEnvBuffers *buf, int num_envs, const float *target, float *obs,
                     void *stream);

/* Navigation task reward (navigation_task.py:416-521).  rp: 18 floats in the order of
 * config/task_config/navigation_task_config.py:30-48.  pos_err / prev_pos_err [3][N]. */
int agx_reward_navigation(const AgxEnvBuffers *buf, int num_envs, const float *target,
                          const float *rp, float curriculum_progress, float *pos_err,
                          float *prev_pos_err, int episode_len, int reset_on_collision,
                          float *reward, void *stream);

/* process_obs_for_task of the navigation task (navigation_task.py:369-393): obs [N][obs_dim]
 * row-major = unit vector to target (+0.2 U01 noise) | distance | roll, pitch (+-0.05 noise) | 0 |
 * body lin/ang velocity | robot_actions(4) | latents.  u_vec, u_euler: [N][3] U01 draws, or both
 * NULL = device generator (stream of (env, buf->step_counter)).
 * The reference fills the latents with a VAE encoding of the depth image: with vae_config.use_vae the
 * host passes pixels == NULL, which leaves the latent slots untouched, and places the encoder's output
 * there itself (the "VAE depth-image encoder" section at the end of this header).  Without the encoder
 * latents = grid_h x grid_w min-pooled depth image (pixels [N][S][H][W], sensor 0).
 * min_pixel [N] (optional, num_sensors == 1 only): what agx_image_min would write
 * (post_image_reward_addition, navigation_task.py:351-357), produced by the same sweep over the
 * image.                                                                                    */
int agx_obs_navigation(const AgxEnvBuffers *buf, int num_envs, const float *target,
                       const float *u_vec, const float *u_euler, const float *pixels,
                       int num_sensors, int height, int width, int grid_h, int grid_w,
                       int obs_dim, float *obs, float *min_pixel, void *stream);

/* ---- LiDAR navigation task (task/lidar_navigation_task/lidar_navigation_task.py) -----------
 * process_image_observation (:313-363) + add_noise_to_downsampled_lidar_data (:281-310):
 * pointcloud [N][H][W][3] in the world frame (sensor 0) -> range = |p - robot_position| clipped to
 * 10 outside [0.2, 10]; time_to_collision [N] = clamp(min over rays of range / (v . dir), 0, 10);
 * pool_h x pool_w min-pooling; noise; downsampled [N][(H/pool_h) * (W/pool_w)] = 1 / range.
 * Noise: device_noise = 0 and the five tensors ([N][cells]; 0/1 masks as floats, low_* only read
 * for pooled rows >= low_row0; all may be NULL = no noise) reproduce the reference's torch draws;
 * device_noise = 1 draws from the device generator (stream of env, buf->step_counter).          */
int agx_lidar_image_obs(const AgxEnvBuffers *buf, int num_envs, int height, int width, int pool_h,
                        int pool_w, int low_row0, const float *pointcloud, const float *noise_mask,
                        const float *noise_val, const float *max_mask, const float *low_mask,
                        const float *low_val, int device_noise, float *time_to_collision,
                        float *downsampled, void *stream);

/* compute_rewards_and_crashes + compute_reward (:472-719) + truncation / reset set (:399-403, like
 * agx_reward_navigation).  action / prev_action: the task's transformed actions [N][4] row-major;
 * rp: HOST pointer to the 22 reward parameters in the order of lidar_navigation_task_config.py:30-53;
 * target [3][N], target_yaw [N], pos_err / prev_pos_err [3][N].                                  */
int agx_reward_lidar_navigation(const AgxEnvBuffers *buf, int num_envs, const float *target,
                                const float *target_yaw, const float *action,
                                const float *prev_action, const float *time_to_collision,
                                const float *rp, float curriculum_progress, float *pos_err,
                                float *prev_pos_err, int episode_len, int reset_on_collision,
                                float *reward, void *stream);

/* ---- Radar navigation task (task/radar_navigation_task/radar_navigation_task.py), a subclass of the LiDAR
 * task: its process_image_observation (:24-63) + add_noise_to_downsampled_lidar_data (:6-21).  Ranges,
 * time_to_collision and the pool_h x pool_w min-pooling as in agx_lidar_image_obs (the same point pass);
 * then, per pooled cell: m += noise_val where noise_mask == 1, m = -1 where invalid_mask == 1,
 * downsampled = 1 / m (an invalid cell reads -1, a valid one lies in [1/20, 5]).  device_noise = 0: the
 * three tensors ([N][cells]; 0/1 masks as floats; a NULL pointer = no such mask) reproduce the reference's
 * torch draws; device_noise = 1: device generator, stream RNG_RADAR_NOISE of (env, buf->step_counter), one
 * block per cell: u0 < 0.03 -> m += 9.8 u1 + 0.2; u2 < 0.8 -> m = -1.                                   */
int agx_radar_image_obs(const AgxEnvBuffers *buf, int num_envs, int height, int width, int pool_h,
                        int pool_w, const float *pointcloud, const float *noise_mask,
                        const float *noise_val, const float *invalid_mask, int device_noise,
                        float *time_to_collision, float *downsampled, void *stream);

/* agx_reward_lidar_navigation with the radar task's compute_reward (:179-342): negative_x_vel_penalty
 * takes clamp(v_x, max = 0) (:242-246) instead of clamp(v_x, min = 0); everything else, the truncation and
 * the reset set are the same code.  rp in the order of radar_navigation_task_config.py:30-53.            */
int agx_reward_radar_navigation(const AgxEnvBuffers *buf, int num_envs, const float *target,
                                const float *target_yaw, const float *action,
                                const float *prev_action, const float *time_to_collision,
                                const float *rp, float curriculum_progress, float *pos_err,
                                float *prev_pos_err, int episode_len, int reset_on_collision,
                                float *reward, void *stream);

/* process_obs_for_task (:440-470): obs [N][17 + cells] = unit vector to target (+-0.1 noise) |
 * distance | roll, pitch (+-0.05 noise) | yaw error | body lin/ang velocity | robot_actions(4) |
 * downsampled.  u_vec / u_euler [N][3] U01 draws, or both NULL = device generator.              */
int agx_obs_lidar_navigation(const AgxEnvBuffers *buf, int num_envs, const float *target,
                             const float *target_yaw, const float *u_vec, const float *u_euler,
                             const float *downsampled, int cells, float *obs, void *stream);

/* *buf->step_counter_dev = (*buf->step_counter_dev + 1) mod 2^31, stream-ordered: the last node of an env step that is
 * captured into a hipGraph and replayed (small batches are launch bound: ~15 launches per navigation step).           */
int agx_step_counter_advance(const AgxEnvBuffers *buf, void *stream);

/* task_config.action_transformation_function of the reference's task configs as one launch: policy action [N][4] (clamped
 * to +-1) -> controller command.  NAV_VELOCITY: navigation_task_config.py:87-117 (speed, inclination, yaw rate -> [N][4]);
 * LIDAR_ACCELERATION: lidar_navigation_task_config.py:98-108 ([N][4]); FULLY_ACTUATED_POSE: the 7-D position + attitude
 * set-point of BASELINE configs[3] ([N][7]).  A user-supplied function (any other callable in the config) stays torch.   */
enum { AGX_ACTION_NAV_VELOCITY = 1, AGX_ACTION_LIDAR_ACCELERATION = 2, AGX_ACTION_FULLY_ACTUATED_POSE = 3 };
int agx_action_transform(int kind, int num_envs, const float *actions_in, float *out, void *stream);

/* ---- the lmf2 sim2real set-point tasks (position_setpoint_task_sim2real.py, position_setpoint_task_acceleration_sim2real.py) ----
 * Three launches of one lane per env around the env step.  target: [3][N]; the action tensors are [N][4] row-major and
 * 16-byte aligned (`actions` IS the tensor the caller handed to task.step()); the vehicle-frame tensors are read and written
 * by the acceleration kind only (NULL otherwise).
 *
 * agx_sim2real_pre_step: step() up to sim_env.step (velocity :157-161, acceleration :161-170), in that order:
 *   prev_actions <- actions_before (what task.actions reads at the time of the call: the previous call's tensor, possibly
 *   overwritten by the caller since, possibly `actions` itself), prev_dist <- |target - robot_position| on the pre-step
 *   position; acceleration kind: prev_actions_vehicle_frame[0:3] <- quat_rotate(robot_orientation, prev_actions[0:3]),
 *   [3] copied (:162-165), then actions[:, 0:3] *= 2 in place (:170).                                                        */
enum { AGX_SIM2REAL_VELOCITY = 0, AGX_SIM2REAL_ACCELERATION = 1 };
int agx_sim2real_pre_step(int kind, const AgxEnvBuffers *buf, int num_envs, const float *target, const float *actions_before,
                          float *actions, float *prev_actions, float *prev_dist, float *prev_actions_vehicle_frame,
                          void *stream);

/* compute_rewards_and_crashes + compute_reward (velocity :230-259,286-339; acceleration :239-273,300-356: different constants)
 * and `truncations = sim_steps > episode_len` (:180-182 / :189-191).  Reads buf->state and the derived tensors as the env
 * step left them; writes reward[N], actions_vehicle_frame (acceleration: quat_rotate(robot_vehicle_orientation, actions[0:3])),
 * ORs `dist > 10` into crashes, reward = -50 where crashed, and leaves reset_mask / reset_flag[flag_parity] exactly as
 * agx_reward_position does (env_manager.py:364-371).                                                                         */
int agx_sim2real_reward(int kind, const AgxEnvBuffers *buf, int num_envs, const float *target, const float *actions,
                        const float *prev_actions, const float *prev_dist, float *actions_vehicle_frame,
                        const float *prev_actions_vehicle_frame, int episode_len, int reset_on_collision, float *reward,
                        void *stream);

/* process_obs_for_task (:202-228 / :211-237, identical in both tasks): obs [N][17] row-major = position error + 0.03 z_p |
 * quat_from_euler_xyz(ssa(euler_xyz(q)) + 0.02 z_e) | body linvel + 0.02 z_v | body angvel + 0.02 z_w | robot_actions, where
 * q = sign(w) * robot_orientation is STORED BACK into buf->state like the reference's in-place write (:204-207; sign is 0 at
 * +-0).  noise: standard normals [4][N][3] in the reference's randn_like order (euler, position, linvel, angvel).  Exchange
 * rows (buf->step_rows) are not written for this observation: the call refuses them.                                       */
int agx_sim2real_obs(const AgxEnvBuffers *buf, int num_envs, const float *target, const float *noise, float *obs,
                     void *stream);

/* ---- the end-to-end motor-command set-point task (position_setpoint_task_sim2real_end_to_end.py: tinyprop, no_control) ----
 * Four launches per step: pre-step, the env step, reward, and the step's tail (reset + observation + bookkeeping).  target,
 * prev_position and prev_pos_error are [3][N]; actions / prev_actions are the task's own [N][4] row-major tensors, 16-byte
 * aligned; obs is [N][15] row-major.
 *
 * Pre-step: step() up to sim_env.step (:164-168).  actions <- clamp(actions_in, -1, 1) * (max - min) / 2 + (max + min) / 2 per
 * column (task_config.process_actions_for_task, ..._end_to_end_config.py:28-33; actions_in is neither kept nor changed), and
 * prev_position <- robot_position.  limits: HOST pointer, passed to the kernel by value.                                     */
typedef struct AgxEndToEndLimits {
  float min[4], max[4];  /* task_config.action_limit_min / action_limit_max */
} AgxEndToEndLimits;
int agx_end_to_end_pre_step(const AgxEnvBuffers *buf, int num_envs, const float *actions_in, const AgxEndToEndLimits *limits,
                            float *actions, float *prev_position, void *stream);

/* The constants of compute_reward (:267-309) as one table (HOST pointer, passed by value): a sibling task with other numbers is
 * another instance.  exp_func(x, gain, exp) = gain * exp(-exp * x * x), exp_penalty_func = gain * (exp(-exp * x * x) - 1).   */
typedef struct AgxEndToEndReward {
  float z_error_weight;               /* pos_error[:, 2] *= 11 (:282), after both distances were taken                  */
  float pos_gain[2], pos_exp[2];      /* the two per-component position terms (:283): (10, 10) and (2, 2)               */
  float upright_gain, upright_exp;    /* on 1 - quat_axis(q, 2).z (:285-287): 2.5, 5                                    */
  float alignment_gain, alignment_exp;/* on 1 - quat_axis(q, 0).x (:289-291): 6, 5                                      */
  float angvel_gain, angvel_exp;      /* per component of robot_body_angvel (:293): 0.3, 10                             */
  float vel_gain, vel_exp;            /* per component of robot_linvel (:294): 1, 5                                     */
  float hover_thrust;                 /* 9.81 * 0.372 / 4 (:296): a double, rounded to float once                       */
  float action_gain, action_exp;      /* penalty on action - hover_thrust (:297): 0.01, 10                              */
  float closer_gain, farther_gain;    /* the two-sided towards_goal_reward (:300): 10, 15                               */
  float diff_gain, diff_exp;          /* penalty on action - prev_action (:303): 1.3, 6                                 */
  float divisor;                      /* :305: 100                                                                      */
} AgxEndToEndReward;
/* Reward: compute_rewards_and_crashes + compute_reward (:232-252, 267-309) and `truncations = sim_steps > episode_len` (:176-178).
 * Reads buf->state (position, orientation, world linear velocity) and robot_body_angvel of buf->derived as the env step left
 * them; writes reward[N], ORs `|target - position| > crash_dist` into crashes (the reward is NOT replaced there) and leaves
 * reset_mask / reset_flag[flag_parity] exactly as agx_sim2real_reward does (env_manager.py:364-371).                           */
int agx_end_to_end_reward(const AgxEnvBuffers *buf, int num_envs, const float *target, const float *actions,
                          const float *prev_actions, const float *prev_pos_error, const AgxEndToEndReward *constants,
                          float crash_dist, int episode_len, int reset_on_collision, float *reward, void *stream);

/* Observation: process_obs_for_task (:204-225).  obs row = position error + 0.001 z_p | rotation_6d of the attitude whose "ZYX"
 * Euler angles carry pi / 1032 z_o each (pytorch3d quaternion_to_matrix -> matrix_to_euler_angles -> euler_angles_to_matrix ->
 * matrix_to_rotation_6d; no clamp in front of asin: NaN where the reference gives NaN) | robot_linvel + 0.002 z_v |
 * robot_body_angvel + 0.001 z_w.  noise: standard normals [4][N][3] in the reference's draw order (position, orientation, linear
 * velocity, angular velocity), or NULL = twelve normals per env from the device generator, a function of (rng_seed, env_index_base
 * + env, env step).  Exchange rows (buf->step_rows) are not written for this observation: the call refuses them.               */
int agx_end_to_end_obs(const AgxEnvBuffers *buf, int num_envs, const float *target, const float *noise, float *obs,
                       void *stream);
/* Diagnostic: noise_out [4][N][3] <- the normals the NULL-noise form above draws at this env step.                            */
int agx_end_to_end_noise(const AgxEnvBuffers *buf, int num_envs, float *noise_out, void *stream);

/* The reset set of EnvManager.reset_terminated_and_truncated_envs (env_manager.py:364-371) from the flags as they are:
 * reset_mask = crashes * reset_on_collision | truncations, reset_flag[flag_parity] |= any.  For callers that did not
 * run one of the task reward kernels above this step (stand-alone EnvManager; tasks that set truncations in torch). */
int agx_reset_set(const AgxEnvBuffers *buf, int num_envs, int reset_on_collision, void *stream);

/* ---- task glue of the navigation-type tasks (sync-free mode: no torch launches per step) ----
 * successes / timeouts (navigation_task.py:311-326, lidar_navigation_task.py:405-418): u8 [N] each;
 * counters int32[3] += (sum successes, sum crashes, sum timeouts) for the curriculum.            */
int agx_nav_bookkeeping(const AgxEnvBuffers *buf, int num_envs, const float *target, float radius,
                        uint8_t *successes, uint8_t *timeouts, int32_t *counters, void *stream);
/* reset_idx of the tasks (navigation_task.py:166-175, lidar_navigation_task.py:164-181) for the envs
 * of buf->reset_mask: target [3][N] = bounds_min + (bounds_max - bounds_min) * U(min_ratio, max_ratio),
 * target_yaw [N] (or NULL) = U(-pi, pi), robot_prev_actions = 0 if asked.  min/max_ratio: HOST float[3];
 * u [N][4] uniform draws or NULL = device generator (env, episode).                              */
int agx_nav_target_reset(const AgxEnvBuffers *buf, int num_envs, int num_actions, const float *min_ratio,
                         const float *max_ratio, const float *u, float *target, float *target_yaw,
                         int zero_prev_actions, void *stream);
/* WarpSensor.reset_idx (warp_sensor.py:153-172) for the envs of buf->reset_mask: local_pos [N][S][3] =
 * U(min_translation, max_translation), local_quat [N][S][4] = quat_from_euler(U(min_rot, max_rot))
 * (HOST float[3] each, radians); u_pos / u_rot [N][S][3] or both NULL = device generator.         */
int agx_sensor_mount_reset(const AgxEnvBuffers *buf, int num_envs, int num_sensors,
                           const float *min_translation, const float *max_translation,
                           const float *min_rot, const float *max_rot, const float *u_pos,
                           const float *u_rot, float *local_pos, float *local_quat, void *stream);

/* ---- IMU (aerial_gym/sensors/imu_sensor.py:74-153) ------------------------------------------
 * The reference reads Isaac Gym's force sensor on the base link (total force incl. gravity, body
 * frame) every physics sub-step; here the same quantity is m * (body_force / m + R^T gravity),
 * with the gravity the simulation runs under whatever gravity_compensation says: the flag only
 * decides what the sensor subtracts again (g_world).
 * agx_imu_update is called once per env step after agx_env_step with the same k: the bias random
 * walk takes k steps (z_bias [k][N][6] normal draws), noise (z_noise [N][6]) and the measurement are
 * those of the last sub-step.  z_noise == z_bias == NULL: device generator (Box-Muller on the
 * stream of (env, buf->step_counter)).  sensor_quat [N][4], bias [N][6] (in/out), imu_meas [N][6]
 * = [accel(3), gyro(3)] clamped to +-max_value.                                                 */
typedef struct AgxImuArgs {
  float bias_std[6], noise_std[6], max_value[6], max_bias_init[6];
  float min_rot[3], max_rot[3]; /* sensor mount perturbation, radians                              */
  float g_world[3];             /* gravity * (1 - gravity_compensation): what the sensor subtracts */
  float sqrt_dt, mass;
  int32_t world_frame, enable_noise, enable_bias;
  float gravity[3];             /* the simulation's gravity: what the force sensor's reading holds
                                   (g_world must be zero or equal to it: anything else is refused)  */
} AgxImuArgs;
int agx_imu_update(const AgxEnvBuffers *buf, int num_envs, int k_substeps, const AgxImuArgs *args,
                   const float *sensor_quat, const float *z_noise, const float *z_bias, float *bias,
                   float *imu_meas, void *stream);
/* IMUSensor.reset_idx for the envs of buf->reset_mask (when reset_flag[flag_parity] != 0):
 * bias = max_bias_init * (2 (u - 0.5)), sensor_quat = quat_from_euler(U(min_rot, max_rot)).
 * u_bias [N][6], u_rot [N][3] uniform draws, or both NULL = device generator (env, episode).     */
int agx_imu_reset(const AgxEnvBuffers *buf, int num_envs, const AgxImuArgs *args, const float *u_bias,
                  const float *u_rot, float *bias, float *sensor_quat, void *stream);

/* ---- reset ----------------------------------------------------------------------
 * Masked reset, in the order of EnvManager.reset_idx (env_manager.py:273-301):
 *   env bounds (IsaacGymEnv.reset_idx, IGE_env_manager.py:513-519), robot state
 *   (BaseMultirotor.reset_idx base_multirotor.py:177-205), controller gains
 *   (BaseLeeController.randomize_params base_lee_controller.py:101-118, if enabled),
 *   motor model (MotorModel.reset_idx motor_model.py:140-154), sim_steps[reset] = 0;
 * and, when *buf->reset_flag != 0, update_states for ALL envs (base_multirotor.py:205):
 * the reference refreshes every env's derived tensors whenever at least one env resets.
 * Nothing is touched when the flag is 0.
 * The uniform draws are inputs, in the AoS layout torch produces them:
 *   u_bounds_lo/hi [N][3], u_state [N][13], u_gains [N][12],
 *   u_tau_inc/u_tau_dec/u_thrust/u_kT [N][M].
 * If u_state is NULL the kernel draws them itself with a counter-based generator
 * (Philox4x32-10 keyed by `seed`, counter = (env, episode_count[env], stream, block)):
 * the sync-free mode, reproducible (the parity tests restate the generator bit for bit).
 * randomize_gains != 0 resamples the controller gains (randomize_params).
 * The reset set is buf->reset_mask.                                                   */
typedef struct AgxResetArgs {
  const float *u_bounds_lo, *u_bounds_hi;
  const float *u_state, *u_gains, *u_tau_inc, *u_tau_dec, *u_thrust, *u_kT;
  float lower_bound_min[3], lower_bound_max[3], upper_bound_min[3], upper_bound_max[3];
  float min_state[13], max_state[13];
  float gains_min[12], gains_max[12];
  float tau_inc_min, tau_inc_max, tau_dec_min, tau_dec_max, kT_min, kT_max;
  int32_t randomize_gains;
  uint64_t seed;
} AgxResetArgs;

int agx_reset_masked(const AgxRobotParams *params, const AgxEnvBuffers *buf, int num_envs,
                     const AgxResetArgs *args, void *stream);

/* The robot side of a navigation task's step as ONE launch (sync-free mode: device generator only): agx_reset_masked, then for
 * the envs that reset agx_sensor_mount_reset and agx_nav_target_reset, then agx_sensor_pose for every env -- the same device
 * functions as those four entry points, in that order (the mount and the target draws are keyed by the episode count the robot
 * reset has just advanced).  Replaces four dependent 5-us launches at the 256 .. 1024 envs an RL run uses.
 * num_sensors = 0: no sensor part; randomize_mount = 0: the mount is left alone; reset_target = 0: no target part.   */
typedef struct AgxNavRobotSideArgs {
  int32_t num_sensors, randomize_mount;
  float mount_t_min[3], mount_t_max[3], mount_r_min[3], mount_r_max[3];
  float *local_pos, *local_quat;   /* [N][S][3], [N][S][4]: the mount in the robot frame */
  float frame_quat[4];
  float *sensor_pos, *sensor_quat; /* out [N][S][3], [N][S][4]: world pose of every sensor */
  int32_t reset_target, num_actions, zero_prev_actions, pad_;
  float target_ratio_min[3], target_ratio_max[3];
  float *target;      /* [3][N] */
  float *target_yaw;  /* [N] or NULL */
} AgxNavRobotSideArgs;
int agx_nav_robot_side(const AgxRobotParams *params, const AgxEnvBuffers *buf, int num_envs, const AgxResetArgs *args,
                       const AgxNavRobotSideArgs *nav, void *stream);

/* agx_reset_masked + agx_obs_position in one launch (the position task has no sensor to
 * render between reset and observation).                                                  */
int agx_post_step_position(const AgxRobotParams *params, const AgxEnvBuffers *buf, int num_envs,
                           const AgxResetArgs *args, const float *target, float *obs, void *stream);

/* The tail of step() of the end-to-end task (position_setpoint_task_sim2real_end_to_end.py:180-190, return_state_before_reset
 * False) in one launch: the masked reset as the call of that name performs it; the task's own reset_idx (:146-153) -- when some env
 * resets, the target of EVERY env goes back to zero; the end-to-end observation (see there for `noise`) on the post-reset tensors;
 * then prev_actions <- actions (:189) and prev_pos_error <- target - robot_position (:190).                                     */
int agx_post_step_end_to_end(const AgxRobotParams *params, const AgxEnvBuffers *buf, int num_envs, const AgxResetArgs *args,
                             float *target, const float *noise, float *obs, const float *actions, float *prev_actions,
                             float *prev_pos_error, void *stream);

/* One task.step() of the position-setpoint task as a single host call.  Toggles buf->flag_parity first, exactly like the
 * host does once per env step.
 *
 * Two launches in general: agx_env_step with the position epilogue, then agx_post_step_position.  The second exists because
 * when ANY env resets, the reference refreshes the derived tensors of EVERY env (base_multirotor.py:205): each observation
 * depends on an OR over the batch.  When that OR is known before the step is issued, the step is ONE launch
 * (k_position_step_fused):
 *   AGX_STEP_ANY   some env certainly resets: step, reset of the env's own flagged envs, refresh and observation per env;
 *   AGX_STEP_NONE  no env can reset: step and the observation from the pre-step derived tensors.
 * The proof comes from a record the kernels leave in mapped host memory, read without any HIP synchronisation:
 *   - every wave stores a slot about the END of its step: a horizon mask (bit k: a "witness" env truncates in step t + k,
 *     1 <= k <= AGX_PROOF_HORIZON, and cannot crash before), max sim_steps, max |target - p|, max |v|, "some env reset";
 *   - one extra workgroup of the NEXT launch folds those slots into the record (seqlock: [0] end tag, [1] horizon,
 *     [2] max sim_steps, [3] max dist bits, [4] max speed bits, [5] flags, [7] begin tag; tag = step_counter + 1 of the
 *     launch that wrote the slots, 31 bits, 0 = none);
 *   - agx_step_proof_decide turns the record into the mode of step `now_tag`.
 * The proof is about what the KERNELS did: the caller voids older records (proof_min_tag = this step's tag) whenever it
 * touched the state, target, sim_steps or motor-thrust tensors, the episode length, or called anything else on the env.
 * Two launches, always, for: a stream that is capturing (and every later step of a plan that was captured), the strict-RNG
 * draws (reset->u_state), a bound step exchange (step_rows, step_signal, peer push), anything the four-lanes-per-env kernel
 * does not cover, agx_set_option("single_launch_step", 0), proof_* NULL.  Bit-identical in every mode.                    */
#define AGX_PROOF_HORIZON 31
#define AGX_PROOF_SLOT_WORDS 8
#define AGX_PROOF_RECORD_WORDS 8
enum { AGX_STEP_TWO = 0, AGX_STEP_ANY = 1, AGX_STEP_NONE = 2 };
/* why a step ran as it did (AgxPositionStepPlan.reason_count) */
enum {
  AGX_PROOF_PROVED = 0,       /* ANY or NONE */
  AGX_PROOF_OFF = 1,          /* option single_launch_step = 0, or no proof buffers in the plan */
  AGX_PROOF_NOT_COVERED = 2,  /* strict RNG, step exchange, kernel choice: the two launches are the only form */
  AGX_PROOF_CAPTURE = 3,      /* stream capturing now, or a step of this plan was captured before */
  AGX_PROOF_NO_RECORD = 4,    /* nothing published yet (tag 0) */
  AGX_PROOF_TORN = 5,         /* the seqlock read saw a write in progress */
  AGX_PROOF_VOID = 6,         /* the record is older than the caller's last interference */
  AGX_PROOF_TAG = 7,          /* the record is not from a step before this one, or more than 64 steps old */
  AGX_PROOF_RESET_NO_WITNESS = 8, /* some env reset in the recorded step (no "none" proof) and no witness covers this step */
  AGX_PROOF_MAY_TRUNCATE = 9, /* no witness, and an env may truncate by this step */
  AGX_PROOF_MAY_CRASH = 10,   /* no witness, and an env may crash by this step */
  AGX_PROOF_LAG = 11,         /* the host ran more than max_lag steps ahead and the record did not catch up within 2 ms */
  AGX_PROOF_REASONS = 12
};
typedef struct AgxPositionStepPlan {
  const AgxRobotParams *params;
  AgxEnvBuffers *buf;
  const AgxTaskArgs *task;
  const AgxResetArgs *reset;
  const float *target; /* [3][N] */
  float *obs;          /* [N][13] */
  int32_t num_envs;
  int32_t k_substeps;
  /* single-launch steps (all three buffers non-NULL to enable) */
  uint32_t *proof_slots;     /* device, 2 * ceil(num_envs / 16) * AGX_PROOF_SLOT_WORDS words, zero-filled */
  uint32_t *proof_record;    /* agx_host_record_alloc(AGX_PROOF_RECORD_WORDS * 4) */
  uint32_t *proof_violation; /* device, 1 word, zero-filled */
  uint32_t proof_min_tag;    /* in: records with an older tag are void */
  int32_t max_lag;           /* in: the call does not run more than this many steps ahead of the newest record (it spins on
                                the record, no HIP call, at most 2 ms); 2 .. AGX_PROOF_HORIZON - 1, 0 = 8               */
  int32_t captured;          /* out: 1 once a step of this plan was issued into a capturing stream */
  int32_t slot_run;          /* out: consecutive calls whose launches wrote proof slots */
  int32_t last_mode;         /* out: AGX_STEP_* of the last call */
  int32_t last_reason;       /* out: AGX_PROOF_* of the last call */
  uint64_t mode_count[3];    /* out: calls per AGX_STEP_* */
  uint64_t reason_count[AGX_PROOF_REASONS]; /* out: calls per AGX_PROOF_* */
  uint64_t lag_wait_ns;      /* out: time spent spinning on the record because the call was max_lag steps ahead of it */
  uint64_t lag_waits;        /* out: entries into that spin loop */
} AgxPositionStepPlan;
int agx_position_task_step(AgxPositionStepPlan *plan, const float *actions_in, void *stream);

/* The host decision of agx_position_task_step, a pure function of the record and the step (CPU tests drive it with
 * synthetic records).  Returns AGX_STEP_*; *reason = AGX_PROOF_*.                                                       */
typedef struct AgxStepProofQuery {
  uint32_t now_tag;            /* the tag THIS step's launch writes: (step_counter + 1) mod 2^31 */
  uint32_t min_tag;            /* records with an older tag are void */
  int32_t episode_len;
  int32_t reset_on_collision;
  float dt, max_linear_velocity, dv; /* dv: agx_step_proof_dv */
  int32_t reserved;
} AgxStepProofQuery;
int agx_step_proof_decide(const uint32_t *record, const AgxStepProofQuery *query, int32_t *reason);
/* the bound on the growth of |v| per env step: (num_motors max(|max_thrust|, |min_thrust|) / mass + |g|) dt 1.1 */
float agx_step_proof_dv(const AgxRobotParams *params);
/* bounds on how far a robot whose speed is `speed` gets in m env steps, margins included (dist + bound < 8 proves "no crash"):
 * per_env = 1: m dt min(v_max, speed + m dv) (the witnesses' bound); 0: the sum over the steps of min(v_max, speed + i dv) dt
 * (the "none" proof's, from the batch's largest speed)                                                                    */
float agx_step_proof_travel(int m, float speed, float dt, float max_linear_velocity, float dv, int per_env);
/* the slot's horizon bit of one env at the end of step t (1 << k if it is a witness for step t + k, else 0): the device's rule */
uint32_t agx_step_proof_witness_bit(int episode_len, int reset_on_collision, int sim_steps, float dist, float speed, float dt,
                                    float max_linear_velocity, float dv);
/* Mapped, device-visible, coherent host memory for small records that kernels write and the host polls (zero-filled). */
int agx_host_record_alloc(size_t bytes, void **out);
int agx_host_record_free(void *record);

/* ---- the same step in the reference-faithful RNG mode (args={"strict_rng": True}) -------------------------------------
 * The reference consumes torch's generator only on steps on which some env resets (`if len(env_ids) > 0` behind a
 * nonzero(): env_manager.py:364-375), with one rand_like per reset quantity (IGE_env_manager.py:513-519,
 * base_multirotor.py:177-205, motor_model.py:140-154).  Keeping that contract costs the host one bit per step.
 *
 * agx_torch_uniform_fill: the numbers `Tensor.uniform_(0, 1)` produces for `count` dense float32 tensors called one after
 * another on a device generator whose state is (seed, offset) -- torch 2.10 / ROCm 7: ATen/native/cuda/DistributionTemplates.h
 * (launch policy, thread -> element mapping, bound reversal) over rocrand's Philox4x32-10 (csrc/agx_strict.hip cites the
 * lines) -- in ONE launch.  sm_count / max_threads_per_sm: the device properties torch's launch policy reads
 * (multiProcessorCount, maxThreadsPerMultiProcessor).  *offset_after = the generator offset after those calls
 * (Generator.set_offset).  Pinned bit for bit against the real calls by tests/test_gpu_strict_fast.py.
 *
 * agx_host_word_create: one 32-bit word of mapped, coherent host memory (hipHostMalloc) that kernels store to and the host
 * polls; agx_position_task_step_strict: agx_position_task_step with, between its two launches, a one-lane kernel that
 * publishes (sequence << 1 | reset_flag[parity]) into that word, a host spin until it arrives (no stream synchronisation),
 * and -- only when the flag is set -- the uniform fill of the reset's draw tensors (plan->reset->u_*).  *drew = the flag;
 * *offset_after = the generator offset the caller must set (unchanged when nothing was drawn).                              */
#define AGX_MAX_UNIFORM_SEGMENTS 8
int agx_torch_uniform_fill(int count, float *const *out, const int64_t *numel, uint64_t seed, uint64_t offset, int sm_count,
                           int max_threads_per_sm, uint64_t *offset_after, void *stream);
int agx_host_word_create(uint32_t **word);
int agx_host_word_destroy(uint32_t *word);
typedef struct AgxStrictStepPlan {
  const AgxPositionStepPlan *plan;
  uint32_t *host_word;                       /* agx_host_word_create */
  int32_t count;                             /* draw tensors, in the reference's call order */
  int32_t timeout_ms;                        /* 0: 10 s */
  float *out[AGX_MAX_UNIFORM_SEGMENTS];
  int64_t numel[AGX_MAX_UNIFORM_SEGMENTS];
  uint64_t seed, offset;                     /* the generator's state before this step (Generator.initial_seed / get_offset) */
  int32_t sm_count, max_threads_per_sm;
} AgxStrictStepPlan;
int agx_position_task_step_strict(const AgxStrictStepPlan *plan, const float *actions_in, int *drew, uint64_t *offset_after,
                                  void *stream);

/* Obstacle pose randomisation of the reset envs: AssetManager.reset_idx
 * (asset_manager.py:51-71) incl. the half-obstacle resample of env_manager.py:283-295.
 * u1/u2 [N][K][13] and u_sel [N] are the uniform draws (first / second rand_like and the
 * bernoulli(0.15)); all NULL = device generator.  u_bounds as in AgxResetArgs (the new env
 * bounds are needed before the robot reset kernel has stored them).  Assets with index
 * >= the active count are parked at -1000 m.                                              */
int agx_reset_assets(const AgxEnvBuffers *buf, int num_envs, int num_assets,
                     const AgxResetArgs *args, const float *u1, const float *u2,
                     const float *u_sel, const float *min_ratio, const float *max_ratio,
                     int num_obstacles, int num_keep_in_env, float *asset_state, void *stream);

/* ---- scene / ray-cast -------------------------------------------------------------
 * Scene = per-env triangle soup with a fixed topology: T triangles, each owned by one
 * asset (obstacle) whose pose comes from env_asset_state_tensor.                      */

/* WarpEnv.reset_idx (warp_env_manager.py:40-54): v_world = tf_apply(q_asset, p_asset, v).
 * tri_local/tri_world: [N][T][9] (a,b,c xyz); tri_asset: [T]; asset_state: [N][K][13].
 * Only envs with mask[env] != 0 are transformed (mask NULL = all).  The env is the launch's
 * grid.x: no cap on num_envs from the grid; num_tris <= 65535 * 256 (chunks on grid.y).  */
int agx_scene_transform(int num_envs, int num_tris, int num_assets, const float *tri_local,
                        const int32_t *tri_asset, const float *asset_state, const uint8_t *mask,
                        float *tri_world, void *stream);

/* Multi-primitive assets (URDFs with several links, e.g. the reference's `trees`): prim_state [N][P][13]
 * pose = asset pose (x) local pose (local_pos [N][P][3], local_quat [N][P][4], prim_asset [N][P] = owning
 * asset index in that env), velocities copied.  prim_state then stands in for asset_state (num_assets = P) in
 * agx_scene_transform (tri_asset = primitive index) and agx_boxes_from_assets.                     */
int agx_prims_from_assets(int num_envs, int num_prims, int num_assets, const int32_t *prim_asset,
                          const float *asset_state, const float *local_pos, const float *local_quat,
                          const uint8_t *mask, float *prim_state, void *stream);

/* Kinematic obstacles: EnvManager.step(actions, env_actions) with env_actions = obstacle twists
 * (obstacle_manager.py:40-44, examples/dynamic_env_example.py:33-45).  twist [N][K][6] = world-frame
 * linear and angular velocity; asset_state [N][K][13] gets the twist in its velocity slots and its
 * pose advanced by k sub-steps of dt (same rule as the robot integrator).  Follow with
 * agx_scene_transform / agx_bvh_build / agx_boxes_from_assets (mask NULL) to move the geometry.  */
int agx_assets_integrate(int num_envs, int num_assets, float *asset_state, const float *twist,
                         float dt, int k_substeps, void *stream);

/* wp.Mesh(...) BVH build / mesh.refit() (warp_env_manager.py:162-166, 52-53).
 * A workgroup builds a binary LBVH over the T triangles of an env in LDS and stores
 * T-1 nodes of 16 floats each: [lo_l(3) child_l | hi_l(3) child_r | lo_r(3) pad | hi_r(3) pad],
 * child < 0 encodes a leaf: triangle index = ~child.
 * prims_per_object > 0: the soup is made of objects of that many consecutive triangles (boxes:
 * 12); the Morton order is then taken over object centres, which keeps an object's triangles
 * together (two-level hierarchy).  0 = order by triangle centroid.
 * mask != NULL rebuilds only the flagged envs and needs `work` (int32[num_envs + 2], scratch):
 * the dirty env ids are compacted into it and a CU-sized persistent grid pulls from the list.
 * With objects, the order of the keys is obtained from a sort of the OBJECTS' codes plus every triangle's rank inside its
 * object (the full key sort runs only when two objects that are in the env share a code); AGX_BVH_FULL_SORT ORed into
 * prims_per_object forces the full sort -- a test hook: both must give the same tree.   */
#define AGX_BVH_FULL_SORT 0x40000000
/* AGX_BVH_BOX_OBJECTS ORed into prims_per_object (= 12): every object is a box of trimesh.creation.box's topology (the
 * reference's box URDFs through urdfpy: 8 corners, the 12 faces in trimesh's order).  The builder then ends the tree at the
 * OBJECT: the subtree root whose leaves are exactly one object's 12 triangles becomes an OBJECT NODE -- its 64-byte record
 * holds the box's frame instead of two child boxes,
 *     [0..2] axis x (unit, world)  [3] half extent x     [4..6] axis y  [7] half extent y
 *     [8..10] axis z               [11] half extent z    [12..14] centre  [15] index of the object's first triangle (int bits)
 * (derived from the object's world-frame triangles: corners 0, 1, 2, 4 of the box), and the parent's child reference carries
 * AGX_BVH_OBJECT_REF.  The ray-cast kernels intersect the box's slabs in its own frame, conservatively (tolerance >> rounding),
 * and run the exact triangle test only on the face(s) a ray can enter through: the closest hit over the triangles the exact test
 * accepts -- the result's definition -- is unchanged, the five in-object nodes and most face tests are gone.  An object whose
 * triangles do not make an orthogonal box (or whose keys interleave with another object's) keeps its triangle subtree.
 * AGX_BVH_OBJECT_TREE (round 6; with AGX_BVH_BOX_OBJECTS, 2 <= T / 12 <= 256, no AGX_BVH_FULL_SORT): the tree is BUILT over the
 * K = T / 12 objects instead of over the triangles: records 0 .. K - 2 are the radix tree over the objects' Morton keys (root 0),
 * records K - 1 + 5 o .. + 4 belong to object o -- its object node at the first of them, or, for an object that is not a recognised
 * box (parked beyond the curriculum level at -1000 m, or simply not a box), a five-node subtree over its six triangle pairs with its
 * root at the fifth.  Consumers follow child references only; nothing depends on the numbering.  For scenes whose objects ARE boxes
 * (one dirty env: 24 us instead of 55-60); the quick subtrees of non-box chunks (cylinders, spheres, meshes) traverse 7-9 % slower
 * than their LBVH subtrees (profiles/forest_probe_r06.py), so callers leave the flag off for such scenes.                       */
#define AGX_BVH_BOX_OBJECTS 0x20000000
#define AGX_BVH_OBJECT_TREE 0x10000000
#define AGX_BVH_OBJECT_REF 0x40000000   /* bit 30 of a non-negative child reference: the child is an object node */
size_t agx_bvh_nodes_bytes(int num_envs, int num_tris);
int agx_bvh_build(int num_envs, int num_tris, int prims_per_object, const float *tri_world,
                  const uint8_t *mask, float *nodes, int32_t *work, void *stream);

/* Obstacle OBBs for the collision test, from the same asset poses:
 * boxes [K][11][N] <- asset_state [N][K][13], half_extents [N][K][3]; row 10 of a box is
 * its bounding radius |half_extents| * 1.000001.  num_assets <= 65535 (grid.y).         */
int agx_boxes_from_assets(int num_envs, int num_assets, const float *asset_state,
                          const float *half_extents, const uint8_t *mask, float *boxes,
                          void *stream);

/* The three calls above as ONE, for the geometry refresh behind a reset (asset_manager.py:51-71 moves the obstacles of the
 * envs that reset; env_manager.py:283-295; the reference then refits its Warp meshes: warp_env.py / `mesh.refit()`):
 * world-frame triangles, collision boxes (boxes may be NULL) and the tree of the envs flagged in `mask`.  With a mask: the
 * dirty env ids are compacted into `work` and ONE persistent launch transforms, boxes and builds per dirty env -- as three
 * launches the two small ones are a dispatch over every env each (22 + 9 us per step at 8192 envs x 106 obstacles for a few
 * dozen dirty envs).  mask == NULL: every env, through the three stand-alone kernels.  Same arithmetic either way.          */
int agx_scene_refresh(int num_envs, int num_tris, int num_assets, const float *tri_local,
                      const int32_t *tri_asset, const float *asset_state, const float *half_extents,
                      int prims_per_object, const uint8_t *mask, float *tri_world, float *boxes,
                      float *nodes, int32_t *work, void *stream);

/* Scenes above the LDS-resident build's 2944 triangles per env (the reference hands Warp whatever mesh it is given: the Warp
 * mesh build / refit behind asset_manager.py:51-71, warp_env_manager.py:40-54, 162-166): the same LBVH -- same keys, order, tree and
 * records, all prims_per_object forms; AGX_BVH_OBJECT_TREE and AGX_BVH_FULL_SORT are accepted and change nothing -- built with its
 * working arrays in `scratch`, a caller-provided buffer in GLOBAL memory, for 2 <= num_tris <= 65536.  One workgroup builds one
 * env, a persistent grid of at most 256 workgroups owns one slab of the scratch each: agx_bvh_large_scratch_bytes(num_envs,
 * num_tris) = slabs x bytes per slab (about 40 B per triangle at the most) stops growing with num_envs at 256 envs and stays below 1 GiB.
 * It returns 0 for sizes the build refuses.  mask / work as for agx_bvh_build.  At the cap a radix tree over the unique keys
 * (32 bits of code with the parked marker, 16 of index) is at most 48 levels deep, below the ray-cast's 64-entry stack.
 * agx_scene_refresh_large: agx_scene_refresh's arguments plus the scratch -- transform, collision boxes and this build for the
 * envs of `mask`, or for every env.  All refuse by message before anything is launched: num_tris outside [2, 65536], null buffers,
 * a mask without `work`, a scratch buffer smaller than required.  agx_bvh_build, agx_scene_refresh and agx_scene_reset_refresh
 * keep their 2944 limit.                                                                                                        */
size_t agx_bvh_large_scratch_bytes(int num_envs, int num_tris);
int agx_bvh_build_large(int num_envs, int num_tris, int prims_per_object, const float *tri_world,
                        const uint8_t *mask, float *nodes, int32_t *work, void *scratch, size_t scratch_bytes,
                        void *stream);
int agx_scene_refresh_large(int num_envs, int num_tris, int num_assets, const float *tri_local,
                            const int32_t *tri_asset, const float *asset_state, const float *half_extents,
                            int prims_per_object, const uint8_t *mask, float *tri_world, float *boxes,
                            float *nodes, int32_t *work, void *scratch, size_t scratch_bytes, void *stream);

/* AssetManager.reset_idx AND the geometry refresh behind it for the envs of buf->reset_mask (agx_reset_assets + agx_scene_refresh,
 * asset_manager.py:51-71 -> warp_env_manager.py:40-54), draws from the device generator (args->u_* NULL).  Up to 2048 envs this is
 * ONE launch -- a workgroup per env that resets the env's obstacle poses, moves its triangles and collision boxes and rebuilds its
 * tree; a clean env's workgroup leaves at once, a step without a reset costs one dispatch -- above, the three launches it replaces
 * at small batches (asset reset, mask compaction, persistent refresh).  num_assets = obstacles per env (one rigid piece each:
 * multi-primitive scenes keep agx_reset_assets + agx_prims_from_assets + agx_scene_refresh).  Same device functions either way,
 * and either way a step whose flag word buf->reset_flag[buf->flag_parity] is 0 changes nothing, whatever reset_mask holds.     */
int agx_scene_reset_refresh(const AgxEnvBuffers *buf, int num_envs, int num_tris, int num_assets, const AgxResetArgs *args,
                            const float *min_ratio, const float *max_ratio, int num_obstacles, int num_keep, float *asset_state,
                            const float *tri_local, const int32_t *tri_asset, const float *half_extents, int prims_per_object,
                            float *tri_world, float *boxes, float *nodes, int32_t *work, void *stream);

/* WarpSensor.update pose composition (warp_sensor.py:177-187).
 * local_pos [N][S][3], local_quat [N][S][4], frame_quat [4] -> pos [N][S][3], quat [N][S][4] */
int agx_sensor_pose(const AgxEnvBuffers *buf, int num_envs, int num_sensors,
                    const float *local_pos, const float *local_quat, const float *frame_quat,
                    float *pos, float *quat, void *stream);

enum {
  AGX_RAY_RANGE = 0, AGX_RAY_DEPTH = 1, AGX_RAY_POINTCLOUD = 2, AGX_RAY_POINTCLOUD_WORLD = 3,
  /* draw_optimized_kernel_normal_faceID (warp_camera_kernels.py:70-121, warp_lidar_kernels.py:90-126):
   * pixels [..][3] = geometric normal of the hit face in the sensor / world frame (0 on a miss),
   * seg = face index (-1 on a miss; tri_seg is not read)                                          */
  AGX_RAY_NORMAL = 4, AGX_RAY_NORMAL_WORLD = 5
};

/* WarpSensor.apply_range_limits + normalize_observation (warp_sensor.py:216-247) as the epilogue of the
 * ray-cast itself.  With `limits` != NULL (scalar images only: modes RANGE / DEPTH) a pixel is stored
 * already limited and normalised -- bit for bit what agx_sensor_postprocess(count, pixels, NULL, NULL,
 * ...) leaves -- and the image needs no second pass over HBM.  NULL = raw distances (and the only
 * choice with sensor noise, which the reference applies BEFORE the limits).                          */
typedef struct AgxRangeLimits {
  float min_range, max_range;
  float far_oor, near_oor; /* cfg.far_out_of_range_value, cfg.near_out_of_range_value */
  int32_t normalize;       /* cfg.normalize_range: p / max_range                     */
} AgxRangeLimits;

/* DepthCameraWarpKernels.draw_optimized_kernel_{depth_range,depth_range_segmentation,
 * pointcloud,pointcloud_segmentation} (warp_camera_kernels.py:176-282, 13-66, 125-172).
 * kinv = {K_inv[0][0], K_inv[0][2], K_inv[1][1], K_inv[1][2]} (warp_cam.py:31-64).
 * pixels [N][S][H][W] (or x3), seg [N][S][H][W] int32 or NULL; tri_seg [N][T] int32.    */
int agx_raycast_camera(int num_envs, int num_sensors, int width, int height, const float *kinv,
                       float far_plane, int c_x, int c_y, int mode, const float *cam_pos,
                       const float *cam_quat, const float *tri_world, const int32_t *tri_seg,
                       const float *nodes, int num_tris, float *pixels, int32_t *seg,
                       const AgxRangeLimits *limits, void *stream);

/* StereoCameraWarpKernels.* (warp_stereo_camera_kernels.py:13-299): as agx_raycast_camera
 * (modes 0..3), but a pixel is valid only if the stereo partner at cam_pos + R(cam_quat)
 * (-baseline, 0, 0) also sees the hit point (second, any-hit ray from 0.999 t).  Occluded:
 * -1 / seg -2; a missed ray whose far-plane point the partner sees: 1000, else -1.            */
int agx_raycast_stereo_camera(int num_envs, int num_sensors, int width, int height,
                              const float *kinv, float far_plane, float baseline, int c_x, int c_y,
                              int mode, const float *cam_pos, const float *cam_quat,
                              const float *tri_world, const int32_t *tri_seg, const float *nodes,
                              int num_tris, float *pixels, int32_t *seg,
                              const AgxRangeLimits *limits, void *stream);

/* LidarWarpKernels.draw_optimized_kernel_{range,range_segmentation,pointcloud,
 * pointcloud_segmentation} (warp_lidar_kernels.py:167-194,130-163,13-86).
 * ray_vectors [H][W][3] (warp_lidar.py:40-64).                                          */
int agx_raycast_lidar(int num_envs, int num_sensors, int width, int height,
                      const float *ray_vectors, float far_plane, int mode, const float *pos,
                      const float *quat, const float *tri_world, const int32_t *tri_seg,
                      const float *nodes, int num_tris, float *pixels, int32_t *seg,
                      const AgxRangeLimits *limits, void *stream);

/* Which kernel instance the three entry points above launch for these sizes, as "<kernel name incl. template arguments>_<grid
 * size in threads>" (e.g. "k_raycast<false,0>_6291456"): the key under which profilers list it (like agx_env_step_kernel).
 * variant: 0 depth / range / point cloud, 1 normal + face id, 2 stereo.                                                  */
int agx_raycast_kernel(int num_envs, int num_sensors, int width, int height, int lidar, int variant, char *out, int out_len);

/* WarpSensor.apply_noise / apply_range_limits / normalize_observation
 * (warp_sensor.py:202-247), scalar images, in place.  z_normal/u_dropout optional.     */
int agx_sensor_postprocess(size_t count, float *pixels, const float *z_normal,
                           const float *u_dropout, float std_a, float std_b, float std_c,
                           float mean_offset, float dropout_prob, float min_range,
                           float max_range, float far_oor, float near_oor, int normalize,
                           void *stream);

/* Point-cloud branch of the same three functions: pixels [count][3]; noise / dropout act on
 * every component, the range limits on the point's norm (all three components replaced).
 * limits = 0 for world-frame clouds, which the reference neither limits nor normalises.     */
int agx_sensor_postprocess_points(size_t count, float *pixels, const float *z_normal,
                                  const float *u_dropout, float std_a, float std_b, float std_c,
                                  float mean_offset, float dropout_prob, float min_range,
                                  float max_range, float far_oor, float near_oor, int limits,
                                  int normalize, void *stream);

/* NavigationTask.post_image_reward_addition's min over the image
 * (navigation_task.py:351-357): min_pixel[N] = min(10*img, with img<0 -> 10).          */
int agx_image_min(int num_envs, int pixels_per_env, const float *pixels, float *min_pixel,
                  void *stream);

/* ---- sharded stepping: the per-step observation exchange -----------------------
 * One RCCL all-gather per env step of the [N_local][obs_dim + 3] fp32 rows the observation kernels
 * write (AgxEnvBuffers.step_rows), enqueued by a worker thread of this library on its own stream so
 * that the gather of step t overlaps the kernels of step t+1 and costs the stepping thread one
 * event record + one stream wait.  The reference has no distributed path (replicas only), so this
 * replaces nothing upstream; the host mirror is sharding.StepGather.
 *   rccl_path: the librccl.so to bind at run time (the one torch loaded); NULL = "librccl.so".
 *   agx_exchange_unique_id: rank 0 only; the 128 id bytes travel to the other ranks out of band
 *                           (torch.distributed broadcast in the host mirror).
 *   agx_exchange_create:    collective over all ranks (ncclCommInitRank), `device` = HIP ordinal.
 *   agx_exchange_post:      rows `send` [count] of this step (written on `stream`) -> `recv`
 *                           [world * count]; returns at once.  One post per parity in flight.
 *                           signal = AgxEnvBuffers.step_signal of the env whose kernels write `send`
 *                           and seq = its step_counter + 1 for this step: the gather waits for
 *                           signal[parity] >= seq on the device (no HIP call on this thread);
 *                           signal = NULL: an event recorded on `stream` now orders the gather.
 *   agx_exchange_probe:     must return 1 before a post with signal != NULL: checks (and arranges) that
 *                           the communication stream does not share a hardware queue with `stream`,
 *                           where a device-side wait would block its own producer; 0 = use events.
 *   agx_exchange_wait:      `stream` waits (no host block beyond the enqueue hand-off) for the
 *                           latest posted gather of `parity`: after it the stream may read that
 *                           recv buffer and overwrite that send buffer.
 *   agx_exchange_step:      post(parity) then wait(wait_parity) in one call (wait_parity < 0: none).
 *   agx_exchange_info:      rank and size AS THE COMMUNICATOR REPORTS THEM (ncclCommUserRank / ncclCommCount):
 *                           lets the caller assert that the collective really spans the ranks it was built for. */
typedef struct AgxExchange AgxExchange;
int agx_exchange_unique_id(const char *rccl_path, void *id_out, int id_bytes);
int agx_exchange_create(const char *rccl_path, const void *id, int id_bytes, int rank, int world,
                        int device, AgxExchange **out);
int agx_exchange_post(AgxExchange *x, int parity, const float *send, float *recv,
                      size_t count_per_rank, const uint32_t *signal, uint32_t seq, void *stream);
int agx_exchange_probe(AgxExchange *x, void *stream);
int agx_exchange_wait(AgxExchange *x, int parity, void *stream);
int agx_exchange_step(AgxExchange *x, int parity, const float *send, float *recv,
                      size_t count_per_rank, const uint32_t *signal, uint32_t seq, int wait_parity,
                      void *stream);
int agx_exchange_info(AgxExchange *x, int *rank, int *world);
int agx_exchange_destroy(AgxExchange *x);

/* Peer push (round 3): the same exchange WITHOUT a collective kernel per step.  Every rank stores its rows straight into
 * every peer's receive buffer (peer memory mapped through hipIpcMemHandle: one xGMI link per destination) and raises a
 * per-sender arrival flag there; the consumer's stream waits on its own flags.  post / wait / step / probe / info / destroy
 * are the entry points above (post ignores `recv`: the receive buffer belongs to the exchange; wait launches a one-wave flag
 * wait on `stream` instead of a cross-queue event wait).
 *   agx_exchange_create_push:  allocates this rank's receive buffer [slots][world][count_per_rank] and flags; not collective.
 *   agx_exchange_push_export:  2 x 64 bytes (hipIpcMemHandle of buffer and flags) for the peers; the host mirror all-gathers
 *                              them through torch.distributed.
 *   agx_exchange_push_connect: maps the peers' buffers (world x 128 bytes, rank-major); after it posts are allowed.
 *   agx_exchange_push_buffer:  this rank's receive buffer and slot count: the rows gathered by the s-th post (s = 1, 2, ...)
 *                              lie in slot (s - 1) % slots once agx_exchange_wait for that post's parity has passed.       */
int agx_exchange_create_push(int rank, int world, int device, size_t count_per_rank, AgxExchange **out);
int agx_exchange_push_export(AgxExchange *x, void *handles_out, int bytes);
int agx_exchange_push_connect(AgxExchange *x, const void *all_handles, int bytes);
int agx_exchange_push_buffer(AgxExchange *x, void **recv, int *slots, int *flags_uncached);
/* Rows pushed by the observation kernels THEMSELVES (AgxEnvBuffers.push_*: no launch and no host call per step for the
 * exchange): agx_exchange_push_peers hands out the addresses, in this process, of every rank's receive buffer and flag array
 * ([world] each, own included) and the device-visible time-out word; agx_exchange_push_wait_seq makes `stream` wait until
 * the rows with sequence number `seq` of every rank have arrived here.                                                   */
/* Peer push by the kernels: a new env step -- next sequence number, its slot (step_rows), the step (two back) to wait for.
 * agx_position_task_step calls it itself; callers of agx_env_step call it once per env step before the launch.           */
int agx_push_advance(AgxEnvBuffers *buf);
int agx_exchange_push_peers(AgxExchange *x, void **recv_out, void **flags_out, void **timed_out);
int agx_exchange_push_wait_seq(AgxExchange *x, uint32_t seq, void *stream);
/* Has anything gone wrong so far (worker thread; a bounded device-side wait that gave up)?  Two host reads.            */
int agx_exchange_check(AgxExchange *x);
/* Connection self-test of the peer push; every rank calls it after agx_exchange_push_connect and before the first post (the
 * callers put a barrier of their own behind it).  Each rank stores one word into every rank's receive buffer through the
 * mapped addresses -- the way the observation kernels store rows --, raises a flag, waits at most timeout_ms for every rank's
 * flag and compares what arrived.  *passed = 1: this rank received every rank's word.  The buffers are left as found. */
int agx_exchange_push_selftest(AgxExchange *x, int timeout_ms, int *passed, void *stream);

/* ---- VAE depth-image encoder (aerial_gym/utils/vae/VAE.py ImgEncoder + the sampling of VAE.encode,
 * vae_image_encoder.py:35-55) -----------------------------------------------------------------------------------------
 * Nine convolutions, two dense layers and the reparametrisation, all fp32 on the exact-fp32 matrix instruction
 * (v_mfma_f32_32x32x2_f32): every output element is ONE k-ordered fmaf chain over k = (ci, kh, kw) ascending from 0, then
 * + bias, then (optionally) + a second tensor, then (optionally) ELU with alpha 1 -- each a rounded fp32 operation.  The
 * order does not depend on batch size, env index, tile position or chunking.  DESIGN.md "VAE encoder".
 *
 * Weights reach the kernels repacked [K8][Cout] (k-major, K8 = K rounded up to a multiple of 8, the tail zero), K = Cin kh kw
 * in torch's [Cout][Cin][kh][kw] order.  Pack and unpack are host functions on host memory.                              */
enum { AGX_VAE_ELU = 1 };            /* flags of the single-layer entry points */
enum { AGX_VAE_LAYERS = 11 };        /* conv0, conv0_1, conv1_0, conv1_1, conv0_jump_2, conv2_0, conv2_1, conv1_jump_3, conv3_0,
                                        dense0, dense1: the order of every per-layer array below */
typedef struct AgxVaeConv {
  int32_t cin, cout;                 /* cout: a multiple of 32 */
  int32_t kh, kw, stride;
  int32_t pad_h, pad_w;
  int32_t in_h, in_w;                /* the (zero-padded) input the taps index: the index tables' lengths when they are given */
  int32_t out_h, out_w;              /* (in + 2 pad - k) / stride + 1 */
  int32_t src_h, src_w;              /* rows and columns of x in memory: in_h, in_w unless index tables are given */
} AgxVaeConv;
size_t agx_vae_packed_floats(int cout, int k);
int agx_vae_pack_weight(int cout, int k, const float *w /*[cout][k]*/, float *packed);
int agx_vae_unpack_weight(int cout, int k, const float *packed, float *w);
/* y [B][cout][out_h][out_w] <- conv(x [B][cin][src_h][src_w]) + bias [cout] (+ add, shaped like y) (ELU).  row_map [in_h],
 * col_map [in_w] (int32, device; both or neither): the input is x gathered as x[b][ci][row_map[r]][col_map[c]] -- a
 * nearest-neighbour resize that costs no pass of its own.  Everything is a DEVICE pointer but `shape`.                   */
int agx_vae_conv2d(int batch, const float *x, const float *w_packed, const float *bias, const float *add, float *y,
                   const AgxVaeConv *shape, int flags, const int32_t *row_map, const int32_t *col_map, void *stream);
/* y [B][out_features] <- x [B][in_features] W^T + bias (ELU): the convolution kernel at 1 x 1 spatial size.              */
int agx_vae_linear(int batch, const float *x, const float *w_packed, const float *bias, float *y, int in_features,
                   int out_features, int flags, void *stream);
/* out_hw [AGX_VAE_LAYERS][2]: output height and width of every layer for an image_h x image_w input (dense: 1 x 1).
 * AGX_E_ARG unless the last convolution ends in 3 x 6 (x 128 = the 2304 inputs of dense0).  Host only.                    */
int agx_vae_geometry(int image_h, int image_w, int32_t *out_hw);
/* The reparametrisation (VAE.py:236-244) of z [N][128]: mean = z[:64], std = exp(0.5f * z[64:]) (exp_cw), latents = mean +
 * eps * std -- each operation rounded.  eps [N][64], or NULL = the device generator: 64 standard normals per env, a function
 * of (rng_seed, env_index_base + env, env_step) alone.  means, std: optional.                                             */
int agx_vae_sample(int num_envs, const float *z, const float *eps, float *latents, float *means, float *std,
                   uint64_t rng_seed, int env_index_base, int env_step, void *stream);
/* Diagnostic: noise_out [N][64] <- the normals the NULL-eps form draws.                                                   */
int agx_vae_noise(int num_envs, uint64_t rng_seed, int env_index_base, int env_step, float *noise_out, void *stream);
/* obs [N][obs_dim], columns obs_offset .. obs_offset + 63 <- latents [N][64]                                              */
int agx_vae_place_latents(int num_envs, const float *latents, float *obs, int obs_dim, int obs_offset, void *stream);

/* The whole encoder.  Create: weights / biases = AGX_VAE_LAYERS HOST pointers each, torch's layouts ([Cout][Cin][kh][kw],
 * [out][in]); the handle owns the repacked device copies (the only entry points of this section that allocate and
 * synchronise).  AGX_E_ARG: latent_dims != 64, or an image_res agx_vae_geometry refuses.
 * agx_vae_encode: pixels [N][src_h][src_w] -> latents / means / std [N][64] (means, std optional), in chunks of as many envs
 * as `workspace` holds (agx_vae_workspace_bytes(handle, 1) at least); no allocation, no host synchronisation, no host
 * randomness.  row_map / col_map as agx_vae_conv2d (NULL: src_h x src_w must be image_res).  It issues exactly the
 * single-layer calls above, so its result equals theirs bit for bit, whatever the chunking.                               */
typedef struct AgxVaeEncoder AgxVaeEncoder;
int agx_vae_create(const float *const *weights, const float *const *biases, int image_h, int image_w, int latent_dims,
                   AgxVaeEncoder **out);
int agx_vae_destroy(AgxVaeEncoder *enc);
size_t agx_vae_workspace_bytes(const AgxVaeEncoder *enc, int envs_per_chunk);
/* The chunk size agx_vae_encode derives: as many envs as workspace_bytes holds, at most num_envs (0: not even one).  The
 * workspace size is linear in the chunk, so agx_vae_workspace_bytes of n gives back exactly n.                              */
int agx_vae_envs_per_chunk(const AgxVaeEncoder *enc, size_t workspace_bytes, int num_envs);
int agx_vae_encode(AgxVaeEncoder *enc, int num_envs, const float *pixels, int src_h, int src_w, const int32_t *row_map,
                   const int32_t *col_map, const float *eps, float *latents, float *means, float *std, void *workspace,
                   size_t workspace_bytes, uint64_t rng_seed, int env_index_base, int env_step, void *stream);
/* Diagnostic: the device copies of layer `layer` (packed weights, bias) and the buffer of its output inside a workspace
 * laid out for `envs_per_chunk` envs (byte offset).  On a bf16 handle *w_packed is the bf16 copy ([Cout][Kp] uint16_t behind
 * the float pointer) and the offsets are those of the bf16 workspace; the bias is fp32 in both.                           */
int agx_vae_layer_info(const AgxVaeEncoder *enc, int layer, int envs_per_chunk, const float **w_packed, const float **bias,
                       size_t *out_offset_bytes);

/* ---- the bf16 path of the encoder (csrc/agx_vae_bf16.hip), opt-in; everything above is unchanged by it -------------------
 * Arithmetic: weights rounded ONCE to bf16 (nearest even) when packed, the depth image rounded to bf16 as conv0 reads it,
 * biases fp32.  Products are exact and accumulate in fp32 inside v_mfma_f32_32x32x16_bf16, all of K in one chain per output
 * element (no split-K) in the k order of the packing: the result of an element does not depend on batch size, env index,
 * tile, channel-tile count or chunking (the order INSIDE one instruction is the hardware's).  Epilogue in fp32: + bias, then
 * (optionally) + the second tensor (stored bf16, widened), then (optionally) ELU (expm1_cw), then ONE round to nearest even
 * for the bf16 store.
 * Layout: activations [B][H][W][C] bf16; weights [Cout][Kp] bf16 with k = (kh, kw, ci), ci fastest, Kp = K rounded up to 16,
 * the tail zero.  A dense layer that reads a flattened [H][W][C] activation is packed with the AgxVaeConv of that
 * activation (cin = C, kh = H, kw = W): its torch columns (c, h, w) land in (h, w, c) order.
 * A tap outside the image and a pixel past the batch are never addressed.                                                  */
enum { AGX_VAE_FP32 = 0, AGX_VAE_BF16 = 1 };           /* encoder precision */
enum { AGX_VAE_OUT_F32 = 2, AGX_VAE_IN_IMAGE_F32 = 4 }; /* flags of the bf16 entries, beside AGX_VAE_ELU: y is fp32 [B][H][W][C];
                                                           x is the fp32 planar image [B][src_h][src_w] (cin == 1 only) */
/* Host functions on host memory; only cin, cout, kh, kw of `shape` are read.  w / the unpacked result: torch's
 * [cout][cin][kh][kw] fp32 (unpack returns the ROUNDED values); packed: agx_vae_packed_bf16_elems(shape) uint16_t.       */
size_t agx_vae_packed_bf16_elems(const AgxVaeConv *shape);
int agx_vae_pack_weight_bf16(const AgxVaeConv *shape, const float *w, uint16_t *packed);
int agx_vae_unpack_weight_bf16(const AgxVaeConv *shape, const uint16_t *packed, float *w);
/* y [B][out_h][out_w][cout] (bf16, or fp32 with AGX_VAE_OUT_F32) <- conv(x [B][src_h][src_w][cin] bf16) + bias [cout] fp32
 * (+ add, bf16 [B][out_h][out_w][cout]) (ELU).  With AGX_VAE_IN_IMAGE_F32 x is the fp32 image and row_map / col_map act as
 * in agx_vae_conv2d.  AGX_E_ARG before any device call: a null buffer, cout % 32, cin % 8 without the image flag, the image
 * flag with cin != 1, index tables without the image flag, x / w_packed / add / y not 16-byte aligned, unknown flag bits.  */
int agx_vae_conv2d_bf16(int batch, const void *x, const uint16_t *w_packed, const float *bias, const uint16_t *add, void *y,
                        const AgxVaeConv *shape, int flags, const int32_t *row_map, const int32_t *col_map, void *stream);
/* y [B][out_features] <- x [B][in_features] (bf16) W^T + bias (ELU): the same kernel at 1 x 1 spatial size
 * (in_features % 8 == 0, out_features % 32 == 0; flags: AGX_VAE_ELU, AGX_VAE_OUT_F32).                                     */
int agx_vae_linear_bf16(int batch, const uint16_t *x, const uint16_t *w_packed, const float *bias, void *y, int in_features,
                        int out_features, int flags, void *stream);
/* agx_vae_create with a precision (AGX_VAE_FP32: exactly agx_vae_create).  On a AGX_VAE_BF16 handle agx_vae_workspace_bytes,
 * agx_vae_envs_per_chunk and agx_vae_encode follow the precision: every layer's buffer is bf16 but dense1's (fp32, what
 * agx_vae_sample reads), the workspace is still linear in the chunk, and agx_vae_encode issues exactly the single-layer
 * bf16 calls above (conv0 with AGX_VAE_IN_IMAGE_F32, dense1 with AGX_VAE_OUT_F32).                                         */
int agx_vae_create_precision(const float *const *weights, const float *const *biases, int image_h, int image_w,
                             int latent_dims, int precision, AgxVaeEncoder **out);
int agx_vae_precision(const AgxVaeEncoder *enc);       /* AGX_VAE_FP32 / AGX_VAE_BF16; -1 for NULL */

/* ---- snapshot / restore / fork of the simulator state (csrc/agx_snapshot.hip) ---------------------------------------------
 * The state of a running simulation is spread over many tensors (AgxEnvBuffers, obstacle poses, sensor images and mounts,
 * IMU bias walks, per-task tensors).  A table names them once; ONE launch packs them into a block of 32-bit words, ONE
 * launch puts a block back -- whole, for the envs of a mask, or with every env taking the row of another env (fork).
 *
 * The block is [block_rows][num_envs] words; an entry of `rows` rows owns the rows * num_envs words from word
 * block_row * num_envs on, in the order its live tensor has them:
 *   AGX_SNAP_SOA     live [rows][N]: word r * N + env.  Lanes run along the env axis on both sides.
 *   AGX_SNAP_AOS     live [N][rows] (images, obstacle poses): word env * rows + r.  Lanes run along the env's own words,
 *                    which are contiguous on both sides (lanes along the env axis would stride the live side by `rows`).
 *   AGX_SNAP_GLOBAL  live [rows], not per env (reset_flag, curriculum counters): the entry's first `rows` words; the rest of
 *                    its rows is unused.  Written back only when every env is (mask NULL).              
 * elem_size 4: words are copied as they are (float / int32, bits).  elem_size 1 (bool / uint8): a byte is widened to a
 * word in the block and narrowed on the way back.  Without mask and src_index, entries whose live pointer is 16-byte
 * aligned move 16 bytes per lane (the block side is aligned whenever num_envs % 4 == 0).                                   */
#define AGX_SNAPSHOT_MAX_ENTRIES 96
enum { AGX_SNAP_SOA = 0, AGX_SNAP_AOS = 1, AGX_SNAP_GLOBAL = 2 };
typedef struct {
  void *ptr;          /* device, live tensor                                                                               */
  int32_t rows;       /* > 0; rows * num_envs < 2^31                                                                        */
  int32_t block_row;  /* first row of this entry in the block: the sum of `rows` of the entries before it                   */
  int32_t elem_size;  /* 1 or 4 bytes                                                                                       */
  int32_t layout;     /* AGX_SNAP_*                                                                                         */
} AgxSnapshotEntry;
typedef struct {
  int32_t count;        /* entries in use, 1 .. AGX_SNAPSHOT_MAX_ENTRIES                                                    */
  int32_t block_rows;   /* sum of rows                                                                                      */
  uint32_t *error;      /* device [1], zero: set to 1 by a scatter that met an out-of-range src_index entry                 */
  AgxSnapshotEntry entry[AGX_SNAPSHOT_MAX_ENTRIES];
} AgxSnapshotTable;
/* block <- live tensors.  One launch, no host synchronisation.                                                             */
int agx_state_gather(const AgxSnapshotTable *table, int num_envs, void *block, void *stream);
/* live[row][env] <- block[row][src_index[env]] where mask[env] != 0.  src_index (int32 [N], device; NULL: identity), mask
 * (uint8 [N], device; NULL: every env).  One launch.  Every wave range-checks ALL of src_index before it stores anything:
 * with an entry outside [0, N) nothing is written, nothing is read out of bounds and table->error becomes 1.  With
 * src_index the call then waits for the stream, reads the word, clears it and returns AGX_E_ARG when it was set (a fork is
 * a planner's branch point, not a per-step call); without src_index it does not synchronise.  Cost of the check: every wave
 * of the launch reads all N indices (N / 64 loads per wave, served from L2 after the first); with large AoS entries (images)
 * at thousands of envs that is millions of redundant loads per fork.  Not measured.                                        */
int agx_state_scatter(const AgxSnapshotTable *table, int num_envs, const void *block, const int32_t *src_index,
                      const uint8_t *mask, void *stream);

/* ---- policy actor: a trained MLP in the loop as one launch (csrc/agx_policy.hip) -------------------------------------------
 * Replaces the torch module of examples/rl_games_example/rl_games_inference.py:7-48 (MLP: Linear / ELU x 3, Linear) and, for
 * input normalisation, sampling and clamping, what rl_games' player does around it (players.py PpoPlayerContinuous.get_action:
 * running_mean_std, mu + sigma * randn, clamp to [-1, 1]; common/player.py BasePlayer).  DESIGN.md "Policy actor".
 *
 * Numerics: every layer output is ONE fmaf chain over k = 0, 1, 2, ... starting from 0 (v_mfma_f32_32x32x2_f32), then + bias,
 * then the activation -- each a rounded fp32 operation: the bits of agx_vae_linear applied layer by layer.  The result does not
 * depend on the batch size, the env's position in the batch or how the waves split the channels.
 *
 * Limits: 1 .. AGX_POLICY_MAX_LAYERS layers; input width 1 .. AGX_POLICY_MAX_WIDTH; hidden widths multiples of 32 up to
 * AGX_POLICY_MAX_WIDTH; output width 1 .. AGX_POLICY_MAX_WIDTH; the activations of 32 envs of any two consecutive layers fit the
 * 160 KiB of LDS of a workgroup.  Outside them: AGX_E_ARG, the message names the offending number.                          */
#define AGX_POLICY_MAX_LAYERS 8
#define AGX_POLICY_MAX_WIDTH 512
enum { AGX_POLICY_NONE = 0, AGX_POLICY_ELU = 1 /* alpha 1, expm1_cw on the negative side */, AGX_POLICY_RELU = 2 };
enum { AGX_POLICY_SAMPLE = 1, AGX_POLICY_CLAMP = 2, AGX_POLICY_RESET_AFTER = 4 /* agx_recurrent_act only */ };  /* flags of the act calls */
typedef struct AgxPolicy AgxPolicy;
/* Host only: the limits above for dims [num_layers + 1] (what the create call checks first); lds_bytes (optional) receives the
 * dynamic LDS of the launch.                                                                                                */
int agx_policy_check(int num_layers, const int32_t *dims, size_t *lds_bytes);
/* weights / biases: num_layers HOST pointers each, torch's [out][in] and [out].  hidden_activation: AGX_POLICY_NONE / _ELU /
 * _RELU after every layer but the last (mu_activation None in both rl_games recipes).  The handle owns the repacked device
 * copies ([K8][Cout] as the VAE's, the last layer padded to a multiple of 32 zero rows the caller never sees) and the buffers
 * the two setters fill.  Create, the setters and destroy are the set-up calls: they copy from host memory and wait for the
 * copy; only create and destroy allocate and free.                                                                          */
int agx_policy_create(int num_layers, const int32_t *dims, const float *const *weights, const float *const *biases,
                      int hidden_activation, AgxPolicy **out);
/* rl_games' normalize_input (running_mean_std.py RunningMeanStd.forward): before layer 0 the kernel computes
 * clamp((x - mean) / denom, -clip, clip) with IEEE subtraction and division.  mean, denom: HOST [in]; the caller computes
 * denom = sqrt(var + 1e-5) in float32.  Both NULL: switched off again.                                                        */
int agx_policy_set_input_norm(AgxPolicy *p, const float *mean, const float *denom, float clip);
/* logstd: HOST [out], the per-action `sigma` parameter of the checkpoint (fixed_sigma).  NULL: none.                         */
int agx_policy_set_logstd(AgxPolicy *p, const float *logstd);
/* obs [N][in] -> actions [N][out] (device): one launch, no allocation, no host synchronisation, no host randomness.
 * mu_out (optional, [N][out]): the mean before sampling and clamping.  AGX_POLICY_SAMPLE: sigma = exp_cw(logstd), t = eps *
 * sigma, a = mu + t, each rounded; eps [N][out], or NULL = the device generator: standard normals that are a function of
 * (rng_seed, env_index_base + env, env_step, action index) alone (RNG_POLICY_EPS).  AGX_POLICY_CLAMP: clip to [-1, 1], last.
 * num_envs = 0 does nothing.                                                                                                */
int agx_policy_act(AgxPolicy *p, int num_envs, const float *obs, float *actions, float *mu_out, const float *eps, int flags,
                   uint64_t rng_seed, int env_index_base, int env_step, void *stream);
/* Diagnostic: noise_out [N][out] <- the normals the NULL-eps form draws.                                                     */
int agx_policy_noise(const AgxPolicy *p, int num_envs, uint64_t rng_seed, int env_index_base, int env_step, float *noise_out,
                     void *stream);
int agx_policy_destroy(AgxPolicy *p);

/* ---- recurrent actor: encoder MLP -> GRU cell -> linear head as one launch (csrc/agx_policy.hip k_recurrent_act) -------------
 * Replaces sample-factory's actor with a recurrent core as the reference runs it in
 * examples/dce_rl_navigation/sf_inference_class.py:80-101 and sim2real/nn_inference_class.py:77-101 (normalize_obs, forward_head,
 * forward_core, forward_tail, then rnn_states kept between calls).  DESIGN.md 3.8.
 *
 * The net: observation normaliser (optional); an encoder of L linear layers with the hidden activation after EVERY layer, the
 * last included (sample-factory's create_mlp); one torch.nn.GRU cell, gate order r, z, n; one linear head of P outputs: P = 2 A
 * when adaptive_stddev (means, then log-std), P = A with a constant log-std vector (agx_recurrent_set_logstd).
 *
 * Numerics: every linear map has the bits of agx_vae_linear (see the policy actor above); the cell per env and channel j < H,
 * each line one rounded fp32 operation:  r = sigmoid_cw(gi_r + gh_r);  z = sigmoid_cw(gi_z + gh_z);  n = tanh_cw(gi_n + r * gh_n);
 * a = 1 - z;  b = a * n;  c = z * h;  h' = b + c.  Independent of the batch size, the env's place and other envs' flags.
 *
 * Limits: 1 .. AGX_POLICY_MAX_LAYERS - 2 encoder layers; widths as for agx_policy_create (dims[1 .. L] multiples of 32; dims[L] is
 * the cell's input size); hidden a multiple of 32 within 32 .. AGX_POLICY_MAX_WIDTH; 1 .. 64 actions; the live LDS buffers of 32
 * envs (the encoder's ping-pong pair, h, gi, gh: (w0 + w1 + 7 hidden) x 128 bytes) within 160 KiB.  Outside them: AGX_E_ARG, the
 * message names the offending number.                                                                                      */
typedef struct AgxRecurrent AgxRecurrent;
/* Host only: the limits above for the encoder widths dims [num_encoder_layers + 1], the hidden size and the head's P;
 * lds_bytes (optional) receives the dynamic LDS of the launch.                                                              */
int agx_recurrent_check(int num_encoder_layers, const int32_t *dims, int hidden, int head_out, size_t *lds_bytes);
/* All arrays are HOST pointers in torch's layouts: enc_weights / enc_biases num_encoder_layers pointers each ([out][in], [out]);
 * w_ih [3 hidden][dims[L]], w_hh [3 hidden][hidden], b_ih, b_hh [3 hidden] (weight_ih_l0 ... of torch.nn.GRU); head_weight
 * [P][hidden], head_bias [P].  hidden_activation: AGX_POLICY_ELU or _RELU.  Packing and ownership as agx_policy_create; like it,
 * create, the setters and destroy are the set-up calls (sf_inference_class.py:40-78 builds and loads the torch module here).  */
int agx_recurrent_create(int num_encoder_layers, const int32_t *dims, int hidden, int num_actions, int adaptive_stddev,
                         const float *const *enc_weights, const float *const *enc_biases, const float *w_ih, const float *w_hh,
                         const float *b_ih, const float *b_hh, const float *head_weight, const float *head_bias, int hidden_activation,
                         AgxRecurrent **out);
/* sample-factory's RunningMeanStdInPlace as agx_policy_set_input_norm states rl_games' (sf_inference_class.py:86,
 * nn_inference_class.py:82 prepare_and_normalize_obs): HOST mean, denom [in]; both NULL: off.                               */
int agx_recurrent_set_input_norm(AgxRecurrent *p, const float *mean, const float *denom, float clip);
/* the constant log-std [num_actions] of a head that is not adaptive (action_parameterization.learned_stddev); HOST; NULL: none */
int agx_recurrent_set_logstd(AgxRecurrent *p, const float *logstd);
/* One step of the actor for num_envs envs (sf_inference_class.py:80-101 get_action, nn_inference_class.py:77-101): obs [N][in],
 * hidden [N][hidden] read and written IN PLACE, actions [N][A]; one launch, no allocation, no host synchronisation.
 * done0, done1 (optional): per-env bytes (torch bool / uint8); an env with either set has its state zeroed BEFORE the cell
 * (default: what sample-factory's sampler does with the flags of the step that produced obs), or with AGX_POLICY_RESET_AFTER
 * evaluates with the state it has and STORES zero (dce_nn_navigation.py: get_action, then reset(ids)).
 * mu_out, logstd_out (optional, [N][A]): the means and the log-std this call used.  AGX_POLICY_SAMPLE / _CLAMP and eps as
 * agx_policy_act, sigma = exp_cw(logstd); the device generator is the stream of agx_policy_noise.  num_envs = 0 does nothing. */
int agx_recurrent_act(AgxRecurrent *p, int num_envs, const float *obs, float *hidden, const uint8_t *done0, const uint8_t *done1,
                      float *actions, float *mu_out, float *logstd_out, const float *eps, int flags, uint64_t rng_seed,
                      int env_index_base, int env_step, void *stream);
/* Diagnostic: noise_out [N][A] <- the normals the NULL-eps form draws (the values of agx_policy_noise for A actions).          */
int agx_recurrent_noise(const AgxRecurrent *p, int num_envs, uint64_t rng_seed, int env_index_base, int env_step, float *noise_out,
                        void *stream);
int agx_recurrent_destroy(AgxRecurrent *p);

#ifdef __cplusplus
}
#endif
#endif /* AERIAL_GYM_HIP_H */
