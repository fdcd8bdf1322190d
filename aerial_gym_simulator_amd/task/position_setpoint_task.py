"""PositionSetpointTask with the reference's API and step ordering
(aerial_gym/task/position_setpoint_task/position_setpoint_task.py:21-203); reward, crash,
truncation and observation packing run in agx_reward_position / agx_obs_position."""
import torch

from .. import _lib
from ..utils.logging import CustomLogger
from ..utils import roctx
from .setpoint_task_base import SetpointTaskBase

logger = CustomLogger("position_setpoint_task")


class PositionSetpointTask(SetpointTaskBase):
    OBSERVATION_SPACE_SHAPE = (13,)
    # (actions / prev_actions are re-bound to the caller's tensors every step and never read: not state)
    SNAPSHOT_TENSORS = (("target_soa", "soa"), ("rewards", "soa"), ("task_obs[observations]", "aos"), ("task_obs[collisions]", "aos"))
    SNAPSHOT_HOST = ("counter",)

    def __init__(self, task_config, seed=None, num_envs=None, headless=None, device=None, use_warp=None):
        # args={"lean_step": True} (opt-in, effective above 65 536 envs: EnvManager._enable_lean_step) lets the fused step stop
        # maintaining the tensors that exist only to be looked at through the dict.  Never implied by num_envs: the dict behaves
        # the same at every batch size unless the caller asks otherwise.
        args = dict(task_config.args) if isinstance(task_config.args, dict) else task_config.args
        super().__init__(task_config, seed, num_envs, headless, device, use_warp, env_args=args)
        self.sim_env.rows_written_twice_per_step = bool(self.task_config.return_state_before_reset)  # see sharding.StepGather
        self._plan = None
        self._proof_watch = self._proof_record = None
        self._fuse_with_env()

    def _fuse_with_env(self):
        """Ask the EnvManager to evaluate this task's reward / crash / truncation / reset set in the
        env-step launch and its observation in the reset launch (2 launches per task.step())."""
        env = self.sim_env
        if env._buffers is None:
            return
        T = _lib.AgxTaskArgs()
        T.kind = _lib.TASK_POSITION
        T.episode_len = int(self.task_config.episode_len_steps)
        T.reset_on_collision = int(env.cfg.env.reset_on_collision)
        T.target = _lib.dptr(self.target_soa)
        T.reward = _lib.dptr(self.rewards)
        env.task_args = T
        env.post_obs = (_lib.dptr(self.target_soa), _lib.dptr(self.task_obs["observations"]))
        self._plan = self._strict = None
        e = env.cfg.env
        plain = (env.scene.num_assets == 0 and env.robot_manager.warp_sensor is None and env.robot_manager.imu_sensor is None
                  # host-evaluated controller / robot classes run between launches: the general path dispatches them
                  and not getattr(env.robot_manager.robot, "external_controller", False)
                  and not getattr(env.robot_manager.robot, "external_robot", False)
                  and not env.robot_manager.robot.cfg.disturbance.enable_disturbance
                  and env._com is None  # centre of mass off the base link: agx_env_step_com, which the step plans do not launch
                  and e.num_physics_steps_per_env_step_std == 0 and not self.task_config.return_state_before_reset)
        draws = env.strict_draw_plan() if (plain and env.strict_rng) else None
        if plain and (not env.strict_rng or draws is not None):
            # whole task.step() = one host call launching two kernels (agx_position_task_step)
            import ctypes as C

            plan = _lib.AgxPositionStepPlan()
            plan.params, plan.buf = C.pointer(env._params), C.pointer(env._buffers)
            plan.task, plan.reset = C.pointer(T), C.pointer(env._reset_args)
            plan.target, plan.obs = env.post_obs
            plan.num_envs, plan.k_substeps = env.num_envs, int(e.num_physics_steps_per_env_step_mean)
            self._plan = plan
            self._plan_ref = C.byref(plan)       # (passed as it is every step: ctypes would build a new reference per call)
            self._plan_task = T                  # the struct plan.task points at (plan.task.contents builds a new object per access)
            self._plan_episode_len = T.episode_len
            self._plan_fn = env._lib.agx_position_task_step
            self._action_shape = (env.num_envs, env.num_robot_actions)
            self._publish_step_flags()
            self._proof_watch = None
            if not env.strict_rng:
                self._enable_single_launch(plan)
            if env.strict_rng:
                # reference-faithful RNG consumption, one host call per step: the two launches above with, between them, the
                # reset flag published into a mapped host word the call spins on (no stream synchronisation) and -- only on a
                # step with resets, like the reference's `if len(env_ids) > 0` -- the reset's seven rand_like draws as one launch
                # that reproduces torch's own numbers (csrc/agx_strict.hip); the generator's offset is moved by what they consume
                sp = _lib.AgxStrictStepPlan()
                if getattr(self, "_strict_word", None) is not None:  # (fused again after a re-bind)
                    env._lib.agx_host_word_destroy(self._strict_word)
                word = C.POINTER(C.c_uint32)()
                _lib.check(env._lib.agx_host_word_create(C.byref(word)), "agx_host_word_create")
                self._strict_word = word
                sp.plan, sp.host_word = C.pointer(plan), word
                sp.count = len(draws["tensors"])
                for j, t in enumerate(draws["tensors"]):
                    sp.out[j], sp.numel[j] = t.data_ptr(), t.numel()
                sp.sm_count, sp.max_threads_per_sm = draws["sm_count"], draws["max_threads_per_sm"]
                self._strict = sp
                self._strict_ref = C.byref(sp)
                self._strict_gen = draws["generator"]
                self._strict_drew, self._strict_after = C.c_int(0), C.c_uint64(0)
                self._strict_out = (C.byref(self._strict_drew), C.byref(self._strict_after))
                self._strict_fn = env._lib.agx_position_task_step_strict
                self._plan_fn = self._strict_step

    def _enable_single_launch(self, plan):
        """Single-launch steps (include/aerial_gym_hip.h, AgxPositionStepPlan.proof_*; on unless args={"single_launch_step":
        False}): the kernels leave a record of each step's end in mapped host memory, and agx_position_task_step issues a step
        whose reset outcome it proves from that record as ONE launch.  The proof is about what the KERNELS did: whenever the host
        may have changed what it rests on -- the state, target, sim_steps or motor-thrust tensors written through torch (their
        version counters move), any other public call on the env, a new episode length -- the records up to now are void
        (`proof_min_tag`, set in step())."""
        import ctypes as C

        env = self.sim_env
        if not bool(env.env_args.get("single_launch_step", True)) or env.num_envs > 65536 or env._params.num_motors != 4:
            return
        nb = (env.num_envs + 15) // 16
        self._proof_slots = torch.zeros(2 * nb * _lib.PROOF_SLOT_WORDS, dtype=torch.int32, device=self.device)
        self._proof_violation = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._free_proof_record()
        rec = C.c_void_p()
        _lib.check(env._lib.agx_host_record_alloc(_lib.PROOF_RECORD_WORDS * 4, C.byref(rec)), "agx_host_record_alloc")
        self._proof_record = rec
        plan.proof_slots, plan.proof_violation = _lib.dptr(self._proof_slots), _lib.dptr(self._proof_violation)
        plan.proof_record = rec.value
        plan.proof_min_tag = (env.step_counter + 1) & 0x7FFFFFFF
        plan.max_lag = int(env.env_args.get("single_launch_max_lag", 8))
        g = env.global_tensor_dict
        self._proof_watch = (g["robot_state_soa"], self.target_soa, g["sim_steps"],
                             env.robot_manager.robot.control_allocator.motor_model.thrust_soa)
        self._proof_versions = None
        self._proof_calls = -1

    def _free_proof_record(self):
        if self._proof_record is not None:
            self.sim_env._lib.agx_host_record_free(self._proof_record)
            self._proof_record = None

    def single_launch_stats(self):
        """How the fast path's steps ran: counts per mode (two launches, ONE launch with some env certainly resetting, ONE
        launch with none resetting) and per reason (AGX_PROOF_*), and the device's violation word (reads it: synchronises)."""
        p = self._plan
        if p is None:
            return None
        return {"modes": dict(zip(_lib.STEP_MODES, (int(x) for x in p.mode_count))),
                "reasons": dict(zip(_lib.PROOF_REASONS, (int(x) for x in p.reason_count))),
                "violations": int(self._proof_violation.item()) if self._proof_watch is not None else 0}

    def _strict_step(self, plan_ref, actions_ptr, stream):
        """agx_position_task_step in the strict mode (same signature): generator state in, offset out"""
        sp, gen = self._strict, self._strict_gen
        self.sim_env.num_physics_steps()  # (the reference draws random.gauss(mean, std) every step, std = 0 included: same consumption)
        sp.seed, sp.offset = gen.initial_seed() & 0xFFFFFFFFFFFFFFFF, gen.get_offset()
        rc = self._strict_fn(self._strict_ref, actions_ptr, self._strict_out[0], self._strict_out[1], stream)
        if rc == 0 and self._strict_drew.value:
            gen.set_offset(self._strict_after.value)
        return rc

    def _restored(self, host, whole):
        super()._restored(host, whole)
        if self._proof_watch is not None:
            # the single-launch proof reads a record the KERNELS leave in host memory, tagged with the step index.  Steps still in
            # flight would go on publishing records of the abandoned timeline under tags the restored step counter is about to
            # reach again: wait for them here, once per restore.  What is in the record then carries a tag at or above the next
            # step's and proves nothing (AGX_PROOF_TAG) until the kernels of the new timeline have published theirs.
            torch.cuda.current_stream(self.sim_env.device).synchronize()
            self._proof_versions = None
            self._plan.slot_run = 0

    def close(self):
        if getattr(self, "_strict_word", None) is not None:
            self.sim_env._lib.agx_host_word_destroy(self._strict_word)
            self._strict_word = None
        self._proof_watch = None
        if self._plan is not None:
            self._plan.proof_slots = self._plan.proof_record = self._plan.proof_violation = None
        self._free_proof_record()
        super().close()

    @roctx.ranged("PositionSetpointTask.step")
    def step(self, actions):
        self.counter += 1
        self.prev_actions = self.actions  # previous step's tensor (no copy; the reward does not read it)
        self.actions = actions
        env = self.sim_env
        if (self._plan is not None and actions.dtype is torch.float32 and actions.is_contiguous() and actions.is_cuda
                and actions.shape == self._action_shape):  # anything else takes the general path, which raises like the reference
            # fast path: same two launches as the general path below, one host call.  Host time is 0.9 of this step at 8192 envs
            # (bench.py `host.share_of_step`): nothing here allocates or looks anything up twice.
            env._begin_step(library_advances=True)  # (the library flips the parity and moves the peer push; not a counted call)
            el = self.task_config.episode_len_steps
            if el != self._plan_episode_len:
                self._plan_task.episode_len = self._plan_episode_len = int(el)
                self._proof_versions = None
            w = self._proof_watch
            if w is not None:  # did the host touch what the single-launch proof rests on since the last step?
                v = (w[0]._version, w[1]._version, w[2]._version, w[3]._version)
                if v != self._proof_versions or env._calls != self._proof_calls:
                    self._proof_versions, self._proof_calls = v, env._calls
                    self._plan.proof_min_tag = (env.step_counter + 1) & 0x7FFFFFFF  # only records of this step on count
            rc = self._plan_fn(self._plan_ref, actions.data_ptr(), _lib.current_stream(env.device))
            if rc != 0:
                _lib.check(rc, "agx_position_task_step")
            env._end_step()
            return (self.task_obs, self.rewards, self.terminations, self.truncations, self.infos)
        if env.task_args is not None:
            env.task_args.episode_len = int(self.task_config.episode_len_steps)
        return self._step_env_and_return()

    def compute_rewards_and_crashes(self, obs_dict):
        """compute_reward + `truncations = sim_steps > episode_len` (reference :205-229,:172-174)."""
        env = self.sim_env
        env._require_device()
        if env.take_produced(env.REWARD):  # by the fused epilogue of agx_env_step
            return self.rewards, self.terminations
        _lib.check(
            env._lib.agx_reward_position(env._buffers, env.num_envs, _lib.dptr(self.target_soa),
                                         int(self.task_config.episode_len_steps), int(env.cfg.env.reset_on_collision),
                                         _lib.dptr(self.rewards), env._stream()),
            "agx_reward_position",
        )
        env.mark_produced(env.RESET_SET)  # the reward kernel wrote this step's reset set
        return self.rewards, self.terminations

    def process_obs_for_task(self):
        env = self.sim_env
        env._require_device()
        self._publish_step_flags()
        if env.take_produced(env.OBSERVATION):  # by agx_post_step_position
            return
        _lib.check(
            env._lib.agx_obs_position(env._buffers, env.num_envs, _lib.dptr(self.target_soa),
                                      _lib.dptr(self.task_obs["observations"]), env._stream()),
            "agx_obs_position",
        )
