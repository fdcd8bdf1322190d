"""Open-loop rollouts: T env steps of a raw EnvManager under known actions as ONE launch (agx_env_rollout, k_env_step_rollout), with
the trajectories recorded on the device.

    rec = env.rollout(actions, steps=None, record=(), out=None)

leaves the simulator exactly where `for t in range(T): env.step(actions_t)` leaves it -- every tensor of the dict, the host's
counters, python's `random` stream and the device-generator streams, bit for bit (DESIGN.md section
3.9).  The reference has no counterpart: its step-response scripts (examples/sys_id.py:56-90, examples/tune_controllers.py:121-222)
call EnvManager.step once per step and copy one dict tensor to a host-indexed sequence after each.
"""
import torch

from . import _lib

# key -> (source, first row, rows): what `record=` may name.  `motor_thrusts` is the motor model's current_motor_thrust [N, M]
# (robot.control_allocator.motor_model), the only key that is not an entry of the tensor dict.
RECORD_KEYS = {
    "robot_position": (_lib.REC_STATE, 0, 3),
    "robot_orientation": (_lib.REC_STATE, 3, 4),
    "robot_linvel": (_lib.REC_STATE, 7, 3),
    "robot_angvel": (_lib.REC_STATE, 10, 3),
    "robot_euler_angles": (_lib.REC_DERIVED, 0, 3),
    "robot_vehicle_orientation": (_lib.REC_DERIVED, 3, 4),
    "robot_vehicle_linvel": (_lib.REC_DERIVED, 7, 3),
    "robot_body_linvel": (_lib.REC_DERIVED, 10, 3),
    "robot_body_angvel": (_lib.REC_DERIVED, 13, 3),
    "motor_thrusts": (_lib.REC_THRUST, 0, None),  # rows: the robot's motor count
    "crashes": (_lib.REC_CRASH, 0, 1),
}


class RolloutRecord:
    """What a rollout recorded.  `rec[key]` is a float32 [T, N, C] view: rec[key][t] holds what the dict's tensor of that name
    holds after step t (`crashes` as 0.0 / 1.0).  The storage is ONE tensor `data` [T, channels, N], component-major, so that a
    wave's store of one channel is one contiguous line; the views are its permuted slices, like tensors.aos_view.
    `first_crash_step` int32 [N]: the first step whose crash flag was set, or -1."""

    def __init__(self, keys, rows, steps, num_envs, device):
        self.keys, self.steps, self.num_envs = tuple(keys), int(steps), int(num_envs)
        self._rows = tuple(rows)
        self.channels = sum(self._rows)
        self.data = torch.empty((self.steps, self.channels, self.num_envs), dtype=torch.float32, device=device) if self.channels else None
        self.first_crash_step = torch.empty(self.num_envs, dtype=torch.int32, device=device)
        self.substeps = None  # int32 [T] on the device: the steps' sub-step counts, when they differ
        self._views, at = {}, 0
        for key, r in zip(self.keys, self._rows):
            self._views[key] = self.data[:, at:at + r, :].permute(0, 2, 1)
            at += r
        self._c = None

    def __getitem__(self, key):
        return self._views[key]

    def __contains__(self, key):
        return key in self._views

    def matches(self, keys, rows, steps, num_envs, device):
        return (self.keys == tuple(keys) and self._rows == tuple(rows) and self.steps == int(steps) and self.num_envs == int(num_envs)
                and self.first_crash_step.device == torch.device(device))

    def c_record(self):
        """the AgxRolloutRecord of this record (built once: the storage never moves), or None without channels"""
        if self.channels == 0:
            return None
        if self._c is None:
            R = _lib.AgxRolloutRecord()
            R.out, R.channels = _lib.dptr(self.data), self.channels
            c = 0
            for key, r in zip(self.keys, self._rows):
                source, first, _ = RECORD_KEYS[key]
                for j in range(r):
                    R.source[c], R.component[c] = source, first + j
                    c += 1
            self._c = R
        return self._c


def _check_arguments(env, actions, steps, record, out):
    """shape, dtype, device, `steps`, keys and `out`: ValueError / TypeError before anything else is looked at.  Returns
    (T, per_step, keys, rows)."""
    N, A = env.num_envs, env.num_robot_actions
    if not isinstance(actions, torch.Tensor):
        raise TypeError(f"rollout: actions is a float32 tensor [N, A] or [T, N, A], got {type(actions).__name__}")
    if actions.dtype != torch.float32:
        raise ValueError(f"rollout: actions must be float32, got {actions.dtype}")
    dev = torch.device(env.device)
    if actions.device.type != dev.type or (dev.index is not None and actions.device.index not in (None, dev.index)):
        raise ValueError(f"rollout: actions live on {actions.device}, the env on {env.device}")
    if not actions.is_contiguous():
        raise ValueError("rollout: actions must be contiguous")
    if actions.dim() == 2:
        if tuple(actions.shape) != (N, A):
            raise ValueError(f"rollout: actions of shape {tuple(actions.shape)}; a held action tensor is [{N}, {A}]")
        if steps is None:
            raise ValueError("rollout: `steps` is required with a held [N, A] action tensor")
        per_step = False
    elif actions.dim() == 3:
        if tuple(actions.shape[1:]) != (N, A) or actions.shape[0] < 1:
            raise ValueError(f"rollout: actions of shape {tuple(actions.shape)}; a step schedule is [T, {N}, {A}] with T >= 1")
        if steps is not None and int(steps) != actions.shape[0]:
            raise ValueError(f"rollout: steps={steps} with a schedule of {actions.shape[0]} steps (pass None or {actions.shape[0]})")
        steps, per_step = actions.shape[0], True
    else:
        raise ValueError(f"rollout: actions of shape {tuple(actions.shape)}; expected [{N}, {A}] or [T, {N}, {A}]")
    if isinstance(steps, bool) or int(steps) != steps or int(steps) < 1:
        raise ValueError(f"rollout: steps must be an integer >= 1, got {steps!r}")
    if isinstance(record, str):
        raise TypeError("rollout: `record` is a tuple of keys, e.g. record=('robot_position',)")
    keys = tuple(record)
    M = int(env.robot_manager.robot.cfg.control_allocator_config.num_motors)
    rows = []
    for key in keys:
        if key not in RECORD_KEYS:
            raise ValueError(f"rollout: '{key}' cannot be recorded; the keys are {', '.join(RECORD_KEYS)}")
        if keys.count(key) > 1:
            raise ValueError(f"rollout: '{key}' is named twice in `record`")
        rows.append(RECORD_KEYS[key][2] or M)
    if sum(rows) > _lib.ROLLOUT_MAX_CHANNELS:
        raise ValueError(f"rollout: {sum(rows)} recorded channels, at most {_lib.ROLLOUT_MAX_CHANNELS}")
    if out is not None:
        if not isinstance(out, RolloutRecord):
            raise TypeError("rollout: `out` is the RolloutRecord an earlier rollout returned")
        if not out.matches(keys, rows, steps, N, env.device):
            raise ValueError(f"rollout(out=): `out` holds {out.steps} steps x {out.num_envs} envs of {out.keys}, this call asks for "
                             f"{int(steps)} x {N} of {keys}")
    return int(steps), per_step, keys, rows


def refusal(env):
    """the reason this env manager cannot roll out in one launch, or None.  Each names what the eager step does between or
    beside its launches that the single launch cannot do."""
    robot, g = env.robot_manager.robot, env.global_tensor_dict
    B = env._buffers
    if env.task_args is not None or env._state_owner is not None or env.post_step_launch is not None or env.post_obs is not None:
        return ("rollout on a task-owned env: the task's step also writes the reward and the reset set and resets envs "
                "(task-level rollouts are not built); build the env with SimBuilder().build_env(...)")
    if getattr(robot, "external_controller", False) or getattr(robot, "external_robot", False):
        return "rollout with a user-registered controller or robot class: it is evaluated on the host between the physics sub-steps"
    if dict.get(g, "env_actions") is not None:
        return "rollout with env_actions (moving obstacles): the obstacles are moved by launches of their own before every step"
    if env.strict_rng and robot.cfg.disturbance.enable_disturbance:
        return "rollout with strict_rng and the disturbance enabled: the draws come from the host's generator, step by step"
    if env.robot_manager.imu_sensor is not None:
        return "rollout with an IMU: robot_manager.post_physics_step launches the IMU update after every step"
    if env._lean or env.env_args.get("lean_step"):
        return "rollout with args={'lean_step': True}: the lean step does not maintain the derived and action tensors"
    if getattr(env, "step_graph_mode", False):
        return "rollout with a task stepping by hipGraph replay (args={'step_graph': True})"
    if env._push is not None or (B is not None and (B.step_rows[0] or B.step_rows[1] or B.step_counter_dev)):
        return "rollout with bound exchange rows / peer push or a device step counter (sharded or captured stepping)"
    if env._kind_flags & _lib.LAUNCH_ROV:
        return "rollout of an ROV (the k_env_step_rov kind) is not built"
    if env._com is not None:
        return "rollout of a robot whose centre of mass is off the base link (the k_env_step_com kind) is not built"
    return None


def rollout(env, actions, steps=None, record=(), out=None):
    T, per_step, keys, rows = _check_arguments(env, actions, steps, record, out)
    env._require_device()
    why = refusal(env)
    if why is not None:
        raise RuntimeError(why)
    rec = out if out is not None else RolloutRecord(keys, rows, T, env.num_envs, env.device)
    # the T sub-step counts, drawn up front in the order the separate steps would draw them
    ks = [env.num_physics_steps() for _ in range(T)]
    if max(ks) > _lib.MAX_SUBSTEPS:
        raise ValueError(f"rollout: a step of {max(ks)} physics sub-steps (at most {_lib.MAX_SUBSTEPS})")
    B = env._buffers
    start = env.step_counter
    env._begin_step()  # step 0: the record emptied, the call counted, B.step_counter = start, the flag parity flipped
    for k in ks:  # (not strict_rng: sets the probability of the in-kernel draw, exactly when the separate steps would)
        env._draw_disturbance(k)
    k_max = max(ks)
    k_dev = None
    if min(ks) != k_max:  # one count per step: a device [T] the record keeps (allocated on the first such call, reused after)
        if rec.substeps is None:
            rec.substeps = torch.empty(T, dtype=torch.int32, device=env.device)
        rec.substeps.copy_(torch.tensor(ks, dtype=torch.int32))
        k_dev = rec.substeps
    _lib.check(env._lib.agx_env_rollout(env._params, B, env.num_envs, _lib.dptr(actions), 1 if per_step else 0, T, k_max,
                                        _lib.dptr(k_dev), rec.c_record(), _lib.dptr(rec.first_crash_step), env._stream()),
               "agx_env_rollout")
    # steps 1 .. T-1 of the host's bookkeeping in closed form: what T - 1 more _begin_step() / _end_step() pairs leave
    env._calls += T - 1
    B.flag_parity ^= (T - 1) & 1
    env.step_counter = start + T
    B.step_counter = (start + T - 1) & 0x7FFFFFFF
    return rec
