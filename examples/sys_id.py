"""Step responses of the lmf2 controllers, the counterpart of the reference's examples/sys_id.py -- as ONE launch per action axis.

    PYTHONPATH=. python examples/sys_id.py [--mode velocity|attitude|acceleration] [--num_envs 16] [--json]

The reference runs 500 `env_manager.step` calls per action axis and copies one dict tensor into `observation_sequence[i]` from the
host after each (sys_id.py:56-90).  Here the 500-step schedule -- zero for the first half, ACTION_MAGNITUDE on one axis for the second
-- is a [T, N, 4] tensor handed to `env.rollout(...)` with `record=` of the response tensor: one launch, the trajectory stays on the
device, and the time constant (first step at which the response passes 63.2 % of the command) is ONE reduction over the record.
Every env flies the same schedule from its own start state (and, on lmf2, under its own disturbance draws), so the script reports
the median over the envs next to env 0, which is what the reference prints.

The response tensors are the reference's (DICT_MAP): robot_euler_angles for the attitude mode, robot_vehicle_linvel for the velocity
mode, plus robot_angvel z for the yaw-rate axis.  Its acceleration mode reads `imu_measurement`; a rollout carries no IMU, so the
response there is the acceleration the recorded robot_vehicle_linvel implies, (v[t] - v[t-1]) / dt.  Without --json a table is
printed; no plot is drawn."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aerial_gym_simulator_amd  # noqa: E402,F401
from aerial_gym_simulator_amd.sim.sim_builder import SimBuilder  # noqa: E402

CONTROLLER_MODES = {"attitude": "lmf2_attitude_control", "velocity": "lmf2_velocity_control", "acceleration": "lmf2_acceleration_control"}
DICT_MAP = {"attitude": "robot_euler_angles", "velocity": "robot_vehicle_linvel", "acceleration": "robot_vehicle_linvel"}
AXES = ("X", "Y", "Z", "Yaw Rate")
ACTION_MAGNITUDE, SIM_DURATION_IN_SECONDS, DEV = 1.0, 5.0, "cuda:0"


def identify(mode, num_envs):
    env = SimBuilder().build_env(sim_name="base_sim", env_name="empty_env", robot_name="lmf2", controller_name=CONTROLLER_MODES[mode],
                                 args={"ray_cast_sensors": "off"}, device=DEV, num_envs=num_envs, headless=True, use_warp=False)
    dt = float(env.global_tensor_dict["dt"])
    T = int(SIM_DURATION_IN_SECONDS / dt)
    half, key = T // 2, DICT_MAP[mode]
    schedule = torch.zeros(T, env.num_envs, 4, device=DEV)
    step_of = torch.arange(T - half, device=DEV).unsqueeze(1)
    rec, rows = None, []
    for axis in range(4):
        env.reset()
        schedule.zero_()
        schedule[half:, :, axis] = ACTION_MAGNITUDE
        rec = env.rollout(schedule, record=(key, "robot_angvel"), out=rec)  # the second axis on reuses the first one's buffers
        response = torch.cat([rec[key], rec["robot_angvel"][:, :, 2:3]], dim=2)  # [T, N, 4]: x y z, yaw rate
        if mode == "acceleration":
            response[1:, :, 0:3] = (rec[key][1:] - rec[key][:-1]) / dt
            response[0, :, 0:3] = 0.0
        channel = axis - 1 if mode == "attitude" else axis  # the attitude law's actions are thrust, roll, pitch, yaw rate
        if channel < 0:
            rows.append({"axis": AXES[axis], "time_constant_env0": None, "time_constant_median": None, "crashed_envs": 0})
            continue
        above = response[half:, :, channel] > ACTION_MAGNITUDE * 0.63212
        first = torch.where(above, step_of, T).amin(dim=0)  # the one reduction: first step past 63.2 %, or T
        tau = torch.where(first < T, first.to(torch.float32) * dt, torch.full((), float("nan"), device=DEV))
        reached = tau[~torch.isnan(tau)]
        rows.append({"axis": AXES[axis], "time_constant_env0": None if bool(torch.isnan(tau[0])) else round(float(tau[0]), 4),
                     "time_constant_median": round(float(reached.median()), 4) if reached.numel() else None,
                     "envs_reached": int(reached.numel()), "crashed_envs": int((rec.first_crash_step >= 0).sum()),
                     "final_response_env0": round(float(response[-1, 0, channel]), 4)})
    return {"mode": mode, "controller": CONTROLLER_MODES[mode], "response": key, "num_envs": env.num_envs, "steps": T, "dt": dt,
            "action_magnitude": ACTION_MAGNITUDE, "axes": rows}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=sorted(CONTROLLER_MODES), default="velocity")
    ap.add_argument("--num_envs", type=int, default=16)
    ap.add_argument("--json", action="store_true", help="one JSON object on stdout instead of the table")
    a = ap.parse_args()
    out = identify(a.mode, a.num_envs)
    if a.json:
        print(json.dumps(out))
    else:
        print(f"System identification of {out['controller']} ({out['steps']} steps of {out['dt']} s, {out['num_envs']} envs, one launch per axis)")
        for r in out["axes"]:
            print(f"  action {r['axis']:>8}: time constant env 0 {r['time_constant_env0']} s, median {r['time_constant_median']} s")
