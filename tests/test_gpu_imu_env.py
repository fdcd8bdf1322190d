"""GPU: the IMU as EnvManager and IMUSensor wire it -- base_quadrotor_with_imu in empty_env, 83 envs, 3 physics sub-steps per
env step, 12 steps with resets of strict subsets -- against orc.imu_update / orc.imu_reset fed with what the env itself holds at
the update (imu_body_force_soa, robot_orientation, robot_body_angvel), the sim config's gravity, the robot's mass and the random
numbers of that step: the restated RNG_IMU / RNG_IMU_RESET streams (imu_ref.py) with the device generator, the recorded draws of
the random source under strict_rng.  The bias and the mount quaternions are carried by the test.

What would show here: a step counter that does not advance (every step the same normals), a wrong k (another noise slot, another
number of bias increments), a wrong slice of the strict-mode normals, an update placed behind the reset, a reset that reaches
envs outside the mask, gravity or mass from elsewhere.  The sensor's bias_std and max_bias_init_value are raised for the run:
with the reference's values (1e-6, 1e-3) a whole bias walk stays below the gates."""
import numpy as np
import pytest
import torch
from conftest import rel_err
from imu_ref import SQRT_DT, reset_draws, sensor_force, update_normals
from task_test_util import DEV, RecordingSource, config_restored, npy

pytestmark = pytest.mark.gpu
N, K, STEPS, SEED = 83, 3, 12, 0x1D0C0FFEE


class Recording(RecordingSource):
    """... keeping the uniform fills too, by tag"""

    def __init__(self, device):
        super().__init__(device)
        self.uniforms = {}

    def rand_into(self, out, tag=""):
        r = super().rand_into(out, tag=tag)
        self.uniforms[tag] = out.detach().clone()
        return r


@pytest.mark.parametrize("mode", ["device_generator", "strict_rng"])
def test_env_imu_measurement_follows_the_oracle(orc, mode):
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config.env_config import EmptyEnvCfg
    from aerial_gym_simulator_amd.config.sensor_config import BaseImuConfig
    from aerial_gym_simulator_amd.sim.sim_builder import SimBuilder

    strict = mode == "strict_rng"
    rs = Recording(DEV) if strict else None
    args = {"strict_rng": strict, "rng_seed": SEED}
    if strict:
        args["random_source"] = rs
    with config_restored(EmptyEnvCfg.env, ["num_physics_steps_per_env_step_mean", "num_envs"]), \
            config_restored(BaseImuConfig, ["bias_std", "max_bias_init_value"]):
        EmptyEnvCfg.env.num_physics_steps_per_env_step_mean = K
        BaseImuConfig.bias_std = [0.02, 0.03, 0.04, 0.05, 0.06, 0.07]
        BaseImuConfig.max_bias_init_value = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]
        env = SimBuilder().build_env("base_sim", "empty_env", "base_quadrotor_with_imu", "lee_position_control", DEV, args=args, num_envs=N)
        cfg = dict(bias_std=np.float32(BaseImuConfig.bias_std), noise_std=np.float32(BaseImuConfig.imu_noise_std),
                   max_value=np.float32(BaseImuConfig.max_measurement_value), max_bias_init=np.float32(BaseImuConfig.max_bias_init_value),
                   min_rot=np.deg2rad(np.float32(BaseImuConfig.min_euler_rotation_deg)), max_rot=np.deg2rad(np.float32(BaseImuConfig.max_euler_rotation_deg)))
        assert env.cfg.env.num_physics_steps_per_env_step_std == 0 and not BaseImuConfig.world_frame
        g, imu = env.get_obs(), env.robot_manager.imu_sensor
        gravity, mass = np.float32(env.sim_config.sim.gravity), float(g["robot_mass"][0])
        assert abs(gravity[2] + 9.81) < 1e-6 and 0.1 < mass < 5.0
        bias, sq = np.zeros((N, 6), np.float32), np.tile(np.float32([0, 0, 0, 1]), (N, 1))

        def reset_reference(mask):
            """orc.imu_reset of the envs of `mask` with the draws this reset used; every other env stays as the test carries it"""
            if strict:
                ub, ur = npy(rs.uniforms.pop("imu_bias_init")), npy(rs.uniforms.pop("imu_mount"))
            else:  # keyed by the env's episode, which the robot reset has just counted
                ub, ur = reset_draws(orc, SEED, npy(g["episode_count"]))
            orc.imu_reset(mask, ub, ur, cfg["max_bias_init"], cfg["min_rot"], cfg["max_rot"], bias, sq)
            assert rel_err(npy(imu.bias), bias) < 1e-6 and rel_err(npy(imu.sensor_quats), sq) < 1e-6
            keep = ~np.asarray(mask, bool)
            assert np.array_equal(npy(imu.bias)[keep], bias_dev_before[keep]) and np.array_equal(npy(imu.sensor_quats)[keep], sq_dev_before[keep])

        bias_dev_before, sq_dev_before = npy(imu.bias), npy(imu.sensor_quats)
        env.reset()
        reset_reference(np.ones(N, np.uint8))
        assert np.array_equal(npy(g["episode_count"]), np.ones(N, np.int32))
        pick = np.random.default_rng(5)
        target = torch.cat([g["robot_position"].clone() + 0.5, torch.zeros(N, 1, device=DEV)], dim=1)
        subsets, seen = 0, []
        for t in range(STEPS):
            assert env.step_counter == t
            if strict:
                rs.normals.clear()
            env.step(actions=target)
            torch.cuda.synchronize()
            # ---- the update: K sub-steps folded into one launch, on the state the step left
            if strict:
                assert len(rs.normals) == 1 and tuple(rs.normals[0].shape) == (2 * K, N, 6)  # sample_noise, update_bias per sub-step
                z = npy(rs.normals[0])
                zn, zb = z[2 * (K - 1)], z[1::2]
            else:
                zn, zb = (a.astype(np.float32) for a in update_normals(orc, SEED, N, t, K))
            quat = npy(g["robot_orientation"])
            force = sensor_force(npy(g["imu_body_force_soa"]).T, mass, quat, gravity)
            for s in range(K):
                ref = orc.imu_update(mass, gravity, SQRT_DT, False, 1, 1, cfg["bias_std"], cfg["noise_std"], cfg["max_value"], force, quat,
                                     npy(g["robot_body_angvel"]), sq, zn, zb[s], bias)
            meas = npy(g["imu_measurement"])
            assert rel_err(meas, ref) < 1e-5, t
            assert rel_err(npy(imu.bias), bias) < 1e-6, t
            seen.append(meas)
            # ---- the reset: a strict subset on some steps, one of them the last env (the second wave), nothing on the others
            mask = np.zeros(N, bool)
            if t % 4 == 1:
                mask = pick.random(N) < 0.3
                mask[N - 1], mask[0] = True, False
                g["truncations"][torch.from_numpy(mask).to(DEV)] = True
            bias_dev_before, sq_dev_before = npy(imu.bias), npy(imu.sensor_quats)
            episodes_before = npy(g["episode_count"])
            env.post_reward_calculation_step()
            torch.cuda.synchronize()
            assert np.array_equal(npy(g["reset_mask"]).astype(bool), mask), t
            if mask.any():
                subsets += 0 < mask.sum() < N
                assert np.array_equal(npy(g["episode_count"]), episodes_before + mask)
                reset_reference(mask)
            else:
                assert np.array_equal(npy(imu.bias), bias_dev_before) and np.array_equal(npy(imu.sensor_quats), sq_dev_before)
            assert np.array_equal(npy(g["imu_measurement"]), meas)  # the measurement is the update's: a reset does not touch it
        assert subsets >= 2 and np.isfinite(np.stack(seen)).all()
