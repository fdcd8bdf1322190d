"""Test helper: numpy-float32 restatement of agx_radar_image_obs and agx_reward_radar_navigation and of the radar image's device-noise
rule.  It is the comparator of the GPU tests (the reference's code does not exist where they run) and is itself pinned to the
reference bit for bit by tests/test_radar_navigation_task.py (tests/golden/radar_cr/*.npz: the reference's own code with correctly
rounded elementary functions).

Every array is float32 and every + - * / sqrt one rounded float32 operation; exp is evaluated in float64 and rounded once; the fused
multiply-adds inside torch.norm are explicit (sim2real_ref.norm3).  The noise-free part of the image (ranges, time to collision,
min-pool, inverse) and the Philox uniforms come from the CPU oracle as it stands (oracle.lidar_image_obs, oracle.rng_fill)."""
import numpy as np
from sim2real_ref import F, _el, cross, dot3, f32, norm3, ssa

RNG_RADAR_NOISE = 11  # agx_rng.h


def exp_reward(mag, ex, v):
    return F(mag) * _el(np.exp, -(v * v) * F(ex))


def exp_penalty(mag, ex, v):
    return F(mag) * (_el(np.exp, -(v * v) * F(ex)) - F(1.0))


def reward(pos_err, vveh, wbody, yaw_error, crashes, action, prev_action, ttc, curriculum_progress, rp, radar=True):
    """compute_reward of radar_navigation_task.py:179-342 (radar=False: of lidar_navigation_task.py:554-719, which clamps the
    vehicle-frame x velocity from the other side) in the operation order of k_reward_lidar_navigation"""
    pe, v, a, pa, ye, ttc, rp = f32(pos_err), f32(vveh), f32(action), f32(prev_action), f32(yaw_error), f32(ttc), f32(rp)
    wz = f32(wbody)[:, 2]
    cpf = F(curriculum_progress)
    mult = F(1.0 + 2.0 * float(cpf))  # MULTIPLICATION_FACTOR_REWARD is a python double
    one, zero = F(1.0), F(0.0)
    dist = norm3(pe)
    pos_reward = exp_reward(rp[0], rp[1], dist)
    very_close = exp_reward(rp[2], rp[3], dist)
    vel_norm = norm3(v)
    vden, gden = vel_norm + F(1e-6), dist + F(1e-6)
    vdc = ((v[:, 0] / vden) * (pe[:, 0] / gden) + (v[:, 1] / vden) * (pe[:, 1] / gden)) + (v[:, 2] / vden) * (pe[:, 2] / gden)
    reasonable_vel = exp_reward(2.0, 2.0, vel_norm - F(2.0))
    vdc_reward = np.where(vdc > 0, rp[4] * vdc * reasonable_vel, F(-0.2)).astype(np.float32) * np.minimum(dist / F(3.0), one)
    vel_mag_pen = exp_penalty(2.0, 2.0, np.maximum(vel_norm - F(3.0), zero))
    close_to_goal = one - exp_reward(1.0, 2.0, dist)
    vx = np.minimum(v[:, 0], zero) if radar else np.maximum(v[:, 0], zero)
    neg_x_pen = exp_penalty(2.0, 8.0, vx) * close_to_goal
    vel_pen = vel_mag_pen + neg_x_pen
    low_vel = exp_reward(1.5, 10.0, vel_norm) + exp_reward(1.5, 0.5, vel_norm)
    correct_yaw = exp_reward(2.0, 0.2, ye) + exp_reward(4.0, 15.0, ye)
    alignment = exp_reward(1.0, 2.0, ye)
    low_angvel = exp_reward(1.5, 5.0, wz) * alignment
    stable = np.where(dist < one, (low_vel + correct_yaw) + low_angvel, zero).astype(np.float32)
    dist_reward = (F(20.0) - dist) / F(20.0)
    d = a - pa
    diff_pen = ((exp_penalty(rp[5], rp[6], d[:, 0]) + exp_penalty(rp[7], rp[8], d[:, 1])) + exp_penalty(rp[9], rp[10], d[:, 2])) \
        + exp_penalty(rp[11], rp[12], d[:, 3])
    abs_pen = ((cpf * exp_penalty(rp[13], rp[14], a[:, 0]) + cpf * exp_penalty(rp[17], rp[18], a[:, 2]))
               + cpf * exp_penalty(rp[19], rp[20], a[:, 3])) + cpf * exp_penalty(rp[15], rp[16], a[:, 1])
    total_pen = diff_pen + abs_pen
    ttc_pen = exp_reward(-3.0, 2.0, ttc * ttc)
    r = mult * (((((((pos_reward + very_close * alignment) + vdc_reward) + dist_reward) + stable) + vel_pen) + total_pen) + ttc_pen)
    return np.where(np.asarray(crashes).astype(bool), rp[21], r).astype(np.float32)


def quat_rotate_inverse(q, v):
    """utils/math.py:340-347: a - b + c"""
    q, v = f32(q), f32(v)
    w = q[:, 3:4]
    s = F(2.0) * (w * w) - F(1.0)
    c = cross(q[:, 0:3], v)
    d = dot3(q[:, 0:3], v)[:, None]
    return (v * s - c * w * F(2.0)) + q[:, 0:3] * d * F(2.0)


def reward_inputs(target, position, qveh, euler_z, target_yaw):
    """what the kernel derives from the env buffers before compute_reward (compute_rewards_and_crashes, :129-142):
    (pos_error_vehicle_frame, yaw_error)"""
    pe = quat_rotate_inverse(qveh, f32(target) - f32(position))
    return pe, ssa(f32(target_yaw) - ssa(f32(euler_z)))


def image_obs(orc, pointcloud, position, linvel, noise_mask=None, noise_val=None, invalid_mask=None, ph=3, pw=6):
    """process_image_observation (:24-63) + add_noise_to_downsampled_lidar_data (:6-21): pointcloud [N, H, W, 3] ->
    (time_to_collision [N], 1 / pooled range [N, (H // ph) * (W // pw)]).  The oracle's `+= noise_val where noise_mask == 1` is the
    radar's; its low-row rule from row 0 on with the value -1 is `= -1 where invalid_mask == 1` (same order: after the noise)."""
    pc = f32(pointcloud)
    n, oh, ow = pc.shape[0], pc.shape[1] // ph, pc.shape[2] // pw
    shape = lambda a: None if a is None else f32(a).reshape(n, oh, ow)  # noqa: E731
    low_val = None if invalid_mask is None else np.full((n, oh, ow), -1.0, np.float32)
    return orc.lidar_image_obs(pc, f32(position), f32(linvel), ph=ph, pw=pw, low_row0=0, noise_mask=shape(noise_mask),
                               noise_val=shape(noise_val), low_mask=shape(invalid_mask), low_val=low_val)


def device_noise(orc, seed, steps, cells):
    """the three tensors k_radar_image_obs draws for envs 0 .. len(steps) - 1 (env i in its env step steps[i]): stream
    RNG_RADAR_NOISE, block c = pooled cell c -> u0 < 0.03: noise of 9.8 u1 + 0.2; u2 < 0.8: invalid.  [N, cells] each."""
    u = orc.rng_fill(seed, np.asarray(steps), RNG_RADAR_NOISE, 4 * cells).reshape(len(steps), cells, 4)
    noise_mask = (u[..., 0] < F(0.03)).astype(np.float32)
    noise_val = ((F(10.0) - F(0.2)) * u[..., 1] + F(0.2)).astype(np.float32)
    invalid_mask = (u[..., 2] < F(0.8)).astype(np.float32)
    return noise_mask, noise_val, invalid_mask
