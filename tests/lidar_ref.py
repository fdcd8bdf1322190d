"""Test helper: numpy-float32 restatement of the three LiDAR-navigation kernels (agx_lidar_image_obs, agx_reward_lidar_navigation,
agx_obs_lidar_navigation) and of the image kernel's device-noise rule.  It is the comparator of the GPU tests (the reference's code
does not exist where they run) and is itself pinned to the reference bit for bit by tests/test_lidar_navigation_task.py
(tests/golden/cr/*.npz: the reference's own code with correctly rounded elementary functions).

The reward and what the reward kernel derives from the env buffers are radar_ref's (`reward(..., radar=False)`, `reward_inputs`);
here are the observation, the image with its three noise rules, and the device draws.  Every array is float32 and every + - * / one
rounded float32 operation; the fused multiply-adds inside torch.norm are explicit (sim2real_ref.norm3).  The time to collision and
the Philox uniforms come from the CPU oracle as it stands (oracle.lidar_image_obs, oracle.rng_fill); the pooled ranges are restated
here and checked against the oracle's noise-free image on every call."""
import numpy as np
from radar_ref import quat_rotate_inverse, reward, reward_inputs  # noqa: F401  (the comparators of the reward kernel)
from sim2real_ref import F, f32, norm3, ssa

RNG_LIDAR_NOISE, RNG_OBS_NOISE = 5, 6  # agx_rng.h


def lidar_reward(pos_err, vveh, wbody, yaw_error, crashes, action, prev_action, ttc, curriculum_progress, rp):
    """compute_reward of lidar_navigation_task.py:554-719"""
    return reward(pos_err, vveh, wbody, yaw_error, crashes, action, prev_action, ttc, curriculum_progress, rp, radar=False)


def obs(position, qveh, euler, vbody, wbody, actions, target, target_yaw, u_vec, u_euler, downsampled):
    """process_obs_for_task (:440-470): [N, 17 + cells].  u_vec, u_euler: the two rand_like draws.  A target at the robot divides
    by a distance of 0 as the reference does (+-inf, NaN where the perturbed component is 0)."""
    v = quat_rotate_inverse(qveh, f32(target) - f32(position))
    dist = norm3(v)
    perturbed = v + F(0.2) * (f32(u_vec) - F(0.5))  # 0.1 * 2 * (rand_like - 0.5): the python product 0.2 first
    with np.errstate(divide="ignore", invalid="ignore"):
        unit = perturbed / dist[:, None]
    e = ssa(f32(euler))
    pe = e + F(0.1) * (f32(u_euler) - F(0.5))
    yaw_error = ssa(f32(target_yaw) - e[:, 2])
    n = len(dist)
    cols = [unit, dist[:, None], pe[:, 0:2], yaw_error[:, None], f32(vbody), f32(wbody), f32(actions), f32(downsampled).reshape(n, -1)]
    return np.ascontiguousarray(np.concatenate(cols, axis=1), np.float32)


def pooled_ranges(pointcloud, position, ph, pw):
    """process_image_observation (:313-347) up to the min-pool: ranges above 10 m and below 0.2 m read 10 m; rows and columns that
    do not fill a pool are dropped as max_pool2d drops them.  [N, H // ph, W // pw]"""
    pc = f32(pointcloud)
    n, H, W = pc.shape[0:3]
    oh, ow = H // ph, W // pw
    d = pc - f32(position)[:, None, None, :]
    r = norm3(d.reshape(-1, 3)).reshape(n, H, W)
    r = np.where(r > F(10.0), F(10.0), r)
    r = np.where(r < F(0.2), F(10.0), r).astype(np.float32)
    return r[:, : oh * ph, : ow * pw].reshape(n, oh, ph, ow, pw).min(axis=(2, 4))


def image_obs(orc, pointcloud, position, linvel, noise_mask=None, noise_val=None, max_mask=None, low_mask=None, low_val=None, ph=3,
              pw=6, low_row0=10):
    """process_image_observation (:313-363) + add_noise_to_downsampled_lidar_data (:286-310): pointcloud [N, H, W, 3] ->
    (time_to_collision [N], 1 / pooled range [N, cells]).  The five tensors are [N, cells] (or [N, oh, ow]) over the WHOLE pooled
    image; a mask counts where it is exactly 1.  In the reference's order: += noise_val where noise_mask, = 10 where max_mask,
    = low_val where low_mask on the pooled rows >= low_row0 -- a later rule wins."""
    pc = f32(pointcloud)
    n, oh, ow = pc.shape[0], pc.shape[1] // ph, pc.shape[2] // pw
    ttc, clean = orc.lidar_image_obs(pc, f32(position), f32(linvel), ph=ph, pw=pw, low_row0=low_row0)
    m = pooled_ranges(pc, position, ph, pw)
    assert np.array_equal((F(1.0) / m).reshape(n, -1), clean), "the pooled ranges restated here are not the oracle's"
    shape = lambda a: None if a is None else f32(a).reshape(n, oh, ow)  # noqa: E731
    noise_mask, noise_val, max_mask, low_mask, low_val = (shape(a) for a in (noise_mask, noise_val, max_mask, low_mask, low_val))
    if noise_mask is not None:
        m = np.where(noise_mask == 1, m + noise_val, m)
    if max_mask is not None:
        m = np.where(max_mask == 1, F(10.0), m)
    if low_mask is not None:
        low_rows = (np.arange(oh) >= low_row0)[None, :, None]
        m = np.where((low_mask == 1) & low_rows, low_val, m)
    return ttc, (F(1.0) / m.astype(np.float32)).reshape(n, oh * ow)


def device_noise(orc, seed, steps, cells, ow, low_row0):
    """the five tensors k_lidar_image_obs draws for envs 0 .. len(steps) - 1 (env i in its env step steps[i]): stream
    RNG_LIDAR_NOISE, eight uniforms per pooled cell c from the blocks 2c and 2c + 1 -> u0 < 0.03: noise of 9.8 u1 + 0.2;
    u2 < 0.02: max range; u3 < 0.02 on the pooled rows >= low_row0: the low value 0.8 u4 + 0.2.  [N, cells] each."""
    u = orc.rng_fill(seed, np.asarray(steps), RNG_LIDAR_NOISE, 8 * cells).reshape(len(steps), cells, 8)
    noise_mask = (u[..., 0] < F(0.03)).astype(np.float32)
    noise_val = ((F(10.0) - F(0.2)) * u[..., 1] + F(0.2)).astype(np.float32)
    max_mask = (u[..., 2] < F(0.02)).astype(np.float32)
    low_rows = (np.arange(cells) // ow >= low_row0)[None, :]
    low_mask = ((u[..., 3] < F(0.02)) & low_rows).astype(np.float32)
    low_val = ((F(1.0) - F(0.2)) * u[..., 4] + F(0.2)).astype(np.float32)
    return noise_mask, noise_val, max_mask, low_mask, low_val


def obs_draws(orc, seed, steps):
    """the six uniforms k_obs_lidar_navigation draws per env (stream RNG_OBS_NOISE): (u_vec [N, 3], u_euler [N, 3])"""
    u = orc.rng_fill(seed, np.asarray(steps), RNG_OBS_NOISE, 6)
    return np.ascontiguousarray(u[:, 0:3]), np.ascontiguousarray(u[:, 3:6])
