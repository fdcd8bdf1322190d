"""TEST INFRASTRUCTURE -- golden vectors of the radar navigation task, produced by running the REFERENCE's own code (needs the
reference tree, ref_shells.REFERENCE_ROOT; uses the helpers under oracle/ by path).

    python tests/golden_gen/gen_golden_radar_nav.py [--cr] [--out DIR]

writes, into tests/golden/ (tests/golden/radar_cr/ with --cr: the same code with correctly rounded elementary functions,
oracle/cr_torch.py):

  radar_reward.npz     n = 768: inputs and outputs of radar_navigation_task.compute_reward (:179-342); vehicle-frame x velocities of
                       both signs, distances on both sides of 1 m and 3 m, some crashes; `reward_lidar_formula` is what the LiDAR
                       task's compute_reward returns on the same inputs (at least 200 rows differ: the one clamp, :242-246)
  radar_image_obs.npz  6 envs x 48 x 120: RadarNavigationTask.process_image_observation (:24-63) without and with
                       add_noise_to_downsampled_lidar_data (:6-21), called as unbound methods on a stand-in object; the three random
                       tensors the noise function draws are re-drawn from the same seed and stored next to the outputs.  The seed is
                       the first one for which >= 5 cells have noise and stay valid, >= 20 have noise and are invalidated, and the
                       invalid share lies within 0.8 +- 0.05 (expected out of 1920 cells: about 11, 46 and 1536)
  radar_config.npz     the values of the three reference configs (radar_navigation_task_config.py, lmf2_radar_config.py,
                       fake_radar_config.py) as JSON
"""
import json
import math
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg  # noqa: E402  FIRST: it switches TorchScript off before torch is imported (cr_torch.py)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_shells  # noqa: E402

OUT = (sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
       else os.path.join(ROOT, "tests", "golden", *(["radar_cr"] if gg.CR else [])))
N_IMG, H, W, OH, OW = 6, 48, 120, 16, 20


def reward_keys(cfg):
    return list(cfg.reward_parameters.keys())


def gen_reward(rng, rt, lt, cfg):
    n = 768
    pe = torch.randn(n, 3, generator=rng) * 3
    pe[: n // 6] *= 0.15  # inside the 1 m "stable at goal" radius
    prev = pe + torch.randn(n, 3, generator=rng) * 0.1
    vveh = torch.randn(n, 3, generator=rng) * 1.5
    vveh[::7] *= 3.0  # beyond the 3 m/s penalty knee
    wbody = torch.randn(n, 3, generator=rng)
    yaw_err = (torch.rand(n, generator=rng) - 0.5) * 2 * math.pi
    crashes = torch.rand(n, generator=rng) < 0.1
    act = (torch.rand(n, 4, generator=rng) - 0.5) * 4
    pact = (torch.rand(n, 4, generator=rng) - 0.5) * 4
    ttc = torch.rand(n, generator=rng) * 3
    ttc[::5] = 10.0
    cpf = 0.35
    keys = reward_keys(cfg)
    pdct = {k: torch.tensor(float(cfg.reward_parameters[k])) for k in keys}
    args = (pe, prev, vveh, wbody, yaw_err, crashes.clone(), act, pact, ttc, cpf, pdct)
    r, c = rt.compute_reward(*args)
    r_lidar, _ = lt.compute_reward(*[a.clone() if isinstance(a, torch.Tensor) else a for a in args])
    dist = pe.norm(dim=1)
    differ = int((r != r_lidar).sum())
    assert differ >= 200, differ
    assert int((vveh[:, 0] > 0).sum()) >= 200 and int((vveh[:, 0] < 0).sum()) >= 200
    assert min(int((dist < 1).sum()), int(((dist > 1) & (dist < 3)).sum()), int((dist > 3).sum())) >= 50
    assert 30 <= int(crashes.sum()) <= 150 and torch.equal(c, crashes)
    np.savez(os.path.join(OUT, "radar_reward.npz"), pos_err=pe.numpy(), prev_pos_err=prev.numpy(), vveh=vveh.numpy(),
             wbody=wbody.numpy(), yaw_error=yaw_err.numpy(), crashes=crashes.numpy(), action=act.numpy(), prev_action=pact.numpy(),
             time_to_collision=ttc.numpy(), curriculum_progress=np.float32(cpf),
             rp=np.array([float(cfg.reward_parameters[k]) for k in keys], np.float32), reward=r.numpy(), reward_lidar_formula=r_lidar.numpy())
    print("radar_reward: ok  mean %.5f  rows that differ from the LiDAR formula: %d  crashes: %d" % (float(r.mean()), differ, int(crashes.sum())))


def draw_noise(m, seed):
    """what add_noise_to_downsampled_lidar_data draws (:6-21), same seed, same call order"""
    torch.manual_seed(seed)
    z = torch.zeros(N_IMG, OH, OW)
    noise_mask = torch.bernoulli(0.03 * torch.ones_like(z))
    k = int((noise_mask == 1).sum())
    flat = m.torch_rand_float_tensor(0.2 * torch.ones(k), 10.0 * torch.ones(k))
    noise_val = torch.zeros_like(z)
    noise_val[noise_mask == 1] = flat
    invalid_mask = torch.bernoulli(0.8 * torch.ones_like(z))
    return noise_mask, noise_val, invalid_mask


def noise_counts(noise_mask, invalid_mask):
    nm, im = noise_mask == 1, invalid_mask == 1
    return int((nm & ~im).sum()), int((nm & im).sum()), float(im.float().mean())


def counts_ok(counts):
    return counts[0] >= 5 and counts[1] >= 20 and abs(counts[2] - 0.8) <= 0.05


def gen_image_obs(rng, rt):
    n = N_IMG
    m = ref_shells.ref("utils.math")
    pos = (torch.rand(n, 3, generator=rng) - 0.5) * 4
    # a world-frame point cloud as the sensor writes it: hits at 0.05 .. 12 m, misses at 1000 m along the ray
    dirs = torch.randn(n, H, W, 3, generator=rng)
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    rng_img = torch.rand(n, H, W, generator=rng) * 12 + 0.05
    rng_img[torch.rand(n, H, W, generator=rng) < 0.15] = 1000.0
    pc = (pos[:, None, None, :] + dirs * rng_img[..., None]).unsqueeze(1).contiguous()
    linvel = torch.randn(n, 3, generator=rng) * 2
    linvel[0] = 0.0
    seed = next(s for s in range(1000) if counts_ok(noise_counts(*draw_noise(m, s)[0::2])))
    out = {}
    for tag, sd in (("clean", None), ("noisy", seed)):
        fake = types.SimpleNamespace(
            obs_dict={"depth_range_pixels": pc.clone(), "robot_position": pos.clone(), "robot_linvel": linvel.clone()},
            world_dir_vectors=torch.ones(n, H, W, 3), num_envs=n, time_to_collision=torch.zeros(n),
            downsampled_lidar_data=torch.zeros(n, OH * OW), device="cpu")
        if sd is None:
            fake.add_noise_to_downsampled_lidar_data = lambda x: x
        else:
            fake.add_noise_to_downsampled_lidar_data = types.MethodType(rt.RadarNavigationTask.add_noise_to_downsampled_lidar_data, fake)
            torch.manual_seed(sd)
        rt.RadarNavigationTask.process_image_observation(fake)
        out[tag + "_ttc"] = fake.time_to_collision.numpy().copy()
        out[tag + "_ds"] = fake.downsampled_lidar_data.numpy().copy()
    noise_mask, noise_val, invalid_mask = draw_noise(m, seed)
    counts = noise_counts(noise_mask, invalid_mask)
    assert counts_ok(counts), counts
    ds = out["noisy_ds"].reshape(n, OH, OW)
    assert ((ds == -1.0) == (invalid_mask.numpy() == 1)).all()  # the stored draws are the ones the function made
    assert (ds[(noise_mask.numpy() == 1) & (invalid_mask.numpy() == 0)] != out["clean_ds"].reshape(n, OH, OW)[(noise_mask.numpy() == 1) & (invalid_mask.numpy() == 0)]).all()
    np.savez(os.path.join(OUT, "radar_image_obs.npz"), pointcloud=pc.numpy(), robot_position=pos.numpy(), robot_linvel=linvel.numpy(),
             noise_mask=noise_mask.numpy(), noise_val=noise_val.numpy(), invalid_mask=invalid_mask.numpy(), noise_seed=np.int64(seed), **out)
    print("radar_image_obs: ok  seed %d  noise and valid / noise and invalid / invalid share: %d / %d / %.4f  ttc" % ((seed,) + counts), out["clean_ttc"])


def config_values(cls):
    """the class's own attributes (not the inherited ones) as JSON-able values; nested classes recursively, other classes by name"""
    out = {}
    for k, v in vars(cls).items():
        if k.startswith("__") or callable(v) and not isinstance(v, type):
            continue
        if isinstance(v, type):
            out[k] = config_values(v) if v.__qualname__.startswith(cls.__qualname__ + ".") else {"class": v.__name__}
        elif isinstance(v, str):
            out[k] = v.replace(ref_shells.REFERENCE_ROOT, "")  # (file names relative to the reference's root)
        elif isinstance(v, (bool, int, float, list, tuple, dict, type(None))):
            out[k] = v
    return out


def gen_config(cfg):
    robot = ref_shells.ref("config.robot_config.lmf2_radar_config").LMF2RadarCfg
    sensor = ref_shells.ref("config.sensor_config.lidar_config.fake_radar_config").fake_radar_config
    assert robot.sensor_config.lidar_config is sensor
    cfg.device = "cpu"
    ain = torch.tensor([[-3.0, -1.0, 0.25, 7.0], [0.5, -0.25, 1.0, -0.75]])
    aout = cfg.action_transformation_function(ain.clone())
    cfg.device = "cuda:0"
    rec = dict(task=config_values(cfg), robot=config_values(robot), sensor=config_values(sensor))
    np.savez(os.path.join(OUT, "radar_config.npz"), config=np.array(json.dumps(rec, sort_keys=True)), action_transform_in=ain.numpy(),
             action_transform_out=aout.numpy())
    print("radar_config:", json.dumps(rec["task"], sort_keys=True)[:200], "...")


def main():
    os.makedirs(OUT, exist_ok=True)
    ref_shells.install()
    ref_shells.install_task_shells()
    lt = ref_shells.ref("task.lidar_navigation_task.lidar_navigation_task")
    rt = ref_shells.ref("task.radar_navigation_task.radar_navigation_task")
    assert issubclass(rt.RadarNavigationTask, lt.LiDARNavigationTask)
    cfg = ref_shells.ref("config.task_config.radar_navigation_task_config").task_config
    rng = torch.Generator().manual_seed(6060)
    gen_reward(rng, rt, lt, cfg)
    gen_image_obs(rng, rt)
    gen_config(cfg)


if __name__ == "__main__":
    main()
