"""Times the VAE depth-image encoder of the navigation task: agx_vae_encode alone, navigation_task.step with vae_config.use_vae on
and off, and the same encoder evaluated by torch.nn.functional.conv2d on the same device (how the reference runs it), at 256 and
1024 envs.

    python profiles/vae_encoder_probe.py [--envs 256 1024] [--precision fp32 bf16] [--steps 20] [--warmup 3] [--repeats 5]
                                         [--out profiles/vae_encoder_probe.json]

Weights are random (the trained file is not shipped; time does not depend on the values).  Every time is a host clock around
`steps` calls that end in a device synchronise, best of `repeats`.  The arithmetic floor is 0.716 GFLOP per image at the 157 TFLOP/s
fp32 matrix peak (4.6 us per image); `fraction_of_fp32_matrix_peak` is that floor over the measured time per image.  The bf16
path (vae_config.precision = "bf16") is timed in the same run against its own two floors, derived and not measured: the same FLOPs
at the 2.5 PFLOP/s bf16 matrix peak (0.29 us per image) and 7.3 MB per image of bf16 activation traffic at 8 TB/s (0.9 us)."""
import argparse
import json
import math
import os
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FLOP_PER_IMAGE, PEAK_FLOPS = 0.716e9, 157e12
BF16_PEAK_FLOPS, BF16_BYTES_PER_IMAGE, HBM_BYTES_PER_S = 2.5e15, 7.3e6, 8e12


def random_state_dict(torch):
    from aerial_gym_simulator_amd.utils.vae.vae_image_encoder import expected_shapes

    g = torch.Generator().manual_seed(1)
    sd = {}
    for key, shape in expected_shapes().items():
        fan_in = max(1, int(math.prod(shape[1:])))
        sd[key] = ((torch.rand(shape, generator=g) * 2 - 1) * (1.7 / math.sqrt(fan_in))).float()
    return sd


def torch_encoder(torch, sd, dev):
    """the reference's forward pass (VAE.py ImgEncoder.encode + the sampling) as torch.nn.functional calls"""
    F = torch.nn.functional
    from aerial_gym_simulator_amd.utils.vae.vae_image_encoder import CONV_LAYERS

    p = {k: v.to(dev) for k, v in sd.items()}

    def c(n, x):
        return F.conv2d(x, p[f"encoder.{n}.weight"], p[f"encoder.{n}.bias"], stride=CONV_LAYERS[n][3], padding=CONV_LAYERS[n][4])

    def run(images, res):
        with torch.no_grad():
            x = F.interpolate(images.unsqueeze(1), res, mode="nearest") if tuple(images.shape[-2:]) != tuple(res) else images.unsqueeze(1)
            x01 = F.elu(c("conv0_1", c("conv0", x)))
            x11 = F.elu(c("conv1_1", c("conv1_0", x01)) + c("conv0_jump_2", x01))
            x21 = F.elu(c("conv2_1", c("conv2_0", x11)) + c("conv1_jump_3", x11))
            d0 = F.elu(F.linear(c("conv3_0", x21).flatten(1), p["encoder.dense0.weight"], p["encoder.dense0.bias"]))
            z = F.linear(d0, p["encoder.dense1.weight"], p["encoder.dense1.bias"])
            std = torch.exp(0.5 * z[:, 64:])
            return z[:, :64] + torch.randn_like(std) * std

    return run


def timed(torch, fn, steps, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / steps)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precision", nargs="+", default=["fp32", "bf16"], choices=["fp32", "bf16"])
    ap.add_argument("--no-task", action="store_true", help="skip navigation_task.step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_encoder_probe.json"))
    a = ap.parse_args()
    import torch

    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd.config.task_config import navigation_task_config as cfg
    from aerial_gym_simulator_amd.registry.task_registry import task_registry
    from aerial_gym_simulator_amd.utils.vae.vae_image_encoder import VAEImageEncoder

    if not torch.cuda.is_available():
        raise SystemExit("vae_encoder_probe needs a HIP device: a time taken anywhere else says nothing")
    dev = "cuda:0"
    sd = random_state_dict(torch)
    folder = tempfile.mkdtemp(prefix="vae_probe_")
    torch.save(sd, os.path.join(folder, "w.pth"))
    encoders = {}
    for precision in a.precision:
        vcfg = types.SimpleNamespace(latent_dims=64, model_folder=folder, model_file="w.pth", image_res=(270, 480), interpolation_mode="nearest",
                                     return_sampled_latent=True, precision=precision)
        encoders[precision] = VAEImageEncoder(vcfg, device=dev)
    reference = torch_encoder(torch, sd, dev)
    rows = []
    for n in a.envs:
        px = torch.rand((n, 48, 64), device=dev) * 10.0
        row = {"num_envs": n, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
        for precision, enc in encoders.items():
            t = timed(torch, lambda: enc.encode(px), a.steps, a.warmup, a.repeats)
            if precision == "fp32":
                row["envs_per_chunk"] = enc.envs_per_chunk(n)
                row["agx_vae_encode_ms"] = round(t * 1e3, 3)
                row["us_per_image"] = round(t / n * 1e6, 2)
                row["fraction_of_fp32_matrix_peak"] = round(FLOP_PER_IMAGE / PEAK_FLOPS / (t / n), 4)
            else:
                row["bf16_envs_per_chunk"] = enc.envs_per_chunk(n)
                row["bf16_agx_vae_encode_ms"] = round(t * 1e3, 3)
                row["bf16_us_per_image"] = round(t / n * 1e6, 2)
                row["bf16_fraction_of_matrix_floor"] = round(FLOP_PER_IMAGE / BF16_PEAK_FLOPS / (t / n), 4)
                row["bf16_fraction_of_traffic_floor"] = round(BF16_BYTES_PER_IMAGE / HBM_BYTES_PER_S / (t / n), 4)
        t = timed(torch, lambda: reference(px, (270, 480)), a.steps, a.warmup, a.repeats)
        row["torch_conv2d_ms"] = round(t * 1e3, 3)
        if not a.no_task:
            for use_vae, precision in [(False, "fp32")] + [(True, p) for p in a.precision]:
                old = (cfg.vae_config.use_vae, cfg.vae_config.model_folder, cfg.vae_config.model_file, cfg.device, cfg.vae_config.precision)
                cfg.vae_config.use_vae, cfg.vae_config.model_folder, cfg.vae_config.model_file, cfg.device = use_vae, folder, "w.pth", dev
                cfg.vae_config.precision = precision
                try:
                    task = task_registry.make_task("navigation_task", seed=1, num_envs=n, headless=True)
                    task.reset()
                    act = torch.zeros((n, 4), device=dev)
                    t = timed(torch, lambda: task.step(act), a.steps, a.warmup, a.repeats)
                    key = "navigation_step_ms_vae_off" if not use_vae else ("navigation_step_ms_vae_on" if precision == "fp32" else "navigation_step_ms_vae_on_bf16")
                    row[key] = round(t * 1e3, 3)
                    task.close()
                    del task
                finally:
                    cfg.vae_config.use_vae, cfg.vae_config.model_folder, cfg.vae_config.model_file, cfg.device, cfg.vae_config.precision = old
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = {"rows": rows, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "source_image": [48, 64], "image_res": [270, 480],
              "flop_per_image": FLOP_PER_IMAGE, "fp32_matrix_peak_flops": PEAK_FLOPS, "bf16_matrix_peak_flops": BF16_PEAK_FLOPS,
              "bf16_activation_bytes_per_image": BF16_BYTES_PER_IMAGE, "hbm_bytes_per_s": HBM_BYTES_PER_S, "device": torch.cuda.get_device_name(0),
              "build_id": _lib.build_id()}
    with open(a.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
