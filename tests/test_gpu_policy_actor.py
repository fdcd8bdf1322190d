"""GPU: the fused policy actor (csrc/agx_policy.hip, one launch per call) against

1. the chain of agx_vae_linear calls it restates, bit for bit, over nets, batch sizes and activations that reach every tile edge,
   every number of channel tiles a wave can hold, the k padding and the LDS maximum;
2. float64 on exact-arithmetic inputs, bit for bit: independent of the VAE kernel;
3. float64 on the reference's trained actors within the propagated order-independent bound (policy_ref.mlp64);
4.-8. invariance to batch and position, input normalisation, sampling and the device generator, no allocation, refusals;
9. the closed loop: the reference's trained actors fly the simulator through ActorMLP and through MLP(...).

Measured (MI355X): fused == chain in every case; max |err| / propagated bound 0.0007 (attitude), 0.0002 (both lmf2 actors);
closed-loop figures in the docstrings of the closed-loop tests."""
import ctypes as C

import numpy as np
import policy_ref
import pytest
import torch
import vae_ref
from policy_ref import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = (1, 31, 32, 33, 65, 129, 1057)  # the tile edges, and more than one workgroup
ACTIVATIONS = ("none", "elu", "relu")
RANDOM_NETS = {
    "13-32-1": [13, 32, 1], "17-64-33": [17, 64, 33], "81-256-128-64-4": [81, 256, 128, 64, 4], "15-512-512-4": [15, 512, 512, 4],
    "eight-layers-of-32": [19] + [32] * 7 + [5], "single-layer-13-4": [13, 4], "96-three-tiles": [9, 96, 3], "in-1": [1, 32, 4],
    "in-7": [7, 32, 4], "in-8": [8, 32, 4], "in-9": [9, 32, 4], "in-512": [512, 64, 4], "out-512": [24, 32, 512],
}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _L():
    from aerial_gym_simulator_amd import _lib

    return _lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _actor(ws, bs, **kw):
    from aerial_gym_simulator_amd.utils.policy import ActorMLP

    return ActorMLP.from_arrays(ws, bs, device=DEV, **kw)


class Chain:
    """the net as agx_vae_linear calls, layer by layer: the last layer padded to a multiple of 32 zero rows"""

    def __init__(self, ws, bs):
        from aerial_gym_simulator_amd.utils.policy import pack_layer

        self.out = ws[-1].shape[0]
        self.layers = []
        for l, (w, b) in enumerate(zip(ws, bs)):
            rows = -(-w.shape[0] // 32) * 32 if l + 1 == len(ws) else w.shape[0]
            bias = np.zeros(rows, np.float32)
            bias[:w.shape[0]] = b
            self.layers.append((torch.from_numpy(pack_layer(w, pad_rows_to=rows)).to(DEV), torch.from_numpy(bias).to(DEV), w.shape[1], rows))

    def __call__(self, x, activation):
        L = _L()
        lib = L.load()
        n = x.shape[0]
        for l, (wp, bias, fin, rows) in enumerate(self.layers):
            hidden = l + 1 < len(self.layers)
            y = torch.full((n, rows), float("nan"), device=DEV)
            L.check(lib.agx_vae_linear(n, L.dptr(x), L.dptr(wp), L.dptr(bias), L.dptr(y), fin, rows, L.VAE_ELU if hidden and activation == "elu" else 0,
                                       _stream()), "agx_vae_linear")
            if hidden and activation == "relu":
                y = torch.where(y < 0, torch.zeros_like(y), y)
            x = y
        return x[:, :self.out].contiguous()


def _net(name):
    if name in policy_ref.REAL_NETS:
        ws, bs, _ = policy_ref.load_actor(name)
        return ws, bs
    return policy_ref.random_net(RANDOM_NETS[name], _gen(1000 + sorted(RANDOM_NETS).index(name)), scale=2.0)


@pytest.mark.parametrize("name", list(policy_ref.REAL_NETS) + list(RANDOM_NETS))
def test_fused_equals_the_layer_chain_bit_for_bit(name):
    ws, bs = _net(name)
    chain = Chain(ws, bs)
    g = _gen(7)
    ranges = (1.0, 10.0) if name in policy_ref.REAL_NETS else (2.0,)
    for activation in ACTIVATIONS:
        actor = _actor(ws, bs, activation=activation)
        for span in ranges:
            for n in BATCHES:
                obs = ((torch.rand((n, actor.obs_dim), generator=g) * 2 - 1) * span).to(DEV)
                out = torch.full((n, actor.action_dim), float("nan"), device=DEV)
                got = actor(obs, out=out)
                want = chain(obs, activation)
                torch.cuda.synchronize()
                assert got is out and torch.isfinite(want).all()
                assert np.array_equal(bits(got), bits(want)), (name, activation, span, n, float((got - want).abs().max()))
                assert np.array_equal(bits(actor.mean), bits(want))


def test_a_smaller_actor_created_later_does_not_disturb_a_larger_one():
    """131072 bytes of LDS, then an actor of 73728 bytes (both above 64 KiB: the kernel's dynamic-LDS attribute matters to both),
    then the small one and the large one are called: the twin of the test of that name in test_gpu_recurrent_policy.py.  Measured
    (MI355X, ROCm 7.2): also passes when create sets the attribute to the actor's own size, as it did before it set the limit"""
    (big_ws, big_bs), (small_ws, small_bs) = _net("15-512-512-4"), _net("in-512")
    big = _actor(big_ws, big_bs)
    small = _actor(small_ws, small_bs)
    assert big.lds_bytes == 131072 and small.lds_bytes == 73728
    g = _gen(8)
    obs = (torch.rand((33, 15), generator=g) * 4 - 2).to(DEV)
    small((torch.rand((33, 512), generator=g) * 4 - 2).to(DEV))
    got = big(obs)
    want = Chain(big_ws, big_bs)(obs, "elu")
    torch.cuda.synchronize()
    assert torch.isfinite(want).all() and np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("n", [1, 33, 129])
def test_exact_inputs_equal_float64_bit_for_bit(n):
    """13 -> 32 -> 4, ReLU; weights and biases on the 1/8 grid, inputs on the 1/16 grid, all in [-1, 1].  Layer 1: products are
    multiples of 1/128, |partial sums| <= 13 + 1 = 14; layer 2: its inputs are multiples of 1/128 up to 14, products multiples of
    1/1024, |partial sums| <= 32 * 14 + 1 = 449 < 2^24 / 1024.  Every partial sum is a float32: any order gives float64's result."""
    g = _gen(20 + n)
    ws = [vae_ref.exact_grid((32, 13), 1 / 8, g).numpy(), vae_ref.exact_grid((4, 32), 1 / 8, g).numpy()]
    bs = [vae_ref.exact_grid((32,), 1 / 8, g).numpy(), vae_ref.exact_grid((4,), 1 / 8, g).numpy()]
    x = vae_ref.exact_grid((n, 13), 1 / 16, g)
    ref, _err, pres = policy_ref.mlp64(ws, bs, x, "relu")
    # the premise
    assert float(pres[0].abs().max()) <= 14 and torch.equal(pres[0] * 128, (pres[0] * 128).round())
    assert float(pres[1].abs().max()) <= 449 and torch.equal(pres[1] * 1024, (pres[1] * 1024).round())
    assert all(torch.equal(p.float().double(), p) for p in pres)
    assert (pres[0] < 0).any() and (pres[0] > 0).any()
    got = _actor(ws, bs, activation="relu")(x.to(DEV))
    torch.cuda.synchronize()
    assert np.array_equal(bits(got), bits(ref.float())), float((got.cpu().double() - ref).abs().max())


@pytest.mark.parametrize("name", policy_ref.REAL_NETS)
def test_real_nets_within_the_propagated_bound(name):
    ws, bs, _ = policy_ref.load_actor(name)
    actor = _actor(ws, bs)
    g = _gen(30)
    worst = 0.0
    for span in (1.0, 10.0):
        x = (torch.rand((257, actor.obs_dim), generator=g) * 2 - 1) * span
        ref, bound, _ = policy_ref.mlp64(ws, bs, x, "elu")
        got = actor(x.to(DEV)).cpu().double()
        assert float(bound.min()) > 0
        worst = max(worst, float(((got - ref).abs() / bound).max()))
    print(f"{name}: max |err| / bound = {worst:.4f}")
    assert worst <= 1.0, (name, worst)


def test_an_env_has_the_same_bits_wherever_it_is_evaluated():
    ws, bs, _ = policy_ref.load_actor("lmf2_acceleration")
    actor = _actor(ws, bs)
    g = _gen(40)
    batch = (torch.rand((1057, 17), generator=g) * 6 - 3).to(DEV)
    full = actor(batch).clone()
    for row in (0, 31, 32, 500, 1056):
        alone = actor(batch[row:row + 1].contiguous()).clone()
        assert np.array_equal(bits(alone[0]), bits(full[row])), row
    moved = batch.clone()
    moved[0], moved[1056] = batch[1056], batch[0]
    swapped = actor(moved).clone()
    assert np.array_equal(bits(swapped[0]), bits(full[1056])) and np.array_equal(bits(swapped[1056]), bits(full[0]))
    perm = torch.randperm(1057, generator=g).to(DEV)
    permuted = actor(batch[perm].contiguous()).clone()
    assert np.array_equal(bits(permuted), bits(full[perm]))


def test_input_normalisation_is_the_float32_formula():
    ws, bs, _ = policy_ref.load_actor("lmf2_velocity")
    g = _gen(50)
    mean, denom = (torch.randn(17, generator=g) * 2).numpy(), (torch.rand(17, generator=g) * 2 + 0.05).numpy()
    obs = torch.rand((129, 17), generator=g) * 40 - 20
    xn = policy_ref.norm_f32(obs.numpy(), mean, denom, 5.0)
    assert (xn == 5.0).any() and (xn == -5.0).any() and (np.abs(xn) < 5.0).any()  # beyond the clip on both sides, and inside
    want = Chain(ws, bs)(torch.from_numpy(xn).to(DEV), "elu")
    got = _actor(ws, bs, input_norm=(mean, denom, 5.0))(obs.to(DEV))
    torch.cuda.synchronize()
    assert np.array_equal(bits(got), bits(want))
    assert not np.array_equal(bits(_actor(ws, bs)(obs.to(DEV))), bits(want))


def test_sampling_from_given_normals():
    ws, bs, logstd = policy_ref.load_actor("attitude")
    logstd = (logstd + np.linspace(-1.0, 1.5, 4).astype(np.float32)).astype(np.float32)  # four different sigmas, some above 1
    actor = _actor(ws, bs, logstd=logstd)
    g = _gen(60)
    obs = (torch.rand((161, 13), generator=g) * 4 - 2).to(DEV)
    eps = torch.randn((161, 4), generator=g)
    mu = actor(obs).clone().cpu().numpy()
    for clamp in (False, True):
        got = actor(obs, sample=True, clamp=clamp, eps=eps.to(DEV))
        want = policy_ref.sample_f32(mu, eps.numpy(), logstd, clamp)
        assert np.array_equal(bits(got), bits(want)), clamp
        assert np.array_equal(bits(actor.mean), bits(mu))  # mu_out: the mean before sampling and clamping
    assert (np.abs(policy_ref.sample_f32(mu, eps.numpy(), logstd)) > 1).any()
    assert np.array_equal(bits(actor(obs, clamp=True)), bits(np.clip(mu, np.float32(-1), np.float32(1))))


def test_sampling_from_the_device_generator():
    ws, bs, logstd = policy_ref.load_actor("attitude")
    actor = _actor(ws, bs, logstd=logstd, rng_seed=1234, env_index_base=0)
    g = _gen(70)
    n = 200
    obs = (torch.rand((n, 13), generator=g) * 4 - 2).to(DEV)
    mu = actor(obs).clone().cpu().numpy()
    noise = actor.noise(n, step=5).cpu().numpy()
    got = actor(obs, sample=True, step=5)
    assert np.array_equal(bits(got), bits(policy_ref.sample_f32(mu, noise, logstd)))
    assert np.array_equal(bits(actor.mean), bits(mu))
    # a function of (seed, global env index, step, action) alone
    actor.env_index_base = 37
    shifted = actor.noise(n, step=5).cpu().numpy()
    actor.env_index_base = 0
    assert np.array_equal(bits(shifted), bits(actor.noise(n + 37, step=5).cpu().numpy()[37:]))
    assert np.array_equal(bits(noise[:1]), bits(actor.noise(1, step=5).cpu().numpy()))
    assert not np.array_equal(noise, actor.noise(n, step=6).cpu().numpy())
    other = _actor(ws, bs, logstd=logstd, rng_seed=1235, env_index_base=0)
    assert not np.array_equal(noise, other.noise(n, step=5).cpu().numpy())
    # without step= and without a task the object counts its sampled calls
    assert actor.step == 0
    first = actor(obs, sample=True).clone()
    second = actor(obs, sample=True).clone()
    assert actor.step == 2 and np.array_equal(bits(first), bits(policy_ref.sample_f32(mu, actor.noise(n, step=0).cpu().numpy(), logstd)))
    assert not np.array_equal(bits(first), bits(second))
    # standard normals: 65536 envs x 4 actions, mean and variance within five standard errors
    z = actor.noise(65536, step=9).cpu().numpy().astype(np.float64)
    count = z.size
    assert count == 262144 and np.isfinite(z).all()
    assert abs(z.mean()) < 5.0 / np.sqrt(count), z.mean()
    assert abs(z.var() - 1.0) < 5.0 * np.sqrt(2.0 / count), z.var()
    for j in range(4):  # and per action column
        assert abs(z[:, j].mean()) < 5.0 / np.sqrt(65536) and abs(z[:, j].var() - 1.0) < 5.0 * np.sqrt(2.0 / 65536), j


def test_calls_allocate_nothing_and_run_on_the_current_stream():
    ws, bs, logstd = policy_ref.load_actor("attitude")
    actor = _actor(ws, bs, logstd=logstd)
    g = _gen(80)
    obs = (torch.rand((1057, 13), generator=g) * 4 - 2).to(DEV)
    want = actor(obs, sample=True, clamp=True, step=3).clone()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for _ in range(100):
        out = actor(obs, sample=True, clamp=True, step=3)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert np.array_equal(bits(out), bits(want))
    # a side stream: the observations are written by work queued on that stream right before the call
    host = (torch.rand((1057, 13), generator=g) * 4 - 2)
    ref = actor(host.to(DEV)).clone()
    staging, result = torch.zeros((1057, 13), device=DEV), torch.zeros((1057, 4), device=DEV)
    pinned = host.pin_memory()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(20):  # work in front of the call on the same stream
            staging.copy_(pinned, non_blocking=True).mul_(1.0)
        actor(staging, out=result)
    side.synchronize()
    assert np.array_equal(bits(result), bits(ref))


def test_refusals_and_the_empty_batch():
    L = _L()
    lib = L.load()
    ws, bs, logstd = policy_ref.load_actor("attitude")
    actor = _actor(ws, bs)  # no logstd
    obs = torch.zeros((4, 13), device=DEV)
    out = torch.full((4, 4), 7.0, device=DEV)
    h = actor._handle
    assert lib.agx_policy_act(h, 0, None, None, None, None, 0, 0, 0, 0, _stream()) == 0  # nothing to do
    assert lib.agx_policy_act(h, 0, L.dptr(obs), L.dptr(out), None, None, 0, 0, 0, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert lib.agx_policy_act(h, 4, L.dptr(obs), L.dptr(out), None, None, L.POLICY_SAMPLE, 0, 0, 0, _stream()) == -1
    assert "logstd" in lib.agx_last_error().decode()
    assert lib.agx_policy_act(h, 4, None, L.dptr(out), None, None, 0, 0, 0, 0, _stream()) == -1
    assert "null obs" in lib.agx_last_error().decode()
    assert lib.agx_policy_act(h, 4, L.dptr(obs), None, None, None, 0, 0, 0, 0, _stream()) == -1
    assert "null actions" in lib.agx_last_error().decode()
    assert lib.agx_policy_act(h, 4, L.dptr(obs), L.dptr(out), None, None, 4, 0, 0, 0, _stream()) == -1
    assert "flags" in lib.agx_last_error().decode()
    assert lib.agx_policy_act(h, -1, L.dptr(obs), L.dptr(out), None, None, 0, 0, 0, 0, _stream()) == -1
    assert "num_envs = -1" in lib.agx_last_error().decode()
    assert lib.agx_policy_act(None, 4, L.dptr(obs), L.dptr(out), None, None, 0, 0, 0, 0, _stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # no refused call wrote anything
    # create refuses what the limits exclude, before it touches the device
    handle = C.c_void_p()
    w = np.zeros((48, 13), np.float32)
    wp, bp = (C.c_void_p * 2)(w.ctypes.data, w.ctypes.data), (C.c_void_p * 2)(w.ctypes.data, w.ctypes.data)
    assert lib.agx_policy_create(2, (C.c_int32 * 3)(13, 48, 4), wp, bp, L.POLICY_ELU, C.byref(handle)) == -1 and not handle.value
    assert "48" in lib.agx_last_error().decode()
    assert lib.agx_policy_create(2, (C.c_int32 * 3)(13, 32, 4), wp, bp, 3, C.byref(handle)) == -1 and not handle.value
    assert "hidden_activation = 3" in lib.agx_last_error().decode()
    with pytest.raises(ValueError, match="logstd"):
        actor(obs, sample=True)
    with pytest.raises(ValueError, match=r"float32 \[N, 13\]"):
        actor(torch.zeros((4, 12), device=DEV))
    with pytest.raises(RuntimeError, match="HIP device"):
        actor(torch.zeros((4, 13)))


# ---- the closed loop ------------------------------------------------------------------------------------------------------------
def fly_attitude(sample, n=512, steps=510):
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config.task_config import position_setpoint_task_config as cfg
    from aerial_gym_simulator_amd.registry.task_registry import task_registry
    from aerial_gym_simulator_amd.utils.policy import ActorMLP

    old = (cfg.controller_name, cfg.episode_len_steps, cfg.args, cfg.robot_name)
    cfg.device, cfg.controller_name, cfg.robot_name, cfg.episode_len_steps, cfg.args = DEV, "lee_attitude_control", "base_quadrotor", 500, {}
    try:
        ws, bs, logstd = policy_ref.load_actor("attitude")
        task = task_registry.make_task("position_setpoint_task", seed=42, num_envs=n, headless=True)
        actor = ActorMLP.from_arrays(ws, bs, logstd=logstd, device=DEV, task=task)
        assert actor.rng_seed == task.sim_env.rng_seed and actor.env_index_base == task.sim_env.env_offset
        obs = task.reset()[0]
        crashes, dist_late = 0, []
        for t in range(steps):
            a = actor(obs["observations"], sample=sample, clamp=True)
            obs, _rew, term, _trunc, _ = task.step(a)
            crashes += int(term.sum())
            if 400 <= t < 500:  # the last second of the first episode: obs[:, 0:3] = target - position
                dist_late.append(obs["observations"][:, 0:3].norm(dim=1).clone())
        d = torch.stack(dist_late)
        return {"crashes": crashes, "dist_late_mean": float(d.mean()), "dist_late_p95": float(d.flatten().quantile(0.95)),
                "finite": bool(torch.isfinite(d).all())}
    finally:
        cfg.controller_name, cfg.episode_len_steps, cfg.args, cfg.robot_name = old


@pytest.mark.parametrize("sample", [False, True])
def test_attitude_actor_flies_the_position_task_through_actor_mlp(sample):
    """The thresholds tests/test_gpu_policy_transfer.py holds the torch actor to.  Measured (MI355X, 512 envs, steps 400-499): no
    crash; distance 0.153 m mean / 0.223 m p95 deterministic, 0.162 / 0.244 with sampled actions (the torch actor at 2048 envs:
    0.155 / 0.22 and 0.16 / 0.24)."""
    r = fly_attitude(sample)
    print("fused actor, closed loop:", "sampled" if sample else "deterministic", r)
    assert r["finite"] and r["crashes"] == 0
    assert r["dist_late_mean"] < 0.25 and r["dist_late_p95"] < 0.4


def test_lmf2_acceleration_actor_flies_through_the_reference_mlp_class(tmp_path):
    """MLP(17, 4, path) from a checkpoint file, imported under the reference's path, around EnvManager: the loop of
    tests/test_gpu_policy_transfer.py fly_lmf2 and its thresholds.  Measured (MI355X, 512 spawns, last second of 8): 0.079 m mean /
    0.158 m p95, 0.065 m/s, no crash (the torch actor at 2048 spawns: 0.079 / 0.16, 0.07)."""
    import aerial_gym  # noqa: F401
    from aerial_gym.examples.rl_games_example.rl_games_inference import MLP

    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config.robot_config import LMF2Cfg
    from aerial_gym_simulator_amd.sim.sim_builder import SimBuilder

    ws, bs, logstd = policy_ref.load_actor("lmf2_acceleration")
    path = policy_ref.write_checkpoint(tmp_path / "acc.pth", policy_ref.rl_games_state_dict(ws, bs, logstd))
    model = MLP(17, 4, path).to(DEV).eval()
    n, steps, scale = 512, 800, 2.0
    cam = LMF2Cfg.sensor_config.enable_camera
    LMF2Cfg.sensor_config.enable_camera = False
    try:
        env = SimBuilder().build_env(sim_name="base_sim", env_name="empty_env", robot_name="lmf2", controller_name="lmf2_acceleration_control",
                                     args={}, device=DEV, num_envs=n, use_warp=False, headless=True)
    finally:
        LMF2Cfg.sensor_config.enable_camera = cam
    env.reset()
    od = env.get_obs()
    actions = torch.zeros((n, 4), device=DEV)
    dist, speed_late, d0 = [], [], None
    for t in range(steps):
        q = od["robot_orientation"]
        q = torch.where(q[:, 3:4] < 0.0, -q, q)
        obs = torch.cat([-od["robot_position"], q, od["robot_body_linvel"], od["robot_body_angvel"], od["robot_actions"]], dim=1)
        if d0 is None:
            d0 = obs[:, 0:3].norm(dim=1).clone()
        actions[:] = model.forward(obs).clamp(-1.0, 1.0)
        actions[:, 0:3] *= scale
        env.step(actions=actions)
        if t >= steps - 100:
            dist.append(od["robot_position"].norm(dim=1).clone())
            speed_late.append(od["robot_linvel"].norm(dim=1).clone())
    d = torch.stack(dist)
    r = {"start_dist_mean": float(d0.mean()), "dist_late_mean": float(d.mean()), "dist_late_p95": float(d.flatten().quantile(0.95)),
         "speed_late_mean": float(torch.stack(speed_late).mean()), "crashed": int((od["crashes"] != 0).sum()),
         "finite": bool(torch.isfinite(od["robot_state_tensor"]).all())}
    print("fused actor through MLP, lmf2 acceleration:", r)
    assert r["finite"] and r["crashed"] == 0 and r["start_dist_mean"] > 0.5
    assert r["dist_late_mean"] < 0.2 and r["dist_late_p95"] < 0.35 and r["speed_late_mean"] < 0.2


@pytest.mark.parametrize("from_checkpoint", [False, True])
def test_closed_loop_example_runs_and_reaches_the_set_point(from_checkpoint, tmp_path):
    """examples/rl_env_closed_loop_example.py as a user starts it: from the fixture, and from a checkpoint file through MLP"""
    import os
    import re
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = []
    if from_checkpoint:
        ws, bs, logstd = policy_ref.load_actor("attitude")
        args = [policy_ref.write_checkpoint(tmp_path / "attitude.pth", policy_ref.rl_games_state_dict(ws, bs, logstd))]
    env = dict(os.environ, AGX_EXAMPLE_STEPS="400", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "rl_env_closed_loop_example.py")] + args, env=env, capture_output=True,
                         text=True, timeout=300, cwd=root)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    dist = [float(m) for m in re.findall(r"distance to the set-point ([0-9.]+) m mean", out.stdout)]
    assert len(dist) == 4 and dist[-1] < 0.4 and dist[-1] < dist[0], out.stdout[-1500:]
