"""GPU: the fused recurrent actor (csrc/agx_policy.hip k_recurrent_act, one launch per call) against

1. the chain it restates, bit for bit: agx_vae_linear per linear map (the head padded to 32 zero rows), agx_math_eval for the
   sigmoid and the tanh, the gate arithmetic in float32 numpy with one rounding per operation -- on actions, mean, logstd_out and
   hidden, over three consecutive calls with flags set on the second, over nets and batch sizes that reach every edge;
2.-4. invariance to batch and placement, canary rows behind every output, reset before / after with one and two flag tensors;
5. sigmoid_cw / tanh_cw correctly rounded; 6. sampling; 7. no allocation, current stream; 8. refusals and the empty batch;
9. the closed loop on navigation_task against the chain on a second identically seeded task; 10. the example."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import recurrent_policy_ref as ref
import torch
from recurrent_policy_ref import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 31, 32, 33, 69)
MATH_EXP = 4  # AGX_MATH_EXP
# name: (encoder widths, hidden, actions, adaptive, activation)
NETS = {
    "in1-a1": ([1, 32], 32, 1, True, "elu"), "in7-a3": ([7, 32], 32, 3, True, "elu"), "in8-a4-relu": ([8, 32], 32, 4, True, "relu"),
    "in9-a16": ([9, 64], 64, 16, True, "elu"),            # 2 A = 32: exactly one padded tile
    "a17": ([9, 32], 32, 17, True, "elu"),                 # 2 A = 34 crosses the 32-row padding
    "a17-constant-logstd": ([9, 32], 32, 17, False, "relu"),
    "enc512": ([13, 512, 32], 32, 4, True, "elu"),         # 512 channels: four tiles per wave
    "h96": ([13, 64], 96, 3, True, "elu"),                 # 3 H = nine tiles, uneven over four waves; cell input 64 != H
    "h160": ([8, 32], 160, 4, True, "relu"),               # the largest H the LDS check admits; 3 H = fifteen tiles
    "six-encoder-layers": ([19, 64, 32, 96, 32, 64, 32], 32, 3, True, "elu"),  # the deepest encoder the check admits: nine maps
}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _L():
    from aerial_gym_simulator_amd import _lib

    return _lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _net(name):
    if name == "fixture":
        return ref.load_fixture()
    dims, hidden, actions, adaptive, activation = NETS[name]
    return ref.random_net(dims, hidden, actions, _gen(2000 + sorted(NETS).index(name)), adaptive=adaptive, activation=activation)


def _actor(net, **kw):
    from aerial_gym_simulator_amd.utils.policy import RecurrentActor

    return RecurrentActor.from_arrays(device=DEV, **ref.actor_kwargs(net), **kw)


def math_eval(which, x):
    L = _L()
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV).reshape(-1)
    out = torch.empty_like(xd)
    L.check(L.load().agx_math_eval(which, xd.numel(), L.dptr(xd), L.dptr(xd), L.dptr(out), _stream()), "agx_math_eval")
    return out.cpu().numpy().reshape(np.shape(x))


class Chain:
    """the actor as separate calls: see the module docstring.  step() takes and returns numpy float32."""

    def __init__(self, net):
        from aerial_gym_simulator_amd.utils.policy import pack_layer

        self.net = net
        self.A = ref.num_actions(net)

        def pack(w, b, pad):
            rows = -(-w.shape[0] // pad) * pad
            bias = np.zeros(rows, np.float32)
            bias[:w.shape[0]] = b
            return torch.from_numpy(pack_layer(w, pad_rows_to=pad)).to(DEV), torch.from_numpy(bias).to(DEV), w.shape[1], rows

        self.enc = [pack(w, b, 1) for w, b in zip(net["enc_weights"], net["enc_biases"])]
        self.ih, self.hh = pack(net["w_ih"], net["b_ih"], 1), pack(net["w_hh"], net["b_hh"], 1)
        self.head = pack(net["head_weight"], net["head_bias"], 32)

    def linear(self, x, layer, elu=False):
        L = _L()
        wp, bias, fin, rows = layer
        x = x.contiguous()
        y = torch.full((x.shape[0], rows), float("nan"), device=DEV)
        L.check(L.load().agx_vae_linear(x.shape[0], L.dptr(x), L.dptr(wp), L.dptr(bias), L.dptr(y), fin, rows, L.VAE_ELU if elu else 0, _stream()),
                "agx_vae_linear")
        return y

    def step(self, obs, h, flagged=None, reset="before"):
        net = self.net
        x = np.asarray(obs, np.float32)
        if net["input_norm"] is not None:
            x = ref.norm_f32(x, *net["input_norm"])
        x = torch.from_numpy(x).to(DEV)
        for layer in self.enc:
            x = self.linear(x, layer, elu=net["activation"] == "elu")
            if net["activation"] == "relu":
                x = torch.where(x < 0, torch.zeros_like(x), x)
        h = np.array(h, np.float32)
        if flagged is not None and reset == "before":
            h[flagged] = 0.0
        gi = self.linear(x, self.ih).cpu().numpy()
        gh = self.linear(torch.from_numpy(h).to(DEV), self.hh).cpu().numpy()
        L = _L()
        hn = ref.gates_f32(gi, gh, h, sigmoid=lambda v: math_eval(L.MATH_SIGMOID, v), tanh=lambda v: math_eval(L.MATH_TANH, v))
        y = self.linear(torch.from_numpy(hn).to(DEV), self.head).cpu().numpy()
        assert np.isfinite(y).all() and np.isfinite(hn).all()
        stored = hn.copy()
        if flagged is not None and reset == "after":
            stored[flagged] = 0.0
        A = self.A
        logstd = y[:, A:2 * A] if net["logstd"] is None else np.broadcast_to(net["logstd"], (y.shape[0], A))
        return {"mean": y[:, :A].copy(), "logstd": np.ascontiguousarray(logstd), "hidden": stored}


def _flags(n, g, p=0.3):
    f = torch.rand(n, generator=g) < p
    f[0] = True
    return f


@pytest.mark.parametrize("name", ["fixture"] + list(NETS))
def test_fused_equals_the_chain_bit_for_bit(name):
    net = _net(name)
    chain = Chain(net)
    g = _gen(7)
    span = 3.0 if name == "fixture" else 2.0
    for n in BATCHES:
        actor = _actor(net)
        h = np.zeros((n, actor.hidden_dim), np.float32)
        for call in range(3):
            obs = (torch.rand((n, actor.obs_dim), generator=g) * 2 - 1) * span
            d0, d1 = (_flags(n, g), _flags(n, g, 0.1)) if call == 1 else (None, None)
            flagged = None if d0 is None else (d0 | d1).numpy()
            want = chain.step(obs.numpy(), h, flagged)
            got = actor(obs.to(DEV), done=None if d0 is None else (d0.to(DEV), d1.to(DEV)))
            torch.cuda.synchronize()
            for value, key in ((got, "mean"), (actor.mean, "mean"), (actor.logstd_out, "logstd"), (actor.hidden, "hidden")):
                assert np.array_equal(bits(value), bits(want[key])), (name, n, call, key, float(np.abs(value.cpu().numpy() - want[key]).max()))
            h = want["hidden"]
        assert np.abs(h).max() > 0.01


def test_a_smaller_actor_created_later_does_not_disturb_a_larger_one():
    """the largest LDS the check admits (148480 bytes), then an actor of 33792 bytes, then the large one is called"""
    big_net, small_net = _net("h160"), _net("in1-a1")
    big = _actor(big_net)
    small = _actor(small_net)
    assert big.lds_bytes == 148480 and small.lds_bytes == 33792
    g = _gen(8)
    obs = torch.rand((33, 8), generator=g) * 4 - 2
    small(torch.rand((33, 1), generator=g).to(DEV))
    got = big(obs.to(DEV))
    want = Chain(big_net).step(obs.numpy(), np.zeros((33, 160), np.float32))
    assert np.array_equal(bits(got), bits(want["mean"])) and np.array_equal(bits(big.hidden), bits(want["hidden"]))


def test_an_env_has_the_same_bits_wherever_it_is_evaluated():
    net = ref.load_fixture()
    g = _gen(40)
    n = 69
    obs = [((torch.rand((n, 81), generator=g) * 2 - 1) * 3).to(DEV) for _ in range(2)]
    flags = _flags(n, g).to(DEV)

    def run(rows, other_flags=None):
        """two calls on the sub-batch `rows` (in that order), flags on the second; returns actions and state after both"""
        actor = _actor(net)
        idx = torch.as_tensor(rows, device=DEV)
        actor(obs[0][idx].contiguous())
        f = (flags if other_flags is None else other_flags)[idx].contiguous()
        a = actor(obs[1][idx].contiguous(), done=f).clone()
        return a, actor.hidden.clone()

    full_a, full_h = run(list(range(n)))
    for row in (0, 31, 32, 68):
        a, h = run([row])
        assert np.array_equal(bits(a[0]), bits(full_a[row])) and np.array_equal(bits(h[0]), bits(full_h[row])), row
    perm = torch.randperm(n, generator=g).tolist()
    a, h = run(perm)
    assert np.array_equal(bits(a), bits(full_a[perm])) and np.array_equal(bits(h), bits(full_h[perm]))
    a, h = run(list(range(20, 53)))  # another batch size, other tile boundaries
    assert np.array_equal(bits(a), bits(full_a[20:53])) and np.array_equal(bits(h), bits(full_h[20:53]))
    # other envs' flags: invert every flag but those of rows 5 and 40
    other = ~flags
    other[5], other[40] = flags[5], flags[40]
    a, h = run(list(range(n)), other)
    for row in (5, 40):
        assert np.array_equal(bits(a[row]), bits(full_a[row])) and np.array_equal(bits(h[row]), bits(full_h[row]))


@pytest.mark.parametrize("n", [1, 33])
def test_no_write_behind_the_live_rows(n):
    L = _L()
    lib = L.load()
    net = _net("a17")
    actor = _actor(net)
    H, A, extra = actor.hidden_dim, actor.action_dim, 40
    g = _gen(50 + n)
    obs = torch.rand((n, actor.obs_dim), generator=g).to(DEV)
    hidden = torch.full((n + extra, H), 7.0, device=DEV)
    hidden[:n] = 0.25
    outs = [torch.full((n + extra, A), 7.0, device=DEV) for _ in range(3)]
    done = torch.zeros(n + extra, dtype=torch.uint8, device=DEV)
    L.check(lib.agx_recurrent_act(actor._handle, n, L.dptr(obs), L.dptr(hidden), L.dptr(done), None, L.dptr(outs[0]), L.dptr(outs[1]), L.dptr(outs[2]),
                                  None, 0, 0, 0, 0, _stream()), "agx_recurrent_act")
    torch.cuda.synchronize()
    want = Chain(net).step(obs.cpu().numpy(), np.full((n, H), 0.25, np.float32))
    assert np.array_equal(bits(hidden[:n]), bits(want["hidden"])) and np.array_equal(bits(outs[1][:n]), bits(want["mean"]))
    assert np.array_equal(bits(outs[0][:n]), bits(want["mean"])) and np.array_equal(bits(outs[2][:n]), bits(want["logstd"]))
    assert bool((hidden[n:] == 7.0).all()) and all(bool((o[n:] == 7.0).all()) for o in outs)


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8])
@pytest.mark.parametrize("reset", ["before", "after"])
def test_reset_before_and_after(dtype, reset):
    net = _net("in9-a16")
    chain = Chain(net)
    g = _gen(60)
    n = 33
    obs = [(torch.rand((n, 9), generator=g) * 4 - 2) for _ in range(2)]
    d0, d1 = _flags(n, g), _flags(n, g, 0.2)
    d1[32] = True  # the lone env of the second tile
    h1 = chain.step(obs[0].numpy(), np.zeros((n, 64), np.float32))["hidden"]
    for done, flagged in ((d0, d0), ((d0,), d0), ((d0, d1), d0 | d1)):
        actor = _actor(net)
        actor(obs[0].to(DEV))
        dev_done = tuple(d.to(dtype).to(DEV) for d in done) if isinstance(done, tuple) else done.to(dtype).to(DEV)
        got = actor(obs[1].to(DEV), done=dev_done, reset=reset)
        want = chain.step(obs[1].numpy(), h1, flagged.numpy(), reset)
        assert np.array_equal(bits(got), bits(want["mean"])) and np.array_equal(bits(actor.hidden), bits(want["hidden"]))
        rows = flagged.numpy()
        if reset == "after":
            assert bool((actor.hidden[torch.from_numpy(rows).to(DEV)] == 0).all())
            assert np.array_equal(bits(got), bits(chain.step(obs[1].numpy(), h1)["mean"]))  # the head saw h'
        else:
            zero_state = chain.step(obs[1].numpy(), np.zeros_like(h1))
            assert np.array_equal(bits(got)[rows], bits(zero_state["mean"])[rows])
    # reset(ids) on the device
    actor.reset(torch.tensor([1, 2], device=DEV))
    assert bool((actor.hidden[1:3] == 0).all()) and bool((actor.hidden[3] != 0).any())


def test_sigmoid_and_tanh_are_correctly_rounded():
    """against libm in double, rounded once: <= 0.5 ulp everywhere, equal to the nearest float for > 99.999 % (tests/test_gpu_math.py)"""
    L = _L()
    rng = np.random.default_rng(12)
    sweeps = ((L.MATH_TANH, np.tanh, np.concatenate([np.linspace(-12, 12, 1_000_001), rng.uniform(-12, 12, 1_000_000)])),
              (L.MATH_TANH, np.tanh, np.concatenate([np.linspace(-1e-3, 1e-3, 400_001), rng.uniform(-1e-3, 1e-3, 400_000)])),
              (L.MATH_SIGMOID, lambda v: 1.0 / (1.0 + np.exp(-v)), np.concatenate([np.linspace(-87, 20, 1_000_001), rng.uniform(-87, 20, 1_000_000)])))
    for which, fn, x in sweeps:
        x = x.astype(np.float32)
        got = math_eval(which, x)
        exact = fn(x.astype(np.float64))
        assert np.mean(got == exact.astype(np.float32)) > 0.99999, which
        ulp = np.maximum(np.spacing(np.abs(exact.astype(np.float32))).astype(np.float64), np.spacing(np.float32(1e-30)))
        assert (np.abs(got.astype(np.float64) - exact) / ulp).max() <= 0.5 + 1e-5, which
    # tanh: tiny arguments and signed zeros come back unchanged; saturation to exactly +-1
    tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, 1.17549435e-38, 1e-20, -1e-10, 6e-5, -6.1e-5], np.float32)
    assert np.array_equal(bits(math_eval(L.MATH_TANH, tiny)), bits(tiny))
    big = np.array([9.1, 10.0, 10.5, 12.5, 50.0, 3e38, np.inf], np.float32)
    assert np.array_equal(bits(math_eval(L.MATH_TANH, big)), bits(np.ones(7, np.float32)))
    assert np.array_equal(bits(math_eval(L.MATH_TANH, -big)), bits(-np.ones(7, np.float32)))
    # sigmoid: exactly 1 for large arguments; below the smallest normal float flushed to 0, as exp_cw
    assert np.array_equal(bits(math_eval(L.MATH_SIGMOID, np.array([17.5, 20.0, 20.5, 88.0, 1000.0, np.inf], np.float32))), bits(np.ones(6, np.float32)))
    low = np.array([-87.4, -88.0, -100.0, -104.0, -1000.0, -np.inf], np.float32)
    assert np.array_equal(bits(math_eval(L.MATH_SIGMOID, low)), bits(np.zeros(6, np.float32)))
    assert np.array_equal(bits(math_eval(MATH_EXP, low)), bits(np.zeros(6, np.float32)))
    edge = np.array([-87.3365402, -87.33], np.float32)  # the last arguments before the flush: normal, and exp_cw's value
    assert np.array_equal(bits(math_eval(L.MATH_SIGMOID, edge)), bits(math_eval(MATH_EXP, edge))) and (math_eval(L.MATH_SIGMOID, edge) >= 2.0 ** -126).all()
    assert math_eval(L.MATH_SIGMOID, np.zeros(1, np.float32))[0] == 0.5
    assert np.isnan(math_eval(L.MATH_SIGMOID, np.array([np.nan], np.float32))[0]) and np.isnan(math_eval(L.MATH_TANH, np.array([np.nan], np.float32))[0])


@pytest.mark.parametrize("name", ["fixture", "a17-constant-logstd"])
def test_sampling(name):
    net = _net(name)
    g = _gen(70)
    n = 69
    actor = _actor(net, rng_seed=1234, env_index_base=0)
    A = actor.action_dim
    obs = ((torch.rand((n, actor.obs_dim), generator=g) * 2 - 1) * 3).to(DEV)
    eps = torch.randn((n, A), generator=g) * 2
    mu = actor(obs).clone().cpu().numpy()
    logstd = actor.logstd_out.clone().cpu().numpy()
    if name != "fixture":
        assert np.array_equal(bits(logstd), bits(np.broadcast_to(net["logstd"], (n, A))))
    for clamp in (False, True):  # every call from the same zero state: the same mean and log-std
        actor.reset()
        got = actor(obs, sample=True, clamp=clamp, eps=eps.to(DEV))
        assert np.array_equal(bits(got), bits(ref.sample_f32(mu, eps.numpy(), logstd, clamp))), clamp
        assert np.array_equal(bits(actor.mean), bits(mu)) and np.array_equal(bits(actor.logstd_out), bits(logstd))
    assert (np.abs(ref.sample_f32(mu, eps.numpy(), logstd)) > 1).any()  # the clamp had something to do, and it came last
    # the device generator: the stream noise() predicts, a function of (seed, global env index, step, action) alone
    noise = actor.noise(n, step=5).cpu().numpy()
    actor.reset()
    got = actor(obs, sample=True, step=5).clone()
    assert np.array_equal(bits(got), bits(ref.sample_f32(mu, noise, logstd)))
    actor.env_index_base = 37
    shifted = actor.noise(n, step=5).cpu().numpy()
    actor.reset()
    tail = actor(obs[:32].contiguous(), sample=True, step=5).clone()
    actor.env_index_base = 0
    wide = actor.noise(n + 37, step=5).cpu().numpy()
    assert np.array_equal(bits(shifted), bits(wide[37:]))
    assert np.array_equal(bits(tail), bits(ref.sample_f32(mu[:32], wide[37:69], logstd[:32])))  # another place, another batch size
    assert not np.array_equal(noise, actor.noise(n, step=6).cpu().numpy())
    if A == 4:  # the stream of ActorMLP.noise for the same number of actions
        import policy_ref
        from aerial_gym_simulator_amd.utils.policy import ActorMLP

        ws, bs, ls = policy_ref.load_actor("attitude")
        mlp = ActorMLP.from_arrays(ws, bs, logstd=ls, device=DEV, rng_seed=1234, env_index_base=0)
        assert np.array_equal(bits(mlp.noise(n, step=5)), bits(noise))
    # without step= and without a task the object counts its sampled calls
    assert actor.step == 0
    actor.reset()
    first = actor(obs, sample=True).clone()
    assert actor.step == 1 and np.array_equal(bits(first), bits(ref.sample_f32(mu, actor.noise(n, step=0).cpu().numpy(), logstd)))


def test_calls_allocate_nothing_and_run_on_the_current_stream():
    net = ref.load_fixture()
    actor = _actor(net)
    g = _gen(80)
    n = 1057
    obs = ((torch.rand((n, 81), generator=g) * 2 - 1) * 3).to(DEV)
    done = (_flags(n, g).to(DEV), _flags(n, g).to(DEV))
    actor(obs, done=done, sample=True, clamp=True, step=3)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for _ in range(100):
        actor(obs, done=done, sample=True, clamp=True, step=3)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    # a side stream: the observations are written by work queued on that stream right before the call
    host = (torch.rand((n, 81), generator=g) * 2 - 1) * 3
    actor.reset()
    want = actor(host.to(DEV)).clone()
    want_h = actor.hidden.clone()
    actor.reset()
    staging, result = torch.zeros((n, 81), device=DEV), torch.zeros((n, 4), device=DEV)
    pinned = host.pin_memory()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(20):
            staging.copy_(pinned, non_blocking=True).mul_(1.0)
        actor(staging, out=result)
    side.synchronize()
    assert np.array_equal(bits(result), bits(want)) and np.array_equal(bits(actor.hidden), bits(want_h))


def test_refusals_and_the_empty_batch():
    L = _L()
    lib = L.load()
    net = _net("a17-constant-logstd")
    actor = _actor(net)
    h = actor._handle
    obs = torch.zeros((4, 9), device=DEV)
    hidden = torch.full((4, 32), 7.0, device=DEV)
    out = torch.full((4, 17), 7.0, device=DEV)
    p = L.dptr
    assert lib.agx_recurrent_act(h, 0, None, None, None, None, None, None, None, None, 0, 0, 0, 0, _stream()) == 0  # nothing to do
    assert lib.agx_recurrent_act(h, 0, p(obs), p(hidden), None, None, p(out), None, None, None, 0, 0, 0, 0, _stream()) == 0
    for args, text in (((h, 4, None, p(hidden), None, None, p(out), None, None, None, 0), "null obs"),
                       ((h, 4, p(obs), None, None, None, p(out), None, None, None, 0), "null hidden"),
                       ((h, 4, p(obs), p(hidden), None, None, None, None, None, None, 0), "null actions"),
                       ((h, 4, p(obs), p(hidden), None, None, p(out), None, None, None, 8), "flags = 8"),
                       ((h, -1, p(obs), p(hidden), None, None, p(out), None, None, None, 0), "num_envs = -1"),
                       ((None, 4, p(obs), p(hidden), None, None, p(out), None, None, None, 0), "null handle")):
        assert lib.agx_recurrent_act(*args, 0, 0, 0, _stream()) == -1
        assert text in lib.agx_last_error().decode(), text
    # a head that is not adaptive and has no log-std cannot sample or report one
    assert lib.agx_recurrent_set_logstd(h, None) == 0
    assert lib.agx_recurrent_act(h, 4, p(obs), p(hidden), None, None, p(out), None, None, None, L.POLICY_SAMPLE, 0, 0, 0, _stream()) == -1
    assert "logstd" in lib.agx_last_error().decode()
    assert lib.agx_recurrent_act(h, 4, p(obs), p(hidden), None, None, p(out), None, p(out), None, 0, 0, 0, 0, _stream()) == -1
    assert "logstd" in lib.agx_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((hidden == 7.0).all())  # no refused call wrote anything
    adaptive = _actor(_net("in7-a3"))
    assert lib.agx_recurrent_set_logstd(adaptive._handle, net["logstd"].ctypes.data) == -1 and "adaptive" in lib.agx_last_error().decode()
    # create refuses what the limits exclude, before it touches the device
    handle = C.c_void_p()
    w = np.zeros((3 * 192, 192), np.float32)
    wp = (C.c_void_p * 1)(w.ctypes.data)
    d = w.ctypes.data
    assert lib.agx_recurrent_create(1, (C.c_int32 * 2)(8, 32), 192, 4, 1, wp, wp, d, d, d, d, d, d, L.POLICY_ELU, C.byref(handle)) == -1 and not handle.value
    assert "177152" in lib.agx_last_error().decode()
    assert lib.agx_recurrent_create(1, (C.c_int32 * 2)(8, 32), 32, 65, 1, wp, wp, d, d, d, d, d, d, L.POLICY_ELU, C.byref(handle)) == -1 and not handle.value
    assert "num_actions = 65" in lib.agx_last_error().decode()
    assert lib.agx_recurrent_create(1, (C.c_int32 * 2)(8, 32), 32, 4, 1, wp, wp, d, d, d, d, d, d, L.POLICY_NONE, C.byref(handle)) == -1 and not handle.value
    assert "hidden_activation = 0" in lib.agx_last_error().decode()
    with pytest.raises(ValueError, match=r"float32 \[N, 9\]"):
        actor(torch.zeros((4, 8), device=DEV))
    with pytest.raises(RuntimeError, match="HIP device"):
        actor(torch.zeros((4, 9)))
    assert L.load().agx_math_eval(8, 1, p(obs), p(obs), p(out), _stream()) == -1 and "which = 8" in lib.agx_last_error().decode()


# ---- the closed loop ------------------------------------------------------------------------------------------------------------
CLOSED_LOOP = {"envs": 48, "steps": 12, "seed": 3, "rng_seed": 77, "episode_len_steps": 5}


def _nav_task(n):
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config.task_config import navigation_task_config as cfg
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    old = (cfg.episode_len_steps, cfg.args, cfg.device)
    try:
        cfg.device, cfg.episode_len_steps, cfg.args = DEV, CLOSED_LOOP["episode_len_steps"], {"rng_seed": CLOSED_LOOP["rng_seed"]}
        return task_registry.make_task("navigation_task", seed=CLOSED_LOOP["seed"], num_envs=n, headless=True)
    finally:
        cfg.episode_len_steps, cfg.args, cfg.device = old


def test_closed_loop_on_the_navigation_task_equals_the_chain():
    """48 envs (one full and one partial tile), the fixture actor fed done=(task.terminations, task.truncations): the fused actor
    on one task, the chain on a second identically seeded one; actions and hidden bit for bit at every step.  Seed, episode length
    and step count (CLOSED_LOOP) were picked on the device so that flags fire: measured (MI355X) 6 over the 12 steps."""
    n, steps = CLOSED_LOOP["envs"], CLOSED_LOOP["steps"]
    net = ref.load_fixture()
    task_a = _nav_task(n)
    obs_a = task_a.reset()[0]["observations"]
    task_b = _nav_task(n)  # created after the first one's reset: make_task seeds the host generators the reset draws from
    obs_b = task_b.reset()[0]["observations"]
    try:
        actor, chain = _actor(net, task=task_a), Chain(net)
        h = np.zeros((n, 64), np.float32)
        fired = 0
        for t in range(steps):
            assert np.array_equal(bits(obs_a), bits(obs_b)), t
            flagged = (task_b.terminations | task_b.truncations).cpu().numpy().astype(bool)
            fired += int(flagged.sum())
            act_a = actor(obs_a, done=(task_a.terminations, task_a.truncations), clamp=True)
            want = chain.step(obs_b.cpu().numpy(), h, flagged)
            h = want["hidden"]
            act_b = np.clip(want["mean"], np.float32(-1), np.float32(1))
            assert np.array_equal(bits(act_a), bits(act_b)) and np.array_equal(bits(actor.hidden), bits(h)), t
            obs_a = task_a.step(act_a)[0]["observations"]
            obs_b = task_b.step(torch.from_numpy(act_b).to(DEV))[0]["observations"]
        print(f"closed loop: {fired} flags over {steps} steps of {n} envs")
        assert fired > 0
    finally:
        task_a.close()
        task_b.close()


def test_recurrent_closed_loop_example_runs():
    env = dict(os.environ, AGX_EXAMPLE_STEPS="40", AGX_EXAMPLE_ENVS="48", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "recurrent_actor_closed_loop_example.py")], env=env, capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    assert "steps per second" in out.stdout, out.stdout[-1500:]
