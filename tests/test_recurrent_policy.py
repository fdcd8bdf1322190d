"""CPU: RecurrentActor (utils/policy.py) without a GPU -- the float32 CPU path against the float64 statement within the propagated
bound and against torch.nn.GRU, the sample-factory loader and its refusals, the host-only limits, the hidden-state semantics, the
two drop-in classes, and the header / ctypes mirrors of the recurrent entries.

Measured on the fixture (CPU path, 64 envs): against torch.nn.GRU 1.6e-6 on h; against float64 2e-5 on h after 200 steps; over
the 8 steps of the first test max |err| / bound = 3.5e-5.  The bound holds for any summation order and is carried through eight
recurrent steps, so it is four orders of magnitude loose: it catches a wrong formula, not a wrong rounding.  The check with teeth
on the CPU path is the comparison with torch.nn.GRU on the same weights (1e-5 on h, 1e-4 on the means) in the same test."""
import os
import re
import types

import numpy as np
import pytest
import recurrent_policy_ref as ref
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _actor(net, **kw):
    from aerial_gym_simulator_amd.utils.policy import RecurrentActor

    return RecurrentActor.from_arrays(device="cpu", **ref.actor_kwargs(net), **kw)


def _small(gen=None, **kw):
    return ref.random_net([9, 32], 32, 3, gen or _gen(5), **kw)


def test_cpu_path_within_the_propagated_bound_and_equal_to_torch_gru():
    net = ref.load_fixture()
    actor, module = _actor(net), ref.TorchActor(net)
    g = _gen(1)
    n, H = 64, 64
    h64, err = torch.zeros((n, H), dtype=torch.float64), torch.zeros((n, H), dtype=torch.float64)
    h_torch = torch.zeros((n, H))
    worst = 0.0
    for step in range(8):
        obs = (torch.rand((n, 81), generator=g) * 2 - 1) * (3.0 if step % 2 else 1.0)
        flagged = (torch.rand(n, generator=g) < 0.1) if step == 4 else None
        want = ref.step64(net, obs, h64, err, flagged, fn=ref.FN_TORCH)  # torch's CPU sigmoid / tanh / elu are the path under test
        actor(obs, done=flagged)
        for got, key in ((actor.mean, "mean"), (actor.logstd_out, "logstd"), (actor.hidden, "hidden")):
            bound = want["err_" + key]
            assert float(bound.min()) > 0
            ratio = float(((got.double() - want[key]).abs() / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (step, key, ratio)
        h64, err = want["hidden"], want["err_hidden"]
        if flagged is not None:
            h_torch[flagged] = 0.0
        y, h_torch = module(obs, h_torch)
        assert float((actor.hidden - h_torch).abs().max()) < 1e-5 and float((actor.mean - y[:, :4]).abs().max()) < 1e-4
    print(f"max |err| / bound over 8 steps = {worst:.3e}")


@pytest.mark.parametrize("obs_key", ["obs", "observations"])
@pytest.mark.parametrize("adaptive", [True, False])
def test_loader_round_trips_a_synthetic_checkpoint(tmp_path, obs_key, adaptive):
    from aerial_gym_simulator_amd.utils.policy import RecurrentActor

    g = _gen(2)
    net = ref.random_net([9, 64, 32], 32, 3, g, adaptive=adaptive)
    mean, var = torch.randn(9, generator=g, dtype=torch.float64).numpy(), (torch.rand(9, generator=g, dtype=torch.float64) + 0.1).numpy()
    ckdir = ref.write_experiment(tmp_path, "exp", {"best_000000001_1_reward_1.0.pth": ref.sf_state_dict(net, obs_key, (mean, var))}, ref.SF_CONFIG)
    actor = RecurrentActor.from_sample_factory_checkpoint(ckdir, device="cpu")
    assert actor.obs_key == obs_key and actor.adaptive == adaptive and (actor.obs_dim, actor.hidden_dim, actor.action_dim) == (9, 32, 3)
    for got, want in zip(actor.enc_weights + actor.enc_biases, net["enc_weights"] + net["enc_biases"]):
        assert np.array_equal(got, want)
    for name in ("w_ih", "w_hh", "b_ih", "b_hh", "head_weight", "head_bias"):
        assert np.array_equal(getattr(actor, name), net[name]), name
    assert (actor.logstd is None) if adaptive else np.array_equal(actor.logstd, net["logstd"])
    # float64 statistics: rounded to float32 first, denom = sqrt(var + 1e-5) in float32, clip 5
    m, d, clip = actor.input_norm
    assert m.dtype == d.dtype == np.float32 and clip == 5.0
    assert np.array_equal(m, mean.astype(np.float32)) and np.array_equal(d, ref.sf_denom(var))
    # the same file by its path; normalize_input: false drops the normaliser
    direct = RecurrentActor.from_sample_factory_checkpoint(os.path.join(ckdir, "best_000000001_1_reward_1.0.pth"), device="cpu")
    assert np.array_equal(direct.w_ih, net["w_ih"]) and direct.input_norm is not None
    ckdir2 = ref.write_experiment(tmp_path, "exp2", {"best_1.pth": ref.sf_state_dict(net, obs_key, (mean, var))},
                                  dict(ref.SF_CONFIG, normalize_input=False, nonlinearity="relu"))
    plain = RecurrentActor.from_sample_factory_checkpoint(ckdir2, device="cpu")
    assert plain.input_norm is None and plain.activation == "relu"
    obs = torch.rand((5, 9), generator=g)
    want = ref.step64(dict(net, input_norm=(m, d, clip)), obs, torch.zeros(5, 32), torch.zeros(5, 32))
    actor(obs)
    assert float((actor.mean.double() - want["mean"]).abs().max()) < 1e-5
    assert float((actor.logstd_out.double() - want["logstd"]).abs().max()) < 1e-5


def test_loader_resolves_best_and_latest(tmp_path):
    from aerial_gym_simulator_amd.utils.policy import RecurrentActor, find_sample_factory_checkpoint

    nets = [_small(_gen(10 + i)) for i in range(4)]
    files = {"best_000000100_51200_reward_1.5.pth": ref.sf_state_dict(nets[0]), "best_000000300_153600_reward_9.25.pth": ref.sf_state_dict(nets[1]),
             "checkpoint_000000200_102400.pth": ref.sf_state_dict(nets[2]), "checkpoint_000000400_204800.pth": ref.sf_state_dict(nets[3])}
    ckdir = ref.write_experiment(tmp_path, "exp", files)
    assert os.path.basename(find_sample_factory_checkpoint(ckdir, "best")) == "best_000000300_153600_reward_9.25.pth"
    assert os.path.basename(find_sample_factory_checkpoint(ckdir, "latest")) == "checkpoint_000000400_204800.pth"
    assert np.array_equal(RecurrentActor.from_sample_factory_checkpoint(ckdir, device="cpu").w_hh, nets[1]["w_hh"])
    assert np.array_equal(RecurrentActor.from_sample_factory_checkpoint(ckdir, device="cpu", kind="latest").w_hh, nets[3]["w_hh"])
    with pytest.raises(ValueError, match="newest"):
        find_sample_factory_checkpoint(ckdir, "newest")
    empty = tmp_path / "none" / "checkpoint_p0"
    empty.mkdir(parents=True)
    with pytest.raises(FileNotFoundError, match=r"best_\*"):
        find_sample_factory_checkpoint(str(empty), "best")


def _refused(sd):
    from aerial_gym_simulator_amd.utils.policy import recurrent_arrays_from_state_dict

    with pytest.raises((ValueError, KeyError)) as e:
        recurrent_arrays_from_state_dict(sd)
    return str(e.value)


def test_loader_refuses_other_structures_by_key():
    net = _small()
    base = ref.sf_state_dict(net)
    H = 32
    lstm = dict(base)
    for name in ("weight_ih_l0", "weight_hh_l0"):
        lstm["core.core." + name] = torch.zeros(4 * H, H)
    for name in ("bias_ih_l0", "bias_hh_l0"):
        lstm["core.core." + name] = torch.zeros(4 * H)
    msg = _refused(lstm)
    assert "core.core.weight_ih_l0" in msg and "LSTM" in msg
    assert "core.core.weight_ih_l1" in _refused(dict(base, **{"core.core.weight_ih_l1": torch.zeros(3 * H, H)}))
    assert "decoder.mlp.0.weight" in _refused(dict(base, **{"decoder.mlp.0.weight": torch.zeros(H, H)}))
    assert "encoder.encoders.obs.conv_head.0.weight" in _refused(dict(base, **{"encoder.encoders.obs.conv_head.0.weight": torch.zeros(8, 1, 3, 3)}))
    actor_enc = {k.replace("encoder.", "actor_encoder.", 1): v for k, v in base.items()}
    assert "actor_encoder.encoders.obs.mlp_head.0.weight" in _refused(actor_enc)
    assert "mlp_head.1" in _refused(dict(base, **{"encoder.encoders.obs.mlp_head.1.weight": torch.zeros(H)}))
    two = dict(base, **{"encoder.encoders.depth.mlp_head.0.weight": torch.zeros(H, 9), "encoder.encoders.depth.mlp_head.0.bias": torch.zeros(H)})
    assert "depth" in _refused(two)
    missing = dict(base)
    del missing["core.core.bias_hh_l0"]
    assert "core.core.bias_hh_l0" in _refused(missing)
    missing = dict(base)
    del missing["action_parameterization.distribution_linear.weight"]
    assert "action_parameterization.distribution_linear.weight" in _refused(missing)


@pytest.mark.parametrize("entry,value", [("rnn_type", "lstm"), ("rnn_num_layers", 2), ("nonlinearity", "tanh"), ("decoder_mlp_layers", [64]),
                                         ("continuous_tanh_scale", 1.0), ("obs_subtract_mean", 0.5), ("obs_scale", 255.0)])
def test_loader_refuses_config_entries_by_name(tmp_path, entry, value):
    from aerial_gym_simulator_amd.utils.policy import RecurrentActor

    ckdir = ref.write_experiment(tmp_path, "exp", {"best_1.pth": ref.sf_state_dict(_small())}, dict(ref.SF_CONFIG, **{entry: value}))
    with pytest.raises(ValueError, match=entry):
        RecurrentActor.from_sample_factory_checkpoint(ckdir, device="cpu")


def test_check_limits_and_lds_bytes():
    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd.utils.policy import check_recurrent_dims

    # (the encoder's two ping-pong widths + 7 H) x 32 envs x 4 bytes: 81 -> 88 and 128 share buffer 0, 256 and 64 buffer 1
    assert check_recurrent_dims([81, 256, 128, 64], 64, 8) == (128 + 256 + 7 * 64) * 128
    assert check_recurrent_dims([1, 32], 32, 1) == (8 + 32 + 7 * 32) * 128
    assert check_recurrent_dims([8, 32], 160, 128) == (8 + 32 + 7 * 160) * 128 <= 160 * 1024  # the largest H
    for dims, hidden, head, text in (([8, 32], 192, 8, "177152"), ([8, 512, 512], 64, 8, "188416"), ([81, 48], 64, 8, "48"), ([81, 64], 48, 8, "48"),
                                     ([81, 64], 544, 8, "544"), ([81, 64], 0, 8, "hidden size 0"), ([81, 64], 64, 129, "129"),
                                     ([81, 64], 64, 0, "head width 0"), ([0, 64], 64, 8, "input width 0"), ([513, 64], 64, 8, "513"),
                                     ([81, 1024], 64, 8, "1024"), ([81] + [32] * (_lib.POLICY_MAX_LAYERS - 1), 64, 8, "num_encoder_layers = 7"),
                                     ([81], 64, 8, "num_encoder_layers = 0")):
        with pytest.raises(ValueError, match=re.escape(text)):
            check_recurrent_dims(dims, hidden, head)
    assert check_recurrent_dims([81] + [32] * (_lib.POLICY_MAX_LAYERS - 2), 64, 8) > 0
    net = _small()
    with pytest.raises(ValueError, match="65 actions"):
        _actor(dict(net, head_weight=np.zeros((130, 32), np.float32), head_bias=np.zeros(130, np.float32)))
    with pytest.raises(ValueError, match="odd"):
        _actor(dict(net, head_weight=np.zeros((5, 32), np.float32), head_bias=np.zeros(5, np.float32)))
    with pytest.raises(ValueError, match="activation"):
        _actor(dict(net, activation="tanh"))


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8])
def test_hidden_state_semantics_on_the_cpu_path(dtype):
    net = _small()
    g = _gen(20)
    n = 6
    obs = [torch.rand((n, 9), generator=g) for _ in range(3)]
    free = _actor(net)
    assert free.hidden is None
    free(obs[0])
    assert tuple(free.hidden.shape) == (n, 32) and bool((free.hidden != 0).all())
    h1 = free.hidden.clone()
    a_free, h2_free = free(obs[1]).clone(), free.hidden.clone()
    assert not torch.equal(h1, h2_free)
    fresh = _actor(net)
    a_zero, h2_zero = fresh(obs[1]).clone(), fresh.hidden.clone()  # the second observation from a zero state
    d0 = torch.tensor([0, 1, 0, 0, 1, 0]).to(dtype)
    d1 = torch.tensor([0, 0, 0, 1, 1, 0]).to(dtype)
    for done, rows in ((d0, [1, 4]), ((d0,), [1, 4]), ((d0, d1), [1, 3, 4])):
        keep = [i for i in range(n) if i not in rows]
        before = _actor(net)
        before(obs[0])
        a = before(obs[1], done=done).clone()
        assert torch.equal(a[rows], a_zero[rows]) and torch.equal(before.hidden[rows], h2_zero[rows])
        assert torch.equal(a[keep], a_free[keep]) and torch.equal(before.hidden[keep], h2_free[keep])
        after = _actor(net)
        after(obs[0])
        a = after(obs[1], done=done, reset="after").clone()
        assert torch.equal(a, a_free) and bool((after.hidden[rows] == 0).all()) and torch.equal(after.hidden[keep], h2_free[keep])
    # reset(ids) zeroes rows of the live tensor; the tensor object stays
    live = free.hidden
    free.reset(torch.tensor([0, 5]))
    assert free.hidden is live and bool((live[[0, 5]] == 0).all()) and torch.equal(live[1:5], h2_free[1:5])
    # another batch size raises unless reset() was called
    with pytest.raises(ValueError, match="reset"):
        free(torch.rand((4, 9), generator=g))
    free.reset()
    assert bool((live == 0).all())
    free(torch.rand((4, 9), generator=g))
    assert tuple(free.hidden.shape) == (4, 32)
    # refusals of the call
    with pytest.raises(ValueError, match=r"float32 \[N, 9\]"):
        free(torch.zeros((4, 8)))
    with pytest.raises(ValueError, match="done"):
        free(torch.zeros((4, 9)), done=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="done"):
        free(torch.zeros((4, 9)), done=torch.zeros(5, dtype=torch.bool))
    with pytest.raises(ValueError, match="three|3 tensors"):
        free(torch.zeros((4, 9)), done=(torch.zeros(4, dtype=torch.bool),) * 3)
    with pytest.raises(ValueError, match="reset"):
        free(torch.zeros((4, 9)), reset="during")
    # a refused call leaves the state and the step count as they were
    h_before, step_before = free.hidden.clone(), free.step
    with pytest.raises(ValueError, match="eps"):
        free(torch.ones((4, 9)), sample=True)
    assert torch.equal(free.hidden, h_before) and free.step == step_before


def test_the_deepest_encoder_the_check_admits_runs_on_the_cpu_path():
    from aerial_gym_simulator_amd import _lib

    depth = _lib.POLICY_MAX_LAYERS - 2
    net = ref.random_net([19] + [32] * depth, 32, 3, _gen(25))
    actor = _actor(net)
    assert len(actor.enc_weights) == depth == 6
    obs = torch.rand((5, 19), generator=_gen(26))
    want = ref.step64(net, obs, torch.zeros(5, 32), torch.zeros(5, 32), fn=ref.FN_TORCH)
    actor(obs)
    assert float(((actor.mean.double() - want["mean"]).abs() / want["err_mean"]).max()) <= 1.0
    assert float((actor.mean.double() - want["mean"]).abs().max()) < 1e-5


def test_sampling_and_clamp_on_the_cpu_path():
    g = _gen(30)
    for adaptive in (True, False):
        net = _small(_gen(31), adaptive=adaptive)
        actor = _actor(net)
        obs, eps = torch.rand((7, 9), generator=g) * 4 - 2, torch.randn((7, 3), generator=g) * 3
        got = actor(obs, sample=True, eps=eps).clone()
        want = actor.mean + eps * torch.exp(actor.logstd_out)
        assert torch.allclose(got, want, rtol=0, atol=1e-6) and float(got.abs().max()) > 1
        if not adaptive:
            assert torch.equal(actor.logstd_out, torch.from_numpy(net["logstd"]).expand(7, 3))
        actor.reset()
        clamped = actor(obs, sample=True, clamp=True, eps=eps)
        assert torch.equal(clamped, got.clamp(-1, 1))


@pytest.mark.parametrize("which", ["sim2real", "dce"])
def test_drop_in_classes(tmp_path, which):
    import aerial_gym  # noqa: F401

    if which == "sim2real":
        from aerial_gym.sim2real.nn_inference_class import Sim2RealInferenceClass as cls
    else:
        from aerial_gym.examples.dce_rl_navigation.sf_inference_class import NN_Inference_Class as cls
    from aerial_gym_simulator_amd.utils.policy import SampleFactoryInference

    assert issubclass(cls, SampleFactoryInference)
    key = "observations" if which == "sim2real" else "obs"
    nets = [_small(_gen(40)), _small(_gen(41))]
    files = {"best_000000001_1_reward_1.0.pth": ref.sf_state_dict(nets[0], key), "checkpoint_000000002_2.pth": ref.sf_state_dict(nets[1], key)}
    ref.write_experiment(tmp_path, "nav", files, ref.SF_CONFIG)
    cfg = types.SimpleNamespace(train_dir=str(tmp_path), experiment="nav", load_checkpoint_kind="best", eval_deterministic=True, device="cpu")
    model = cls(5, 3, 9, cfg)
    assert tuple(model.rnn_states.shape) == (5, 32) and bool((model.rnn_states == 0).all())
    g = _gen(42)
    obs = torch.rand((5, 9), generator=g)
    a = model.get_action({key: obs})
    want = ref.step64(nets[0], obs, torch.zeros(5, 32), torch.zeros(5, 32))
    assert tuple(a.shape) == (5, 3) and float((a.double() - want["mean"]).abs().max()) < 1e-5
    assert model.rnn_states is model.actor.hidden and float((model.rnn_states.double() - want["hidden"]).abs().max()) < 1e-5
    model.reset(torch.tensor([1, 3]))
    assert bool((model.rnn_states[[1, 3]] == 0).all()) and bool((model.rnn_states[[0, 2, 4]] != 0).all())
    assert isinstance(model.get_action({key: obs}, get_np=True), np.ndarray)
    assert tuple(model.get_action({key: obs}, get_robot_zero=True).shape) == (3,)
    # a dict cfg; 'latest' is the default kind; sampling by default
    latest = cls(5, 3, 9, {"train_dir": str(tmp_path), "experiment": "nav", "device": "cpu"})
    assert np.array_equal(latest.actor.w_hh, nets[1]["w_hh"]) and not latest.eval_deterministic
    s = latest.get_action({key: obs})
    assert not torch.equal(s, latest.actor.mean)
    with pytest.raises(ValueError, match="9 observations to 3 actions"):
        cls(5, 4, 9, cfg)
    with pytest.raises(ValueError, match="experiment"):
        cls(5, 3, 9, {"train_dir": str(tmp_path)})


def test_header_and_mirrors():
    from aerial_gym_simulator_amd import _lib

    with open(os.path.join(ROOT, "include", "aerial_gym_hip.h")) as f:
        header = f.read()
    symbols = ("agx_recurrent_check", "agx_recurrent_create", "agx_recurrent_set_input_norm", "agx_recurrent_set_logstd", "agx_recurrent_act",
               "agx_recurrent_noise", "agx_recurrent_destroy")
    declared = set(re.findall(r"^int (agx_recurrent_\w+)\(", header, re.M))
    assert declared == set(symbols) == {s for s in _lib.EXPORTED_SYMBOLS if s.startswith("agx_recurrent_")}
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in symbols)
    version = int(re.search(r"#define AGX_ABI_VERSION (\d+)", header).group(1))
    assert version == _lib.ABI_VERSION == lib.agx_abi_version() == 25
    assert _lib.MATH_SIGMOID == 6 and _lib.MATH_TANH == 7 and "AGX_MATH_SIGMOID = 6" in header and "AGX_MATH_TANH = 7" in header
    assert _lib.POLICY_RESET_AFTER == 4 and "AGX_POLICY_RESET_AFTER = 4" in header
    assert (_lib.POLICY_SAMPLE | _lib.POLICY_CLAMP) & _lib.POLICY_RESET_AFTER == 0
    for site in ("sf_inference_class.py:80-101", "nn_inference_class.py:77-101"):
        assert site in header
    # the fixture: weights only
    net = ref.load_fixture()
    assert [w.shape for w in net["enc_weights"]] == [(256, 81), (128, 256), (64, 128)] and net["w_ih"].shape == (192, 64)
    assert net["head_weight"].shape == (8, 64) and os.path.getsize(ref.FIXTURE) < 400 * 1024
