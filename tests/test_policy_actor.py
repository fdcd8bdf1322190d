"""CPU: the policy actor's C-ABI surface, the rl_games checkpoint loader, the CPU path of ActorMLP, the reference's MLP class under
its own import path and the packing of the padded last layer.  The kernel itself: tests/test_gpu_policy_actor.py."""
import ctypes
import os
import re

import numpy as np
import policy_ref
import pytest
import torch
import torch.nn.functional as F
from conftest import ROOT

POLICY_SYMBOLS = ("agx_policy_check", "agx_policy_create", "agx_policy_set_input_norm", "agx_policy_set_logstd", "agx_policy_act",
                  "agx_policy_noise", "agx_policy_destroy")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_header_lib_and_library_agree_on_the_policy_entry_points():
    from aerial_gym_simulator_amd import _build, _lib

    assert "agx_policy.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "agx_policy.hip"))
    header = open(os.path.join(ROOT, "include", "aerial_gym_hip.h")).read()
    declared = {s for s in re.findall(r"\b(agx_[a-z_0-9]+)\s*\(", header) if s.startswith("agx_policy_")}
    assert declared == set(POLICY_SYMBOLS) == {s for s in _lib.EXPORTED_SYMBOLS if s.startswith("agx_policy_")}
    lib = ctypes.CDLL(_build.build_library())
    for name in POLICY_SYMBOLS:
        assert hasattr(lib, name), name
    version = int(re.search(r"#define AGX_ABI_VERSION (\d+)", header).group(1))
    assert version == _lib.ABI_VERSION == _lib.load().agx_abi_version() and version >= 24
    # the call sites the entry points replace are cited, and the constants mirror the header
    assert "rl_games_inference.py:7-48" in header
    for name, value in (("AGX_POLICY_MAX_LAYERS", _lib.POLICY_MAX_LAYERS), ("AGX_POLICY_MAX_WIDTH", _lib.POLICY_MAX_WIDTH)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value
    enums = dict(re.findall(r"(AGX_POLICY_[A-Z]+) = (\d+)", header))
    assert {k: int(v) for k, v in enums.items()} == {"AGX_POLICY_NONE": _lib.POLICY_NONE, "AGX_POLICY_ELU": _lib.POLICY_ELU,
                                                      "AGX_POLICY_RELU": _lib.POLICY_RELU, "AGX_POLICY_SAMPLE": _lib.POLICY_SAMPLE,
                                                      "AGX_POLICY_CLAMP": _lib.POLICY_CLAMP}


def test_limits_are_checked_on_the_host_and_name_the_number():
    from aerial_gym_simulator_amd.utils.policy import check_dims

    assert check_dims([13, 256, 128, 64, 4]) == (256 + 128) * 32 * 4  # activations 16 | 256 | 128 | 64 | 32: even 128, odd 256
    assert check_dims([15, 512, 512, 4]) == 128 * 1024
    assert check_dims([13, 4]) == (16 + 32) * 32 * 4
    assert check_dims([512] + [32] * 7 + [512]) > 0  # eight layers
    for dims, number in (([13, 48, 4], "48"), ([13] + [32] * 8 + [4], "9"), ([513, 32, 4], "513"), ([13, 544, 4], "544"), ([0, 4], "0"),
                         ([13, 32, 513], "513"), ([13, 16, 4], "16")):
        with pytest.raises(ValueError, match=number):
            check_dims(dims)


def test_rl_games_checkpoint_loads_to_the_same_arrays(tmp_path):
    from aerial_gym_simulator_amd.utils.policy import NORM_CLIP, ActorMLP

    ws, bs, logstd = policy_ref.load_actor("attitude")
    g = _gen(1)
    mean, var = torch.randn(13, generator=g).numpy(), (torch.rand(13, generator=g) + 0.1).numpy()
    for running in (None, (mean, var)):
        path = policy_ref.write_checkpoint(tmp_path / f"actor_{running is not None}.pth", policy_ref.rl_games_state_dict(ws, bs, logstd, running))
        actor = ActorMLP.from_rl_games_checkpoint(path, device="cpu")
        assert actor.dims == [13, 256, 128, 64, 4] and actor.activation == "elu"
        assert all(np.array_equal(a, b) for a, b in zip(actor.weights, ws)) and all(np.array_equal(a, b) for a, b in zip(actor.biases, bs))
        assert np.array_equal(actor.logstd, logstd)
        if running is None:
            assert actor.input_norm is None
        else:
            m, d, clip = actor.input_norm
            assert np.array_equal(m, mean) and clip == NORM_CLIP == 5.0
            assert d.dtype == np.float32 and np.array_equal(d, np.sqrt((var + np.float32(1e-5)).astype(np.float32)).astype(np.float32))


def test_checkpoints_the_actor_cannot_run_are_refused_by_name(tmp_path):
    from aerial_gym_simulator_amd.examples.rl_games_example.rl_games_inference import MLP
    from aerial_gym_simulator_amd.utils.policy import ActorMLP

    ws, bs, logstd = policy_ref.load_actor("attitude")
    good = policy_ref.rl_games_state_dict(ws, bs, logstd)

    def load(sd, name):
        return ActorMLP.from_rl_games_checkpoint(policy_ref.write_checkpoint(tmp_path / name, sd), device="cpu")

    missing = {k: v for k, v in good.items() if not k.startswith("a2c_network.actor_mlp.2.")}
    with pytest.raises(KeyError, match=r"a2c_network\.actor_mlp\.2\.weight"):
        load(missing, "missing.pth")
    no_mu = {k: v for k, v in good.items() if k != "a2c_network.mu.bias"}
    with pytest.raises(KeyError, match=r"a2c_network\.mu\.bias"):
        load(no_mu, "no_mu.pth")
    g = _gen(2)
    with pytest.raises(ValueError, match="48"):
        load(policy_ref.rl_games_state_dict(*policy_ref.random_net([13, 48, 4], g), np.zeros(4, np.float32)), "w48.pth")
    with pytest.raises(ValueError, match="num_layers = 9"):
        load(policy_ref.rl_games_state_dict(*policy_ref.random_net([13] + [32] * 8 + [4], g), np.zeros(4, np.float32)), "nine.pth")
    with pytest.raises(ValueError, match="513"):
        load(policy_ref.rl_games_state_dict(*policy_ref.random_net([513, 32, 4], g), np.zeros(4, np.float32)), "in513.pth")
    with pytest.raises(ValueError, match=r"a2c_network\.rnn"):
        load(dict(good, **{"a2c_network.rnn.rnn.weight_ih_l0": torch.zeros(3, 3)}), "rnn.pth")
    with pytest.raises(ValueError, match=r"a2c_network\.sigma\.weight"):
        load(dict(good, **{"a2c_network.sigma.weight": torch.zeros(4, 64)}), "sigma_net.pth")
    with pytest.raises(KeyError, match="model"):
        torch.save({"state_dict": good}, str(tmp_path / "other.pth"))
        ActorMLP.from_rl_games_checkpoint(str(tmp_path / "other.pth"), device="cpu")
    path = policy_ref.write_checkpoint(tmp_path / "good.pth", good)
    with pytest.raises(ValueError, match="13 observations"):
        MLP(12, 4, path)
    with pytest.raises(ValueError, match="4 actions"):
        MLP(13, 3, path)
    assert MLP(13, 4, path).to("cpu").eval().actor.dims == [13, 256, 128, 64, 4]


@pytest.mark.parametrize("name", policy_ref.REAL_NETS)
def test_cpu_path_is_the_torch_actor_bit_for_bit(name):
    from aerial_gym_simulator_amd.utils.policy import ActorMLP

    ws, bs, logstd = policy_ref.load_actor(name)
    actor = ActorMLP.from_arrays(ws, bs, logstd=logstd, device="cpu")
    ref = policy_ref.Actor(ws, bs, logstd).eval()
    obs = torch.rand((97, actor.obs_dim), generator=_gen(3)) * 4 - 2
    with torch.no_grad():
        want = ref(obs)
        got = actor(obs)
    assert got.shape == (97, 4) and np.array_equal(policy_ref.bits(got), policy_ref.bits(want))
    assert np.array_equal(policy_ref.bits(actor.mean), policy_ref.bits(want))
    # the same computation, restated here: F.linear / F.elu
    x = obs
    for w, b in zip(ws[:-1], bs[:-1]):
        x = F.elu(F.linear(x, torch.from_numpy(w), torch.from_numpy(b)))
    assert np.array_equal(policy_ref.bits(F.linear(x, torch.from_numpy(ws[-1]), torch.from_numpy(bs[-1]))), policy_ref.bits(got))
    # out=, sampling from a given eps, clamping
    eps = torch.randn((97, 4), generator=_gen(4)) * 3
    out = torch.empty(97, 4)
    assert actor(obs, out=out, sample=True, clamp=True, eps=eps) is out
    plain = (want + eps * torch.exp(torch.from_numpy(logstd))).clamp(-1, 1)
    assert np.array_equal(policy_ref.bits(out), policy_ref.bits(plain)) and float(out.abs().max()) <= 1.0
    assert np.array_equal(policy_ref.bits(actor.mean), policy_ref.bits(want))  # the mean is the unsampled, unclamped one
    again = actor(obs)
    assert again.data_ptr() == got.data_ptr()  # one buffer per batch size
    with pytest.raises(ValueError, match="float32"):
        actor(obs.double())
    with pytest.raises(ValueError, match="logstd"):
        ActorMLP.from_arrays(ws, bs, device="cpu")(obs, sample=True, eps=eps)


def test_cpu_input_normalisation_and_clamp_equal_the_float32_statement():
    from aerial_gym_simulator_amd.utils.policy import ActorMLP

    ws, bs, logstd = policy_ref.load_actor("lmf2_velocity")
    g = _gen(5)
    mean, denom = (torch.randn(17, generator=g) * 2).numpy(), (torch.rand(17, generator=g) * 2 + 0.05).numpy()
    obs = (torch.rand((64, 17), generator=g) * 40 - 20)  # far beyond the clip on both sides
    xn = policy_ref.norm_f32(obs.numpy(), mean, denom, 5.0)
    assert (xn == 5.0).any() and (xn == -5.0).any() and (np.abs(xn) < 5.0).any()
    plain = ActorMLP.from_arrays(ws, bs, device="cpu")
    normed = ActorMLP.from_arrays(ws, bs, input_norm=(mean, denom, 5.0), device="cpu")
    with torch.no_grad():
        want = plain(torch.from_numpy(xn)).clone()
        got = normed(obs)
    assert np.array_equal(policy_ref.bits(got), policy_ref.bits(want))
    clamped = normed(obs, clamp=True)
    assert np.array_equal(policy_ref.bits(clamped), policy_ref.bits(np.clip(want.numpy(), np.float32(-1), np.float32(1))))
    for act, fn in (("relu", torch.relu), ("none", lambda v: v)):
        a = ActorMLP.from_arrays(ws, bs, activation=act, device="cpu")
        x = obs
        for w, b in zip(ws[:-1], bs[:-1]):
            x = fn(F.linear(x, torch.from_numpy(w), torch.from_numpy(b)))
        assert np.array_equal(policy_ref.bits(a(obs)), policy_ref.bits(F.linear(x, torch.from_numpy(ws[-1]), torch.from_numpy(bs[-1]))))


def test_alias_resolves_the_reference_import_path_to_the_same_class():
    import aerial_gym  # noqa: F401
    from aerial_gym.examples.rl_games_example.rl_games_inference import MLP as alias_mlp

    from aerial_gym_simulator_amd.examples.rl_games_example.rl_games_inference import MLP

    assert alias_mlp is MLP
    import aerial_gym.utils.policy as alias_policy

    from aerial_gym_simulator_amd.utils import policy

    assert alias_policy is policy


@pytest.mark.parametrize("shape", [(4, 64), (1, 13), (33, 17), (512, 512)])
def test_padded_last_layer_packs_and_unpacks_exactly(shape):
    from aerial_gym_simulator_amd.utils.policy import pack_layer
    from aerial_gym_simulator_amd.utils.vae.vae_image_encoder import unpack_weight

    out, fin = shape
    w = (torch.rand(shape, generator=_gen(6)) * 2 - 1).numpy()
    rows, k8 = -(-out // 32) * 32, -(-fin // 8) * 8
    packed = pack_layer(w, pad_rows_to=32)
    assert packed.shape == (k8 * rows,)
    grid = packed.reshape(k8, rows)  # [K8][Cout]
    assert np.array_equal(grid[:fin, :out], w.T)
    assert not grid[fin:].any() and not grid[:, out:].any()  # the k tail and the padding rows are zero
    back = unpack_weight(packed, (rows, fin))
    assert np.array_equal(back[:out].view(np.uint32), w.view(np.uint32)) and not back[out:].any()
