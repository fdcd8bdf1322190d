"""CPU: the open-loop rollout's C ABI surface (agx_env_rollout, AgxRolloutRecord) and the argument checks of EnvManager.rollout on a
device="cpu" env (no compute calls, no GPU).  The bit-identity with the eager loop is tests/test_gpu_rollout.py."""
import ctypes
import os
import re
import subprocess

import pytest
import torch
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "aerial_gym_hip.h")


def test_header_declares_the_entry_and_the_record():
    text = open(HEADER).read()
    assert re.search(r"\bint agx_env_rollout\(const AgxRobotParams \*\w+, const AgxEnvBuffers \*\w+, int \w+, const float \*\w+, int actions_per_step,\s*"
                     r"int steps, int substeps, const int \*substeps_per_step, const AgxRolloutRecord \*\w+, int \*first_crash_step,\s*void \*stream\);", text)
    assert "typedef struct AgxRolloutRecord {" in text and "#define AGX_ROLLOUT_MAX_CHANNELS 32" in text
    # the reference call sites the entry replaces are cited next to it
    at = text.index("Open-loop rollout")
    block = text[at:text.index("int agx_env_rollout(")]
    assert "env_manager.py:399-432" in block and "examples/sys_id.py:56-90" in block


def test_abi_version_stays_25():
    from aerial_gym_simulator_amd import _lib

    text = open(HEADER).read()
    assert int(re.search(r"#define AGX_ABI_VERSION (\d+)", text).group(1)) == 25 == _lib.ABI_VERSION
    assert _lib.load().agx_abi_version() == 25


def test_record_struct_matches_header(tmp_path):
    """AgxRolloutRecord: size and the offset of every member in C == the ctypes mirror's; the ids and the channel bound too."""
    from aerial_gym_simulator_amd import _lib

    names = [name for name, _ in _lib.AgxRolloutRecord._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "aerial_gym_hip.h"\nint main(){printf("%zu\\n", sizeof(AgxRolloutRecord));'
           + "".join('printf("%%zu\\n", offsetof(AgxRolloutRecord, %s));' % name for name in names)
           + 'printf("%d %d %d %d %d\\n", AGX_ROLLOUT_MAX_CHANNELS, AGX_REC_STATE, AGX_REC_DERIVED, AGX_REC_THRUST, AGX_REC_CRASH);return 0;}')
    exe = str(tmp_path / "agx_rollout_layout")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src, text=True, check=True)
    out = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_lib.AgxRolloutRecord)
    assert out[1:1 + len(names)] == [getattr(_lib.AgxRolloutRecord, name).offset for name in names]
    assert out[1 + len(names):] == [_lib.ROLLOUT_MAX_CHANNELS, _lib.REC_STATE, _lib.REC_DERIVED, _lib.REC_THRUST, _lib.REC_CRASH]
    assert names == ["out", "channels", "reserved", "source", "component"]


def test_library_exports_the_symbol():
    from aerial_gym_simulator_amd import _build, _lib

    lib = ctypes.CDLL(_build.build_library())
    assert hasattr(lib, "agx_env_rollout")
    assert "agx_env_rollout" in _lib.EXPORTED_SYMBOLS
    res, args = _lib._SIGNATURES["agx_env_rollout"]
    assert res is ctypes.c_int and len(args) == 11


def test_record_keys_cover_the_documented_set():
    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd.rollout import RECORD_KEYS

    assert set(RECORD_KEYS) == {"robot_position", "robot_orientation", "robot_linvel", "robot_angvel", "robot_body_linvel", "robot_body_angvel",
                                "robot_euler_angles", "robot_vehicle_orientation", "robot_vehicle_linvel", "motor_thrusts", "crashes"}
    # state rows follow robot_state_tensor, derived rows the robot's derived tensor
    assert RECORD_KEYS["robot_orientation"] == (_lib.REC_STATE, 3, 4) and RECORD_KEYS["robot_angvel"] == (_lib.REC_STATE, 10, 3)
    assert RECORD_KEYS["robot_euler_angles"] == (_lib.REC_DERIVED, 0, 3) and RECORD_KEYS["robot_body_angvel"] == (_lib.REC_DERIVED, 13, 3)
    assert RECORD_KEYS["motor_thrusts"] == (_lib.REC_THRUST, 0, None) and RECORD_KEYS["crashes"] == (_lib.REC_CRASH, 0, 1)


@pytest.fixture(scope="module")
def cpu_env():
    from aerial_gym_simulator_amd.sim.sim_builder import SimBuilder

    return SimBuilder().build_env(sim_name="base_sim", env_name="empty_env", robot_name="base_quadrotor", controller_name="lee_position_control",
                                  device="cpu", args=None, num_envs=6, headless=True, use_warp=False)


def test_argument_checks_on_a_cpu_env(cpu_env):
    env, N, A = cpu_env, 6, 4
    a = torch.zeros(N, A)
    before = {k: v.clone() for k, v in env.global_tensor_dict.items() if isinstance(v, torch.Tensor)}
    with pytest.raises(TypeError, match="float32 tensor"):
        env.rollout([[0.0] * A] * N, steps=2)
    with pytest.raises(ValueError, match="must be float32"):
        env.rollout(a.double(), steps=2)
    with pytest.raises(ValueError, match="`steps` is required"):
        env.rollout(a)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="steps must be an integer >= 1"):
            env.rollout(a, steps=bad)
    with pytest.raises(ValueError, match=r"held action tensor is \[6, 4\]"):
        env.rollout(torch.zeros(N, A + 1), steps=2)
    with pytest.raises(ValueError, match=r"held action tensor is \[6, 4\]"):
        env.rollout(torch.zeros(N + 1, A), steps=2)
    with pytest.raises(ValueError, match=r"a step schedule is \[T, 6, 4\]"):
        env.rollout(torch.zeros(3, N, A + 2))
    with pytest.raises(ValueError, match=r"a step schedule is \[T, 6, 4\]"):
        env.rollout(torch.zeros(0, N, A))
    with pytest.raises(ValueError, match="steps=4 with a schedule of 3 steps"):
        env.rollout(torch.zeros(3, N, A), steps=4)
    with pytest.raises(ValueError, match=r"expected \[6, 4\] or \[T, 6, 4\]"):
        env.rollout(torch.zeros(N * A), steps=2)
    with pytest.raises(ValueError, match="must be contiguous"):
        env.rollout(torch.zeros(A, N).t(), steps=2)
    with pytest.raises(ValueError, match="'robot_pose' cannot be recorded"):
        env.rollout(a, steps=2, record=("robot_position", "robot_pose"))
    with pytest.raises(ValueError, match="named twice"):
        env.rollout(a, steps=2, record=("robot_linvel", "robot_linvel"))
    from aerial_gym_simulator_amd.rollout import RECORD_KEYS

    with pytest.raises(ValueError, match="34 recorded channels, at most 32"):  # every key of a four-motor robot at once
        env.rollout(a, steps=2, record=tuple(RECORD_KEYS))
    with pytest.raises(TypeError, match="tuple of keys"):
        env.rollout(a, steps=2, record="robot_position")
    with pytest.raises(TypeError, match="`out` is the RolloutRecord"):
        env.rollout(a, steps=2, out={})
    for k, v in before.items():
        assert torch.equal(env.global_tensor_dict[k], v), k


def test_out_must_match_shape_and_keys(cpu_env):
    from aerial_gym_simulator_amd.rollout import RolloutRecord

    env, a = cpu_env, torch.zeros(6, 4)
    rec = RolloutRecord(("robot_position", "crashes"), (3, 1), 5, 6, "cpu")
    assert rec.data.shape == (5, 4, 6) and rec["robot_position"].shape == (5, 6, 3) and rec["crashes"].shape == (5, 6, 1)
    assert rec["robot_position"].data_ptr() == rec.data.data_ptr()  # a permuted view of the component-major storage
    assert rec.first_crash_step.dtype == torch.int32 and rec.first_crash_step.shape == (6,)
    for kw in (dict(steps=4, record=("robot_position", "crashes")), dict(steps=5, record=("robot_position",)),
               dict(steps=5, record=("crashes", "robot_position"))):
        with pytest.raises(ValueError, match=r"rollout\(out=\)"):
            env.rollout(a, out=rec, **kw)


def test_no_device_message_is_the_existing_one(cpu_env):
    """valid arguments on a CPU env: the refusal every stepping entry gives there (EnvManager._require_device)"""
    with pytest.raises(RuntimeError) as e:
        cpu_env.rollout(torch.zeros(6, 4), steps=3, record=("robot_position",))
    with pytest.raises(RuntimeError) as e_step:
        cpu_env.step(torch.zeros(6, 4))
    assert str(e.value) == str(e_step.value) and "has no CPU fallback" in str(e.value)
