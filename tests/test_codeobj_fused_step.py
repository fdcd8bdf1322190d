"""CPU: the shape of the single-launch position-step kernels, read from the gfx950 code object (no GPU needed).

k_position_step_fused<AGX_STEP_ANY> runs two waves per workgroup -- the step wave and the helper wave that takes the reset, the
refresh and the observation -- with a small static LDS area for the hand-off and exactly one workgroup barrier on either wave's
path; the NONE instance and k_env_step_quad_position (the first of the two launches) stay one-wave workgroups without LDS
(DESIGN.md section 3.2)."""
import os
import re
import subprocess
import tempfile

import pytest

import codeobj
from aerial_gym_simulator_amd import _build

pytestmark = pytest.mark.skipif(not codeobj.tools_available(), reason="objcopy / ROCm LLVM tools not found")

LDS_BUDGET = 2048  # bytes: the hand-off is 5 words per lane of the step wave (1280)
ANY, NONE = "k_position_step_fused<1>", "k_position_step_fused<2>"  # AGX_STEP_ANY = 1, AGX_STEP_NONE = 2


@pytest.fixture(scope="module")
def meta():
    assert os.path.exists(_build.LIB_PATH), "build the library first (python -m aerial_gym_simulator_amd._build)"
    return codeobj.kernel_metadata(_build.LIB_PATH)


@pytest.fixture(scope="module")
def disassembly():
    """{mangled kernel name: [instruction lines]} of the dynamics translation unit"""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dyn.co")
        obj = os.path.join(_build.LIB_DIR, "agx_dynamics.o")
        assert os.path.exists(obj), "build the library first (python -m aerial_gym_simulator_amd._build)"
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
        subprocess.run([os.path.join(codeobj.LLVM_BIN, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                        f"--targets={codeobj.TARGET}", f"--output={co}"], check=True)
        asm = subprocess.run([os.path.join(codeobj.LLVM_BIN, "llvm-objdump"), "-d", co], check=True, capture_output=True,
                             text=True).stdout
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and "\t" in line:
            cur.append(line.split("//")[0].strip())
    return out


def _one(meta, part):
    ks = {n: r for n, r in meta.items() if part in n}
    assert len(ks) == 1, (part, list(ks))
    return next(iter(ks.values()))


def _body(disassembly, part):
    ks = [v for k, v in disassembly.items() if part in k]
    assert len(ks) == 1, part
    assert any(i.startswith("s_endpgm") for i in ks[0])
    return ks[0]


def test_any_instance_runs_two_waves_per_workgroup(meta, disassembly):
    r = _one(meta, ANY)
    assert r["max_flat_workgroup_size"] == 128, r
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert 0 < r["group_segment_fixed_size"] <= LDS_BUDGET, r
    body = _body(disassembly, "k_position_step_fusedILi1E")
    assert not [i for i in body if "scratch_" in i]
    # one barrier in the step wave's code, one in the helper wave's: the branch between them is on a scalar (the wave index)
    assert sum(i.startswith("s_barrier") for i in body) == 2
    # the proof slot's wave reduction does not go through the LDS crossbar: what is left are the 7 x 6 stages of the folding
    # workgroup's butterfly (once per launch)
    assert sum("ds_bpermute" in i for i in body) <= 42


def test_none_and_two_launch_kernels_stay_one_wave_without_lds(meta, disassembly):
    for part, mangled in ((NONE, "k_position_step_fusedILi2E"), ("k_env_step_quad_position", "k_env_step_quad_positionE")):
        r = _one(meta, part)
        assert r["max_flat_workgroup_size"] == 64 and r["group_segment_fixed_size"] == 0, (part, r)
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (part, r)
        body = _body(disassembly, mangled)
        assert not [i for i in body if "scratch_" in i or i.startswith("s_barrier")], part
