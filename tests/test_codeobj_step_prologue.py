"""CPU: how the position-step kernels fetch their kernel arguments and inputs, read from the gfx950 code object (no GPU needed).

A wave of these kernels runs alone on its SIMD, so every `s_waitcnt lgkmcnt(0)` behind an s_load is a scalar-memory round trip it
sits out.  Each wave therefore fetches every argument field it uses as one batch at its top (csrc/agx_dyn_state.h: arg_pin) and
issues every input load before it waits for any; no access goes through a FLAT instruction, which counts on lgkmcnt as well as on
vmcnt.  The caps on the AGX_STEP_ANY instance are set against the parent of this change: 100 s_load and
82 `s_waitcnt lgkmcnt(0)` in its body (the LDS waits at the hand-off included, then as now)."""
import os
import re
import subprocess
import tempfile

import pytest

import codeobj
from aerial_gym_simulator_amd import _build

pytestmark = pytest.mark.skipif(not codeobj.tools_available(), reason="objcopy / ROCm LLVM tools not found")

ANY, NONE = "k_position_step_fusedILi1E", "k_position_step_fusedILi2E"  # AGX_STEP_ANY = 1, AGX_STEP_NONE = 2
TWO, RESET_OBS = "k_env_step_quad_positionE", "k_reset_masked_quad_obsE"
PARENT_ANY_S_LOAD, PARENT_ANY_LGKM_WAITS = 100, 82


def _kernels(asm):
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and "\t" in line:
            cur.append(line.split("//")[0].strip())
    return out


def _objdump(co):
    return subprocess.run([os.path.join(codeobj.LLVM_BIN, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout


@pytest.fixture(scope="module")
def product():
    """{mangled kernel name: [instruction lines]} of the dynamics translation unit of the product build"""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dyn.co")
        obj = os.path.join(_build.LIB_DIR, "agx_dynamics.o")
        assert os.path.exists(obj), "build the library first (python -m aerial_gym_simulator_amd._build)"
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
        subprocess.run([os.path.join(codeobj.LLVM_BIN, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                        f"--targets={codeobj.TARGET}", f"--output={co}"], check=True)
        return _kernels(_objdump(co))


@pytest.fixture(scope="module")
def stamped():
    """the same translation unit with -DAGX_STEP_STAMPS (what profiles/step_phase_probe.py builds as a variant library): the
    device side only, with the product's flags, as assembly text"""
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "dyn_stamps.s")
        src = "agx_dynamics.hip"
        subprocess.run([_build._hipcc()] + _build.FLAGS + _build.PER_SOURCE_FLAGS.get(src, []) +
                       ["-DAGX_STEP_STAMPS", "--cuda-device-only", "-S", "-I", _build.INCLUDE, "-x", "hip", os.path.join(_build.CSRC, src),
                        "-o", asm], check=True)
        out, cur = {}, None
        for line in open(asm):
            m = re.match(r"^(_Z\w+):", line)
            if m:
                cur = out.setdefault(m.group(1), [])
            elif cur is not None and line.startswith("\t") and not line.lstrip().startswith((".", ";")):
                cur.append(line.split(";")[0].strip())
        return out


def _body(kernels, part):
    ks = [v for k, v in kernels.items() if part in k]
    assert len(ks) == 1, part
    assert any(i.startswith("s_endpgm") for i in ks[0])
    return ks[0]


def _is_vector_load(i):
    return i.startswith(("global_load", "buffer_load", "flat_load", "scratch_load"))


def _is_lgkm_wait(i):
    return i.startswith("s_waitcnt") and "lgkmcnt" in i


def _is_clock_read(i):
    return i.startswith(("s_memtime", "s_memrealtime")) or ("s_getreg" in i and "SHADER_CYCLES" in i)


@pytest.mark.parametrize("part", [ANY, NONE, TWO, RESET_OBS])
def test_no_flat_instruction(product, part):
    assert not [i for i in _body(product, part) if i.startswith("flat_")], part


@pytest.mark.parametrize("part", [NONE, TWO])
def test_one_wave_kernels_fetch_arguments_once_and_inputs_in_one_batch(product, part):
    body = _body(product, part)
    first_load = next(k for k, i in enumerate(body) if _is_vector_load(i))
    first_wait = next(k for k, i in enumerate(body) if k > first_load and i.startswith("s_waitcnt") and "vmcnt" in i)
    between = body[first_load:first_wait]
    assert not [i for i in between if i.startswith("s_load")], (part, [i for i in between if i.startswith("s_load")])
    # one wait for the argument batch, one allowed for a dependent implicit-argument fetch
    waits = [i for i in body[:first_load] if _is_lgkm_wait(i)]
    assert len(waits) <= 2, (part, waits)
    # (the input batch is a batch: a dozen loads or more before the first wait on any of them)
    assert sum(_is_vector_load(i) for i in between) >= 12, (part, between)


@pytest.mark.parametrize("part", [NONE, TWO])
def test_one_wave_kernels_spill_no_scalar_register(part):
    assert os.path.exists(_build.LIB_PATH), "build the library first (python -m aerial_gym_simulator_amd._build)"
    meta = {n: r for n, r in codeobj.kernel_metadata(_build.LIB_PATH).items()
            if ("k_position_step_fused<2>" if part == NONE else "k_env_step_quad_position(") in n}
    assert len(meta) == 1, list(meta)
    r = next(iter(meta.values()))
    assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["sgpr_count"] <= 102 + 6, r  # 102 allocatable + VCC, FLAT_SCRATCH, XNACK_MASK as the metadata counts them


def test_any_instance_halves_its_scalar_round_trips(product):
    body = _body(product, ANY)
    waits = sum(i.startswith("s_waitcnt") and "lgkmcnt(0)" in i for i in body)
    loads = sum(i.startswith("s_load") for i in body)
    print(f"k_position_step_fused<AGX_STEP_ANY>: {loads} s_load (parent {PARENT_ANY_S_LOAD}), {waits} s_waitcnt lgkmcnt(0) "
          f"(parent {PARENT_ANY_LGKM_WAITS})")
    assert waits <= PARENT_ANY_LGKM_WAITS // 2, waits
    assert loads < PARENT_ANY_S_LOAD, loads


def test_store_phases_hold_no_scalar_fetch(product):
    """ANY: behind either wave's barrier every store of that wave comes before the next s_load of the listing -- no pointer is
    fetched in front of a group of stores.  The helper wave stores a resetting env (bounds 6, state 13, gains 12, motors 16,
    sim_steps, episode count), the derived tensors (5) and the observation (4): 58; the step wave its state (4) and thrust, the wrench (2),
    both action copies, sim_steps, reward, reset mask, both flags and the two halves of the proof slot: 16, followed in the
    listing by the 7 stores of the folding workgroup's record (proof_fold_publish), which needs no fetch of its own any more."""
    body = _body(product, ANY)
    barriers = [k for k, i in enumerate(body) if i.startswith("s_barrier")]
    assert len(barriers) == 2
    counts = []
    for b in barriers:
        nxt = next((k for k, i in enumerate(body) if k > b and (i.startswith("s_load") or i.startswith("s_barrier"))), len(body))
        counts.append(sum(i.startswith(("global_store", "buffer_store")) for i in body[b:nxt]))
    print("stores behind a barrier and before the next s_load:", counts)
    assert sorted(counts) == [16 + 7, 58], counts


def test_product_build_reads_no_clock_and_stamped_variant_does(product, stamped):
    for part in (ANY, NONE):
        assert not [i for i in _body(product, part) if _is_clock_read(i)], part
        assert sum(_is_clock_read(i) for i in _body(stamped, part)) >= 8, part  # six phase stamps + two wall-clock stamps per wave
    # the stamps are a compile-time switch: nothing but the stamped kernels' own code differs, and the product's instruction
    # stream of these kernels holds no trace of it
    assert "g_step_stamps" not in "".join(product.keys())
