"""CPU: the kernel agx_env_step_kernel names is a kernel of the shipped code object (no GPU needed, nothing is launched).

agx_env_step and agx_env_step_kernel read ONE decision (csrc/agx_dynamics.hip: choose_env_step) -- the four-lanes-per-env position
kernel, the four-lanes-per-env sub-step loop, or k_env_step<M, CTRL, SINGLE, WIDE> -- and bench.py and the GPU tests take the name
for what was launched.  Here every motor count, every control law with the action count it takes, one and two sub-steps, one-wave
and 256-thread workgroups, with and without obstacles and with one non-zero drag coefficient: the name, without its
`_<threads>` suffix, must be an instance that exists in libaerialgym_hip.so, and the suffix the grid of that family."""
import ctypes as C
import os
import re

import pytest

import codeobj
from aerial_gym_simulator_amd import _build, _lib

pytestmark = pytest.mark.skipif(not codeobj.tools_available(), reason="objcopy / ROCm LLVM tools not found")

WRENCH, FULLY_ACTUATED, NONE = _lib.CTRL_IDS["wrench"], _lib.CTRL_IDS["fully_actuated"], _lib.CTRL_IDS["none"]


def _shipped_kernels():
    """{"k_env_step<4,1,true,true>", "k_env_step_quad_position", ...}: the demangled names without return type, namespace,
    parameter list and spaces"""
    assert os.path.exists(_build.LIB_PATH), "build the library first (python -m aerial_gym_simulator_amd._build)"
    out = set()
    for name in codeobj.kernel_metadata(_build.LIB_PATH):
        m = re.match(r"(?:void )?agx::(k_\w+(?:<[^>]*>)?)\(", name)
        if m:
            out.add(m.group(1).replace(" ", ""))
    return out


def test_env_step_kernel_names_a_shipped_kernel():
    lib, shipped = _lib.load(), _shipped_kernels()
    assert len([k for k in shipped if k.startswith("k_env_step<")]) == 108
    dummy = 0x1000  # never dereferenced: the entry point launches nothing
    seen, bad = {}, []
    for M in (4, 6, 8):
        for ctrl in sorted(_lib.CTRL_IDS.values()):
            A = M if ctrl == NONE else (7 if ctrl == FULLY_ACTUATED else 4)
            for k in (1, 2):
                if ctrl == WRENCH and k > 1:
                    continue  # an external controller is one launch per sub-step (agx_env_step refuses k > 1)
                for n in (64, 70000):
                    for variant in ("plain", "boxes", "drag"):
                        P = _lib.AgxRobotParams(num_motors=M, num_actions=A, controller=ctrl)
                        B = _lib.AgxEnvBuffers()
                        if variant == "boxes":
                            B.boxes, B.num_boxes = dummy, 3
                        if variant == "drag":
                            P.ang_drag_quadratic[1] = 0.25
                        buf = C.create_string_buffer(128)
                        assert lib.agx_env_step_kernel(P, B, n, k, None, buf, 128) == 0
                        name, threads = re.sub(r"\s+", "", buf.value.decode()).rsplit("_", 1)
                        case = (M, ctrl, k, n, variant, name)
                        if name not in shipped:
                            bad.append(case)
                        per_block_envs, block = (16, 64) if name.startswith("k_env_step_quad_") else ((64, 64) if n <= 65536 else (256, 256))
                        if int(threads) != -(-n // per_block_envs) * block:
                            bad.append(case + (threads,))
                        seen.setdefault(name.split("<")[0], set()).add(name)
    print({fam: len(names) for fam, names in seen.items()})
    assert not bad, bad
    # the cases reach every family: the position kernel, all nine sub-step loops, and one-lane instances of every law
    assert seen["k_env_step_quad_position"] == {"k_env_step_quad_position"}
    assert len(seen["k_env_step_quad_loop"]) == 9
    assert {int(x.split(",")[1]) for x in seen["k_env_step"]} == set(_lib.CTRL_IDS.values())
