"""GPU: `body_force`, the IMU's only dynamic input -- the net applied force of the LAST physics sub-step of an env step, drag and
disturbance included -- as each of the three env-step kernel families stores it, against the CPU oracle: k calls of orc.substep,
the last call's body_wrench[:, :3].  The gate is the one test_gpu_dynamics.py holds wrench_cmd and the per-sub-step outputs to
against the oracle: bit for bit (EXACT).

Every case names the family it means to reach and asserts it through agx_env_step_kernel:
  * the fused lane-quad position step: 4 motors, position control, k = 1 (16 envs per workgroup: n = 83 leaves a partial one);
  * the lane-quad sub-step loop: the same airframe with k = 2 and k = 10, an octarotor, a velocity-controlled quadrotor;
  * the one-lane family: no controller, or an airframe with drag (the lane-quad kernels carry neither), and every batch above
    65 536 envs -- agx_common.h `inline int pick_block(int n) { return n <= 65536 ? 64 : 256; }`: 65 537 is the smallest n with
    256-thread workgroups, the case runs 65 537 + 3."""
import ctypes as C

import numpy as np
import pytest
import torch
from conftest import golden_params, load_golden, max_abs
from task_test_util import tile
from test_gpu_dynamics import EXACT

pytestmark = pytest.mark.gpu
N_SMALL = 83
N_WIDE = 65537 + 3  # pick_block: the smallest n off the 64-wide shape, plus 3 (a partial last 256-thread workgroup)
DRAG = dict(lin_drag_linear=[0.031, 0.047, 0.059], lin_drag_quadratic=[0.023, 0.037, 0.053], ang_drag_linear=[0.0011, 0.0017, 0.0023],
            ang_drag_quadratic=[0.0007, 0.0013, 0.0019])

# id: (fixture, n, k, kernel name starts with, ... and holds, drag, host-supplied disturbance)
CASES = {
    "quad_position_step": ("quad_position", N_SMALL, 1, "k_env_step_quad_position_", "", False, False),  # (takes no disturbance)
    "quad_loop_k2": ("quad_position", N_SMALL, 2, "k_env_step_quad_loop<4,", "", False, True),
    "quad_loop_k10": ("quad_position", N_SMALL, 10, "k_env_step_quad_loop<4,", "", False, True),
    "quad_loop_k1_disturbed": ("quad_position", N_SMALL, 1, "k_env_step_quad_loop<4,", "", False, True),
    "quad_loop_velocity_k3": ("quad_velocity", N_SMALL, 3, "k_env_step_quad_loop<4,", "", False, False),
    "quad_loop_octarotor_k2": ("octarotor_velocity", N_SMALL, 2, "k_env_step_quad_loop<8,", "", False, True),
    "one_lane_no_control_k2": ("quad_no_control", N_SMALL, 2, "k_env_step<4,", ",false,true>", False, True),
    "one_lane_drag_k1": ("quad_position", N_SMALL, 1, "k_env_step<4,", ",true,true>", True, False),
    "one_lane_drag_k3_disturbed": ("quad_velocity", N_SMALL, 3, "k_env_step<4,", ",false,true>", True, True),
    "one_lane_256_octarotor_k2": ("octarotor_velocity", N_WIDE, 2, "k_env_step<8,", ",false,false>", False, True),
    "one_lane_256_quad_drag_k1": ("quad_position", N_WIDE, 1, "k_env_step<4,", ",true,false>", True, True),
}


def _setup(case, n, drag):
    from gpu_harness import DynHarness

    g = load_golden("step_" + case)
    pd = golden_params(g)
    if drag:
        pd.update(DRAG)
    rng = np.random.default_rng(n + len(case))
    row = rng.integers(0, g["state"].shape[0], n)  # env i: env i % 64 of a recorded sub-step drawn per env, nudged off the record
    env = np.arange(n) % g["state"].shape[1]
    x = dict(state=g["state"][row, env].copy(), thrust=g["thrust_in"][row, env].copy(), action=g["action"][row, env].copy())
    x["state"][:, 7:13] += rng.normal(scale=0.3, size=(n, 6)).astype(np.float32)  # drag acts on the body velocities
    for key in ("kT", "tau_inc", "tau_dec", "Kp", "Kv", "KR", "Kw"):
        x[key] = tile(g[key], n)
    H = DynHarness(pd, n)
    H.set(state=x["state"], thrust=x["thrust"], kT=x["kT"], tau_inc=x["tau_inc"], tau_dec=x["tau_dec"])
    H.set_gains(x["Kp"], x["Kv"], x["KR"], x["Kw"])
    body_force = torch.full((3, n), 777.0, device=H.dev)
    H.B.body_force = _dptr(body_force)
    return g, pd, x, H, body_force, rng


def _dptr(t):
    from aerial_gym_simulator_amd import _lib

    return _lib.dptr(t)


def _kernel_name(H, n, k):
    buf = C.create_string_buffer(128)
    H.lib.agx_env_step_kernel(H.P, H.B, n, k, None, buf, 128)
    return buf.value.decode()


@pytest.mark.parametrize("name", list(CASES))
def test_body_force_is_the_last_substeps_net_force(orc, parity, name):
    case, n, k, prefix, holds, drag, disturbed = CASES[name]
    g, pd, x, H, body_force, rng = _setup(case, n, drag)
    dist = None
    if disturbed:  # other draws in every sub-step, in ~60 % of the envs: the stored force is the LAST sub-step's, disturbance added
        dist = np.zeros((k, n, 7), np.float32)
        dist[:, :, 0] = rng.random((k, n)) < 0.6
        dist[:, :, 1:] = rng.random((k, n, 6))
        H.set_disturb(dist, g["disturb_max"])
        H.B.body_force = _dptr(body_force)
    kernel = _kernel_name(H, n, k)
    assert kernel.startswith(prefix) and holds in kernel, kernel
    if n == N_WIDE:
        assert kernel.endswith("_%d" % (-(-n // 256) * 256)), kernel  # 256-thread workgroups, the last one partial
    P = orc.make_params(pd)
    gains = (x["kT"], x["tau_inc"], x["tau_dec"], x["Kp"], x["Kv"], x["KR"], x["Kw"])
    st, th = x["state"].copy(), x["thrust"].copy()
    seen = []
    for s in range(k):
        if s == k - 1:  # the last sub-step once more without its disturbance, and on the airframe without drag
            undisturbed = orc.substep(P, st.copy(), x["action"], th.copy(), *gains, integrate=False).body_wrench[:, :3].copy()
            no_drag = orc.substep(orc.make_params(golden_params(g)), st.copy(), x["action"], th.copy(), *gains,
                                  disturb=dist[s] if disturbed else None, disturb_max=g["disturb_max"], integrate=False).body_wrench[:, :3].copy()
        o = orc.substep(P, st, x["action"], th, *gains, disturb=dist[s] if disturbed else None, disturb_max=g["disturb_max"])
        seen.append(o.body_wrench[:, :3].copy())
    H.substeps(x["action"], k)
    got = body_force.cpu().numpy().T
    parity.check(f"body_force_vs_oracle[{name}]", max_abs(got, seen[-1]), EXACT, "abs (bit-exact)")
    parity.check(f"body_force_state_vs_oracle[{name}]", max_abs(H.get("state"), st), EXACT, "abs (bit-exact)")
    # the case can tell: the sub-steps' forces differ, and so does a force taken before the disturbance or the drag was added
    differ = lambda a, b, by: (np.abs(a - b).max(axis=1) > by).mean()  # noqa: E731
    assert k == 1 or differ(seen[0], seen[-1], 1e-4) > 0.5
    assert not disturbed or differ(undisturbed, seen[-1], 1e-3) > 0.4
    assert not drag or differ(no_drag, seen[-1], 1e-4) > 0.5


@pytest.mark.parametrize("case,drag", [("quad_position", False), ("quad_position", True), ("octarotor_velocity", False)])
def test_no_substeps_leave_body_force_alone(case, drag):
    """k = 0: no sub-step, no force -- a sentinel stays bit for bit"""
    n = N_SMALL
    g, pd, x, H, body_force, rng = _setup(case, n, drag)
    sentinel = torch.from_numpy(rng.normal(size=(3, n)).astype(np.float32)).to(H.dev)
    body_force.copy_(sentinel)
    H.substeps(x["action"], 0)
    assert torch.equal(body_force.view(torch.int32), sentinel.view(torch.int32))
