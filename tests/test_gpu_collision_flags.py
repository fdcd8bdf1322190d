"""The obstacle crash flag of the env-step kernels at its limits: k_env_step_quad_loop (boxes over the four lanes of an env, batched
cull data), k_env_step -> collide_trajectory (one lane per env, 64- and 256-thread workgroups) and the stand-alone
k_collide_spheres_boxes, on the scenes of tests/collision_cases.py.  Flags are compared with np.array_equal against the oracle's
(per sub-step, OR-accumulated); the final state is compared bit for bit with the oracle's, which is the premise the scenes were
built on; every run asserts the kernel it meant to exercise through agx_env_step_kernel.

Every run starts from a `crashes` buffer full of ONES (a kernel that only ever sets the flag fails everywhere) and from buffers with
a guard band behind env n - 1 that must come back untouched.  The SoA buffers are [channel][n] with stride n, so a lane past n has
no box or state slot of its own that a test could fill (it would read the next channel of a real env): what the tail runs pin is
that n is no multiple of 16 or 64, that envs of the partial last quad row / wave crash (count_edges hits env n - 1 or n - 2), and that
nothing is written behind env n - 1 of any buffer."""
import ctypes as C

import numpy as np
import pytest
import torch

import collision_cases as cc
from aerial_gym_simulator_amd import _lib
from gpu_harness import CTRL_KEY, DynHarness
from task_test_util import bits

pytestmark = pytest.mark.gpu

GUARD = 256  # elements behind every buffer
SENTINEL = 90


class GuardedHarness(DynHarness):
    """DynHarness whose buffers are the front of larger allocations; the rest holds SENTINEL and must keep it"""

    def __init__(self, pd, n):
        super().__init__(pd, n)
        self.raw = {}
        for name, t in list(self.t.items()):
            self.t[name] = self._guarded(name, t)
        self.crashes = self._guarded("crashes", self.crashes.to(torch.uint8))
        self.trunc = self._guarded("trunc", self.trunc.to(torch.uint8))
        self.sim_steps = self._guarded("sim_steps", self.sim_steps)
        self.rebind()

    def _guarded(self, name, t):
        raw = torch.full((t.numel() + GUARD,), SENTINEL, dtype=t.dtype, device=t.device)
        view = raw[:t.numel()].view(t.shape)
        view.copy_(t)
        self.raw[name] = (raw, t.numel())
        return view

    def set_boxes(self, boxes):
        super().set_boxes(boxes)
        self.boxes = self._guarded("boxes", self.boxes)
        self.rebind()

    def check_guards(self):
        for name, (raw, numel) in self.raw.items():
            assert bool((raw[numel:] == SENTINEL).all()), f"{name}: written behind env n - 1"


def kernel_name(H, k):
    buf = C.create_string_buffer(128)
    _lib.check(H.lib.agx_env_step_kernel(H.P, H.B, H.n, k, None, buf, 128))
    return buf.value.decode()


def expected_kernel(pd, quad, k, n):
    ctrl = _lib.CTRL_IDS[CTRL_KEY.get(pd["controller"], pd["controller"])]
    if quad:
        return f"k_env_step_quad_loop<{pd['num_motors']},{ctrl}>_"
    return f"k_env_step<{pd['num_motors']},{ctrl},{'true' if k == 1 else 'false'},{'true' if n <= 65536 else 'false'}>_"


def harness_for(fam, quad):
    state, action, boxes, expected, m = fam
    if quad is not None:  # (None: the option stays at its default, on)
        _lib.set_option("env_step_quad", int(quad))
    H = GuardedHarness(m["pd"], state.shape[0])
    H.set(state=state, thrust=m["thrust"], kT=m["kT"], tau_inc=m["tau_inc"], tau_dec=m["tau_dec"])
    H.set_gains(*m["gains"])
    H.set_boxes(boxes)
    H.crashes.fill_(1)
    return H


def run(fam, quad, tag=""):
    """one env step of the family's scene on the named kernel family: flags == oracle, state == oracle bit for bit, guards intact"""
    state, action, boxes, expected, m = fam
    n, k = state.shape[0], m["k"]
    H = harness_for(fam, quad)
    name = kernel_name(H, k)
    assert name.startswith(expected_kernel(m["pd"], bool(quad), k, n)), (tag, name)
    H.substeps(action, k)
    got = H.crashes.cpu().numpy()
    assert set(np.unique(got).tolist()) <= {0, 1}
    wrong = np.nonzero(got.astype(bool) != expected)[0]
    assert wrong.size == 0, (tag, name, "envs with a wrong flag", wrong[:16].tolist(), "hit index", m.get("hit_index", np.zeros(n))[wrong[:16]].tolist())
    assert np.array_equal(bits(H.get("state")), bits(m["final_state"])), (tag, name, "the state is not the oracle's: the scene's premise")
    assert np.array_equal(bits(H.get("thrust")), bits(m["final_thrust"])), (tag, name)
    assert np.array_equal(H.sim_steps.cpu().numpy(), np.ones(n, np.int32))
    H.check_guards()
    return H


def standalone(H, fam, seed):
    """agx_collide_spheres_boxes at the final positions over a random pre-set flag pattern: kept flags survive, new hits are added"""
    state, action, boxes, expected, m = fam
    n = state.shape[0]
    pre = np.random.default_rng(seed).random(n) < 0.3
    H.crashes.copy_(torch.from_numpy(pre.astype(np.uint8)))
    _lib.check(H.lib.agx_collide_spheres_boxes(H.P, H.B, n, H.stream()))
    torch.cuda.synchronize()
    want = pre | m["hits_per_substep"][-1]
    assert np.array_equal(H.crashes.cpu().numpy().astype(bool), want)
    assert (want & ~pre).any() and (pre & ~m["hits_per_substep"][-1]).any()  # new hits, and flags only the pre-set pattern explains
    H.check_guards()


# ---- box counts at and across the batch edges, hits in every lane / batch position; partial last wave and quad row --------------
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 63, 64, 65, 129])
@pytest.mark.parametrize("case", ["quad_velocity", "magpie_acceleration"])
def test_quad_loop_4_motors_count_edges(orc, case, K):
    """n = 53: three full waves of 16 envs and a tail of 5; 64 boxes per batch trip"""
    run(cc.count_edges(K, case, 53, 4), True, (case, K))


@pytest.mark.parametrize("K", [3, 47, 48, 49, 97])
def test_quad_loop_8_motors_count_edges(orc, K):
    """n = 37: two full waves and a tail of 5; 48 boxes per batch trip"""
    run(cc.count_edges(K, "octarotor_velocity", 37, 4), True, K)


@pytest.mark.parametrize("K", [1, 2, 64, 65])
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("case", ["quad_velocity", "quad_no_control", "tinyprop_no_control"])
def test_one_lane_block_64_count_edges(orc, case, k, K):
    """n = 71: one full wave and a tail of 7; k = 1 is the SINGLE instance; the robots without a controller have no lane-quad kernel
    (the option is left ON for them: the launcher must pick k_env_step by itself)"""
    run(cc.count_edges(K, case, 71, k), False if case == "quad_velocity" else None, (case, k, K))


def test_one_lane_block_256_count_edges(orc):
    """n = 65 536 + 70: 256-thread workgroups (traj[(s*3+c)*256 + tid]), the last one with 70 envs"""
    run(cc.count_edges(5, "quad_velocity", 65536 + 70, 3), False)


def test_one_lane_block_256_above_64_kib_of_lds(orc):
    """k = 22 sub-steps x 3 x 256 lanes x 4 B = 67 584 B of dynamic LDS, above the 64 KiB a launch gets without opting in:
    agx_env_step opts the instance in (hipFuncSetAttribute, as the LBVH build does) and the flags are the oracle's"""
    run(cc.count_edges(2, "quad_velocity", 65536 + 70, 22), False)


# ---- a hit at exactly one sub-step ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 10, 32])
@pytest.mark.parametrize("quad", [True, False])
def test_hit_at_one_substep_only(orc, quad, k):
    fam = cc.substep_only(k)
    assert fam[0].shape[0] == 2 * k + 3 and fam[3].all()
    run(fam, quad, k)


# ---- far centres, culls, grazing separations: both kernel families and the stand-alone entry point ----------------------------
@pytest.mark.parametrize("family", ["cull_adversaries", "grazing"])
@pytest.mark.parametrize("quad", [True, False])
def test_cull_adversaries_and_grazing(orc, quad, family):
    fam = getattr(cc, family)()
    H = run(fam, quad, family)
    standalone(H, fam, 17)


@pytest.mark.parametrize("family", ["cull_adversaries", "grazing"])
def test_cull_adversaries_and_grazing_without_a_controller(orc, family):
    fam = getattr(cc, family)("quad_no_control")
    H = run(fam, None, family)
    standalone(H, fam, 18)


# ---- flag semantics ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quad", [True, False])
def test_clean_step_overwrites_stale_flags(orc, quad):
    """crashes pre-filled with ones, 5 near misses per env that pass the cull: all zero afterwards"""
    fam = cc.all_misses(5)
    H = run(fam, quad)
    assert not H.crashes.cpu().numpy().any()


@pytest.mark.parametrize("k", [1, 4])
def test_launch_flags_bit_0_keeps_the_earlier_launch_flags(orc, k):
    """launch_flags bit 0 (an earlier launch of this env step already ran): the one-lane kernel -- the only one that takes launch
    flags, whatever the option says -- ORs the new hits into the old flags"""
    fam = cc.count_edges(5, "quad_velocity", 71, k)
    state, action, boxes, expected, m = fam
    H = harness_for(fam, True)
    H.B.launch_flags = 1
    assert kernel_name(H, k).startswith(expected_kernel(m["pd"], False, k, 71))
    pre = np.random.default_rng(3).random(71) < 0.4
    H.crashes.copy_(torch.from_numpy(pre.astype(np.uint8)))
    H.substeps(action, k)
    assert np.array_equal(H.crashes.cpu().numpy().astype(bool), pre | expected)
    assert (pre & ~expected).any() and (expected & ~pre).any()
    assert np.array_equal(bits(H.get("state")), bits(m["final_state"]))
    H.check_guards()


@pytest.mark.parametrize("quad", [True, False])
def test_no_substep_means_no_obstacle_test(orc, quad):
    """B.boxes set and k = 0 (k_env_step, `if (B.boxes && k > 0)`; the lane-quad loop needs k >= 1, so the launcher picks the one-lane
    kernel either way): no position was produced, nothing is tested -- the flag is cleared, or, with launch_flags bit 0, what the
    earlier launch left; the state stays and the step counter advances"""
    fam = cc.cull_adversaries()
    state, action, boxes, expected, m = fam
    n = state.shape[0]
    inside = np.zeros_like(boxes)
    inside[..., 0:3], inside[..., 6], inside[..., 7:10] = state[:, None, 0:3], 1.0, 0.5  # every robot sits in the middle of 5 boxes
    H = harness_for((state, action, inside, expected, m), quad)
    name = kernel_name(H, 0)
    assert name.startswith(f"k_env_step<4,{_lib.CTRL_IDS['velocity']},false,true>_"), name
    H.substeps(action, 0)
    assert not H.crashes.cpu().numpy().any()
    assert np.array_equal(bits(H.get("state")), bits(state))
    pre = np.random.default_rng(4).random(n) < 0.5
    H.crashes.copy_(torch.from_numpy(pre.astype(np.uint8)))
    H.B.launch_flags = 1
    H.substeps(action, 0)
    assert np.array_equal(H.crashes.cpu().numpy().astype(bool), pre)
    assert np.array_equal(H.sim_steps.cpu().numpy(), np.full(n, 2, np.int32))
    H.check_guards()
    # ... and the same boxes with one sub-step: every env crashes (the boxes are 0.5 m, a sub-step moves the robot by centimetres)
    H.B.launch_flags = 0
    H.crashes.zero_()
    slow = state.copy()
    slow[:, 7:10] = np.clip(slow[:, 7:10], -3.0, 3.0)
    H.set(state=slow)
    H.substeps(action, 1)
    assert H.crashes.cpu().numpy().all()
