"""GPU: the robot kind BaseROV (AGX_LAUNCH_ROV) through the C ABI and through EnvManager, against the correctly rounded goldens of the
reference's own BaseROV (tests/golden/rov_cr/), the oracle where the two robot kinds coincide and the restatement of their three
differences (tests/rov_ref.py, pinned by tests/test_base_rov.py).  Batch sizes: one lane, a partial wave, the exact wave, one over,
a partial second wave, more than one block."""
import ctypes as C
import json

import numpy as np
import pytest
import rov_ref as R
import torch
from rov_ref import DERIVED, disturb_of, load_golden, same
from task_test_util import DEV, NB, derived_of, harness, no_host_sync, npy, split_step, tile

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 83, 333)
RECORDS = ("step_base_rov_fully_actuated", "step_edge_base_rov_fully_actuated", "step_base_rov_no_control", "step_base_rov_default_fully_actuated")
SPLIT_GATE = 2e-5  # fused step against the split path, per step (tests/test_gpu_robot_plugin.py)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", RECORDS)
def test_robot_step_equals_the_reference_bit_for_bit(name, n):
    """agx_robot_step with the flag: per-body force and torque tensors, the five derived tensors, the motor thrusts"""
    g = load_golden(name, cr=True)
    mask = [int(b) for b in g["application_mask"]]
    for k in range(g["state"].shape[0]):
        H, _ = harness(g, n, k, rov=True)
        F, T = H.robot_step(tile(g["action"][k], n), NB, mask)
        assert same(F, tile(g["force"][k], n)) and same(T, tile(g["torque"][k], n)), (name, k)
        for key, got in derived_of(H).items():
            assert same(got, tile(g[key][k], n)), (name, k, key)
        assert same(H.get("thrust"), tile(g["thrust_out"][k], n))
        H.update_states()  # the stand-alone agx_update_states: the same derived tensors again
        for key, got in derived_of(H).items():
            assert same(got, tile(g[key][k], n)), (name, k, key)


def test_without_the_flag_the_fixtures_differ():
    """the same launch as a multirotor: the drag rows of the nominal record and the Euler rows of the edge record come out different
    -- the fixtures do tell the two robot kinds apart"""
    g = load_golden("step_base_rov_fully_actuated", cr=True)
    mask = [int(b) for b in g["application_mask"]]
    H, _ = harness(g, 64, 0, rov=False)
    F, T = H.robot_step(g["action"][0], NB, mask)
    assert (F[:, 0, :] != g["force"][0][:, 0, :]).any(axis=1).all()                  # norm law: every row
    assert same(F[:, 1:], g["force"][0][:, 1:]) and same(T, g["torque"][0])          # the angular drag law is shared
    e = load_golden("step_edge_base_rov_fully_actuated", cr=True)
    H, _ = harness(e, 64, 0, rov=False)
    H.robot_step(e["action"][0], NB, mask)
    d = derived_of(H)
    assert (d["euler"] != e["euler"][0]).any(axis=1).sum() > 30 and d["euler"].min() < 0   # wrapped to (-pi, pi]
    for key in ("qveh", "vveh", "vbody", "wbody"):
        assert same(d[key], e[key][0]), key
    H.update_states()
    assert (derived_of(H)["euler"] != e["euler"][0]).any(axis=1).sum() > 30


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ("step_base_rov_fully_actuated", "step_edge_base_rov_fully_actuated", "step_base_rov_no_control"))
def test_fused_env_step_equals_the_split_path(name, n):
    """M = 8, FULLY_ACTUATED and NONE, non-zero per-axis drag, host disturbance draws: the one fused launch against robot step ->
    net body wrench -> integration; thrusts and derived tensors bit for bit (the same arithmetic on the same numbers), the state
    within 2e-5 absolute (the wrench map folded ahead of time against the per-body sum).  Measured on an MI355X: at most 2.4e-7 on
    the nominal records, 7.6e-6 on the edge record (one ulp of the 100 m/s rows)"""
    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd.config.robot_config import BaseROVCfg

    g = load_golden(name, cr=True)
    for k in range(g["state"].shape[0]):
        a = tile(g["action"][k], n)
        Hf, _ = harness(g, n, k, rov=True)
        buf = C.create_string_buffer(128)
        assert Hf.lib.agx_env_step_kernel(Hf.P, Hf.B, n, 1, None, buf, 128) == 0
        assert buf.value.decode().startswith("k_env_step_rov<%d,true,true>_" % _lib.CTRL_IDS["none" if "no_control" in name else "fully_actuated"]), buf.value
        Hf.substeps(a, 1)
        Hs, _ = harness(g, n, k, rov=True)
        split_step(Hs, BaseROVCfg, a, n)
        assert same(Hf.get("thrust"), Hs.get("thrust")) and same(Hf.get("thrust"), tile(g["thrust_out"][k], n))
        for key, got in derived_of(Hf).items():
            assert same(got, tile(g[key][k], n)) and same(got, derived_of(Hs)[key]), (name, k, key)
        err = float(np.abs(Hf.get("state") - Hs.get("state")).max())
        print("fused vs split", name, n, k, "max |state difference| %.3e" % err)
        assert err <= SPLIT_GATE, (name, k, err)


@pytest.mark.parametrize("n", SIZES)
def test_fused_env_step_equals_the_oracle_where_the_drag_laws_coincide(orc, n):
    """default zero coefficients: every env; the edge record: the envs whose body velocity lies along one axis.  State, thrusts and
    derived tensors bit for bit; the Euler angles against the restatement (the oracle wraps them)"""
    for name in ("step_base_rov_default_fully_actuated", "step_edge_base_rov_fully_actuated"):
        g = load_golden(name, cr=True)
        for k in range(g["state"].shape[0]):
            H, pd = harness(g, n, k, rov=True)
            H.substeps(tile(g["action"][k], n), 1)
            st, th = tile(g["state"][k], n).copy(), tile(g["thrust_in"][k], n).copy()
            dist = disturb_of(g, k)
            o = orc.substep(orc.make_params(pd), st, tile(g["action"][k], n), th, *(tile(g[x], n) for x in ("kT", "tau_inc", "tau_dec", "Kp", "Kv", "KR", "Kw")),
                            disturb=None if dist is None else tile(dist, n), disturb_max=g["disturb_max"], integrate=True)
            rows = np.ones(n, bool) if "default" in name else tile((g["vbody"][k] != 0).sum(axis=1) <= 1, n)
            assert rows.sum() >= (n if "default" in name else (1 if k == 0 else 0))
            assert same(H.get("state")[rows], st[rows]) and same(H.get("thrust")[rows], th[rows]), (name, k)
            d = derived_of(H)
            for key, want in (("qveh", o.qveh), ("vveh", o.vveh), ("vbody", o.vbody), ("wbody", o.wbody)):
                assert same(d[key], want), (name, k, key)
            assert same(d["euler"], R.euler(tile(g["state"][k], n)[:, 3:7]))


def run_reset(H, g, c, n, parity, target=None):
    """agx_reset_masked with the draws of case c of rov_reset.npz; with `target` [N, 3]: agx_post_step_position, which also returns the
    position task's observation of the post-reset state"""
    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd._lib import AgxResetArgs

    mask = tile(g["mask"][c], n)
    H.reset_mask.copy_(torch.from_numpy(mask.astype(np.uint8)))
    H.reset_flag.zero_()
    H.reset_flag[parity] = 1 if mask.any() else 0
    H.reset_flag[parity ^ 1] = 7  # the NEXT step's flag: the launch clears it
    H.B.flag_parity = parity
    H.sim_steps.fill_(5)
    Rr = AgxResetArgs()
    keep = [torch.zeros(n, 3, device=DEV), torch.from_numpy(tile(g["u_state"][c], n)).to(DEV), torch.from_numpy(tile(g["u_gains"][c], n)).to(DEV)]
    Rr.u_bounds_lo = Rr.u_bounds_hi = _lib.dptr(keep[0])
    Rr.u_state, Rr.u_gains, Rr.randomize_gains = _lib.dptr(keep[1]), _lib.dptr(keep[2]), 1
    Rr.u_tau_inc = Rr.u_tau_dec = Rr.u_thrust = Rr.u_kT = None  # no motor draws are taken for this kind
    for i in range(3):
        Rr.lower_bound_min[i] = Rr.lower_bound_max[i] = float(g["bounds_min"][i])
        Rr.upper_bound_min[i] = Rr.upper_bound_max[i] = float(g["bounds_max"][i])
    for i in range(13):
        Rr.min_state[i], Rr.max_state[i] = float(g["min_init_state"][i]), float(g["max_init_state"][i])
    for i in range(12):
        Rr.gains_min[i], Rr.gains_max[i] = float(g["gains_min"][i]), float(g["gains_max"][i])
    Rr.tau_inc_min, Rr.tau_inc_max, Rr.tau_dec_min, Rr.tau_dec_max, Rr.kT_min, Rr.kT_max = 0.01, 0.03, 0.005, 0.005, 1e-5, 2e-5
    if target is None:
        _lib.check(H.lib.agx_reset_masked(H.P, H.B, n, Rr, H.stream()), "agx_reset_masked")
        torch.cuda.synchronize()
        return mask
    from gpu_harness import to_soa

    tg, obs = to_soa(target, DEV), torch.full((n, 13), -7.0, device=DEV)
    _lib.check(H.lib.agx_post_step_position(H.P, H.B, n, Rr, _lib.dptr(tg), _lib.dptr(obs), H.stream()), "agx_post_step_position")
    torch.cuda.synchronize()
    return mask, npy(obs)


@pytest.mark.parametrize("parity", (0, 1))
@pytest.mark.parametrize("n", SIZES)
def test_masked_reset_keeps_the_motor_state(n, parity):
    """agx_reset_masked with the flag on the four masks of rov_reset.npz (none; env 70, in the last partial wave of 83; all; random):
    state, gains and derived tensors as the reference leaves them, bit for bit, under host draws; motor thrusts and motor constants
    of the reset envs unchanged; envs outside the mask untouched; no motor draw tensors handed in"""
    from aerial_gym_simulator_amd import _lib
    from gpu_harness import DynHarness

    g = load_golden("rov_reset", cr=True)
    pd = json.loads(str(load_golden("step_base_rov_default_fully_actuated", cr=True)["params_json"]))
    for c in range(4):
        H = DynHarness(pd, n)
        H.B.launch_flags = _lib.LAUNCH_ROV
        before = {k: tile(g[k + "_before"][c], n) for k in ("state", "thrust", "tau_inc", "tau_dec", "gains") + DERIVED}
        kT = np.full((n, 8), 1.5e-5, np.float32)
        H.set(state=before["state"], thrust=before["thrust"], tau_inc=before["tau_inc"], tau_dec=before["tau_dec"], gains=before["gains"], kT=kT,
              derived=np.concatenate([before[k] for k in DERIVED], axis=1))
        mask = run_reset(H, g, c, n, parity)
        assert same(H.get("state"), tile(g["state_after"][c], n)) and same(H.get("gains"), tile(g["gains_after"][c], n)), (c, n)
        for key, got in derived_of(H).items():  # (no env resets: nothing is refreshed, like the reference's early return)
            assert same(got, tile(g[key + "_after"][c], n)), (c, key)
        for key in ("thrust", "tau_inc", "tau_dec"):
            assert same(H.get(key), before[key]), (c, key)
        assert same(H.get("kT"), kT)
        assert same(H.get("state")[~mask], before["state"][~mask]) and same(H.get("gains")[~mask], before["gains"][~mask])
        steps = npy(H.sim_steps)
        assert (steps[mask] == 0).all() and (steps[~mask] == 5).all()
        assert npy(H.reset_flag)[parity ^ 1] == 0
        assert same(H.get("bmin"), np.tile(g["bounds_min"], (n, 1))) and same(H.get("bmax"), np.tile(g["bounds_max"], (n, 1)))


@pytest.mark.parametrize("n", (65, 333))
def test_post_step_position_with_the_flag_resets_and_observes(n):
    """agx_post_step_position with the flag (k_reset_masked_rov<true>), none and the random mask of rov_reset.npz: the reset as
    agx_reset_masked does it, and the 13-D observation target - p | q | v_body | w_body of the post-reset state of every env"""
    from aerial_gym_simulator_amd import _lib
    from gpu_harness import DynHarness

    g = load_golden("rov_reset", cr=True)
    pd = json.loads(str(load_golden("step_base_rov_default_fully_actuated", cr=True)["params_json"]))
    target = np.random.default_rng(5).uniform(-1, 1, (n, 3)).astype(np.float32)
    for c in (0, 3):
        H = DynHarness(pd, n)
        H.B.launch_flags = _lib.LAUNCH_ROV
        before = {k: tile(g[k + "_before"][c], n) for k in ("state", "thrust", "tau_inc", "tau_dec", "gains") + DERIVED}
        H.set(state=before["state"], thrust=before["thrust"], tau_inc=before["tau_inc"], tau_dec=before["tau_dec"], gains=before["gains"],
              derived=np.concatenate([before[k] for k in DERIVED], axis=1))
        mask, obs = run_reset(H, g, c, n, 1, target=target)
        assert mask.any() == (c == 3)
        st = tile(g["state_after"][c], n)
        assert same(H.get("state"), st) and same(H.get("gains"), tile(g["gains_after"][c], n)), c
        for key, got in derived_of(H).items():
            assert same(got, tile(g[key + "_after"][c], n)), (c, key)
        for key in ("thrust", "tau_inc", "tau_dec"):
            assert same(H.get(key), before[key]), (c, key)
        want = np.concatenate([target - st[:, 0:3], st[:, 3:7], tile(g["vbody_after"][c], n), tile(g["wbody_after"][c], n)], axis=1)
        assert same(obs, want), c


@pytest.mark.parametrize("n", (65, 333))
def test_fused_two_sub_steps_equal_the_oracle(orc, n):
    """k = 2 in one launch (the k-loop instance k_env_step_rov<7, false, true>) on the default-zero record, where the oracle's drag
    law coincides: state and thrusts bit for bit after both sub-steps, the derived tensors those of the second sub-step's
    pre-physics state with the Euler angles of the restatement"""
    g = load_golden("step_base_rov_default_fully_actuated", cr=True)
    H, pd = harness(g, n, 0, rov=True)
    buf = C.create_string_buffer(128)
    assert H.lib.agx_env_step_kernel(H.P, H.B, n, 2, None, buf, 128) == 0 and buf.value.decode().startswith("k_env_step_rov<7,false,true>_")
    a = tile(g["action"][0], n)
    dist = np.stack([tile(g["disturb"][k], n) for k in range(2)])
    assert dist.any()
    H.set_disturb(dist, g["disturb_max"])
    H.substeps(a, 2)
    st, th = tile(g["state"][0], n).copy(), tile(g["thrust_in"][0], n).copy()
    P = orc.make_params(pd)
    for k in range(2):
        pre = st.copy()
        o = orc.substep(P, st, a, th, *(tile(g[x], n) for x in ("kT", "tau_inc", "tau_dec", "Kp", "Kv", "KR", "Kw")), disturb=dist[k],
                        disturb_max=g["disturb_max"], integrate=True)
    assert same(H.get("state"), st) and same(H.get("thrust"), th)
    d = derived_of(H)
    for key, want in (("qveh", o.qveh), ("vveh", o.vveh), ("vbody", o.vbody), ("wbody", o.wbody)):
        assert same(d[key], want), key
    assert same(d["euler"], R.euler(pre[:, 3:7]))


def test_other_reset_entry_points_refuse_the_flag():
    """agx_nav_robot_side and agx_post_step_end_to_end reset multirotors only: with the flag they say so; agx_post_step_position
    refuses it for another motor count"""
    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd._lib import AgxResetArgs
    from conftest import golden_params
    from conftest import load_golden as load_base
    from gpu_harness import DynHarness

    n = 8
    g = load_golden("step_base_rov_default_fully_actuated", cr=True)
    H, _ = harness(g, n, 0, rov=True)
    Rr = AgxResetArgs()
    z = torch.zeros(n, 16, device=DEV)
    A = _lib.AgxNavRobotSideArgs()
    with pytest.raises(RuntimeError, match="AGX_LAUNCH_ROV"):
        _lib.check(H.lib.agx_nav_robot_side(H.P, H.B, n, Rr, C.byref(A), H.stream()), "agx_nav_robot_side")
    with pytest.raises(RuntimeError, match="AGX_LAUNCH_ROV"):
        _lib.check(H.lib.agx_post_step_end_to_end(H.P, H.B, n, Rr, _lib.dptr(z), None, _lib.dptr(z), _lib.dptr(z), _lib.dptr(z), _lib.dptr(z),
                                                  H.stream()), "agx_post_step_end_to_end")
    q = load_base("step_quad_no_control")
    Hq = DynHarness(golden_params(q), n)
    Hq.B.launch_flags = _lib.LAUNCH_ROV
    with pytest.raises(RuntimeError, match="AGX_LAUNCH_ROV.*num_motors == 8"):
        _lib.check(Hq.lib.agx_post_step_position(Hq.P, Hq.B, n, Rr, _lib.dptr(z), _lib.dptr(z), Hq.stream()), "agx_post_step_position")


def test_launchers_refuse_the_flag_for_other_robots():
    """M != 8, or a Lee controller: every launcher that reads the flag says no, naming it"""
    from aerial_gym_simulator_amd import _lib
    from conftest import golden_params
    from conftest import load_golden as load_base
    from gpu_harness import DynHarness

    for case, what in (("quad_no_control", "num_motors == 8"), ("octarotor_position", "Lee controller")):
        g = load_base("step_" + case)
        pd = golden_params(g)
        n = 8
        H = DynHarness(pd, n)
        H.B.launch_flags = _lib.LAUNCH_ROV
        a = np.zeros((n, pd["num_actions"]), np.float32)
        with pytest.raises(RuntimeError, match="AGX_LAUNCH_ROV.*" + what):
            H.substeps(a, 1)
        with pytest.raises(RuntimeError, match="AGX_LAUNCH_ROV.*" + what):
            H.robot_step(a, g["force"].shape[2], [int(b) for b in g["application_mask"]])
        with pytest.raises(RuntimeError, match="AGX_LAUNCH_ROV.*" + what):
            H.reset_masked(np.ones(n, np.uint8), dict(u_bounds_lo=np.zeros((n, 3)), u_bounds_hi=np.zeros((n, 3)), u_state=np.zeros((n, 13))),
                           dict(tau_inc=(0.01, 0.02), tau_dec=(0.01, 0.02), kT=(1e-5, 2e-5)), np.zeros(13), np.zeros(13), ([-1] * 3, [-1] * 3, [1] * 3, [1] * 3))
        assert not np.isnan(H.get("state")).any()
    g = load_golden("step_base_rov_fully_actuated", cr=True)
    H, _ = harness(g, 8, 0, rov=True)
    H.B.launch_flags = _lib.LAUNCH_ROV | 0x20000
    with pytest.raises(RuntimeError, match="launch_flags"):
        H.substeps(g["action"][0][:8], 1)


# ---- through EnvManager -----------------------------------------------------------------------------------------------------
def build(robot_name="base_rov", n=65, strict=False, seed=5, source=None):
    from aerial_gym.sim.sim_builder import SimBuilder

    args = {"rng_seed": seed, "strict_rng": strict}
    if source is not None:
        args["random_source"] = source
    return SimBuilder().build_env(sim_name="base_sim_no_gravity", env_name="empty_env", robot_name=robot_name, controller_name="fully_actuated_control",
                                  device=DEV, args=args, num_envs=n, headless=True, use_warp=False)


def actions(n, gen):
    a = torch.cat([torch.rand(n, 3, device=DEV, generator=gen) * 2 - 1, torch.randn(n, 4, device=DEV, generator=gen)], dim=1)
    return a


def test_strict_trace_equals_the_oracle_and_consumes_the_reference_draws(orc):
    """20 steps of EnvManager.step + post_reward_calculation_step on base_rov + fully_actuated_control in base_sim_no_gravity,
    strict_rng, n = 65, truncations set by hand every few steps: the state bit-identical to the oracle driven with the same
    parameter block and the draws the random source gave out, Euler angles equal to the restatement, motor state carried through
    every reset, and per reset exactly the reference's draws: bounds (2 x [N, 3]), one [N, 13] for the state, four [m, 3] for the
    gains -- none for the motors; the device generator's offset moves by what those calls take"""
    from aerial_gym_simulator_amd.utils.random_source import TorchRandomSource

    class Recording(TorchRandomSource):
        def __init__(self, device):
            super().__init__(device)
            self.log = []

        def rand(self, *shape, tag=""):
            out = super().rand(*shape, tag=tag)
            self.log.append((tag, out.clone()))
            return out

        def rand_into(self, out, tag=""):
            super().rand_into(out, tag=tag)
            self.log.append((tag, out.clone()))
            return out

        def bernoulli(self, p, *shape, tag=""):
            out = super().bernoulli(p, *shape, tag=tag)
            self.log.append((tag, out.clone()))
            return out

    n = 65
    fx = load_golden("rov_reset", cr=True)
    rs = Recording(DEV)
    env = build(n=n, strict=True, source=rs)
    rob = env.robot_manager.robot
    g = env.get_obs()
    mm, ctrl = rob.control_allocator.motor_model, rob.controller
    assert env.strict_rng and ctrl._per_env_gains_bound and env.cfg.env.num_physics_steps_per_env_step_std == 0
    env.reset()
    P = orc.make_params(rob.params_dict)
    cfg = rob.cfg
    dmax = np.array(cfg.disturbance.max_force_and_torque_disturbance, np.float32)
    gen = torch.Generator(device=DEV).manual_seed(2)
    pick = torch.Generator().manual_seed(3)
    device_gen = torch.cuda.default_generators[torch.device(DEV).index or 0]
    resets = 0
    for t in range(20):
        st, th = npy(g["robot_state_tensor"]), npy(mm.current_motor_thrust)
        st0 = st.copy()
        kT, ti, td = npy(mm.motor_thrust_constant), npy(mm.motor_time_constants_increasing), npy(mm.motor_time_constants_decreasing)
        gains = [npy(x) for x in (ctrl.K_pos_tensor_current, ctrl.K_linvel_tensor_current, ctrl.K_rot_tensor_current, ctrl.K_angvel_tensor_current)]
        a = actions(n, gen)
        rs.log.clear()
        env.step(a)
        draws = dict(rs.log)
        assert [tag for tag, _ in rs.log] == ["disturb_occ", "disturb_f", "disturb_t"]
        dist = np.concatenate([npy(draws["disturb_occ"])[:, None], npy(draws["disturb_f"]), npy(draws["disturb_t"])], axis=1)
        o = orc.substep(P, st, npy(a), th, kT, ti, td, *gains, disturb=dist, disturb_max=dmax, integrate=True)
        assert same(npy(g["robot_state_tensor"]), st) and same(npy(mm.current_motor_thrust), th), t
        assert same(npy(g["robot_euler_angles"]), R.euler(st0[:, 3:7])), t  # of the pre-physics state, not wrapped
        for key, want in (("robot_vehicle_orientation", o.qveh), ("robot_vehicle_linvel", o.vveh), ("robot_body_linvel", o.vbody), ("robot_body_angvel", o.wbody)):
            assert same(npy(g[key]), want), (t, key)
        want_mask = np.zeros(n, bool)
        if t % 4 == 3:
            want_mask = (torch.rand(n, generator=pick) < 0.2).numpy()
            want_mask[64] = True  # the one env of the second wave
            g["truncations"][torch.from_numpy(want_mask).to(DEV)] = True
        rs.log.clear()
        offset0 = device_gen.get_offset()
        ids = env.post_reward_calculation_step()
        offset1 = device_gen.get_offset()
        assert np.array_equal(npy(g["reset_mask"]).astype(bool), want_mask) and len(ids) == want_mask.sum()
        tags = [tag for tag, _ in rs.log]
        if not want_mask.any():
            assert tags == [] and offset1 == offset0
            assert same(npy(g["robot_state_tensor"]), st)
            continue
        resets += 1
        m = int(want_mask.sum())
        # the reference's calls: IsaacGymEnv.reset_idx draws the bounds, BaseROV.reset_idx the state and the gains -- no motor draws
        assert tags == ["bounds_lo", "bounds_hi", "robot_state", "gains0", "gains1", "gains2", "gains3"], tags
        shapes = [list(x.shape) for _, x in rs.log]
        assert shapes[2:] == [[n, 13]] + [[m, 3]] * 4 and json.loads(str(fx["draw_shapes"][3])) == [[83, 13]] + [[28, 3]] * 4
        assert sum(int(np.prod(s)) for s in shapes[2:]) == 13 * n + 12 * m  # rov_reset.npz: consumed = 13 N + 12 m
        assert int(fx["consumed"][3]) == 13 * 83 + 12 * 28
        state = device_gen.get_state()
        before = device_gen.get_offset()
        for s in shapes:
            torch.rand(*s, device=DEV)
        replayed = device_gen.get_offset() - before
        device_gen.set_state(state)
        assert offset1 - offset0 == replayed, (offset1 - offset0, replayed)
        d = dict(rs.log)
        u_gains = np.zeros((n, 12), np.float32)
        for k in range(4):
            u_gains[want_mask, 3 * k:3 * k + 3] = npy(d["gains%d" % k])
        st2 = R.reset(want_mask, st, npy(d["robot_state"]), cfg.init_config.min_init_state, cfg.init_config.max_init_state,
                      npy(g["env_bounds_min"]), npy(g["env_bounds_max"]))
        assert same(npy(g["robot_state_tensor"]), st2), t
        assert same(np.concatenate([npy(x) for x in (ctrl.K_pos_tensor_current, ctrl.K_linvel_tensor_current, ctrl.K_rot_tensor_current,
                                                       ctrl.K_angvel_tensor_current)], axis=1),
                    R.reset_gains(want_mask, np.concatenate(gains, axis=1), u_gains, ctrl.gains_min, ctrl.gains_max))
        assert same(npy(mm.current_motor_thrust), th) and same(npy(mm.motor_time_constants_increasing), ti)  # carried through the reset
        assert same(npy(mm.motor_time_constants_decreasing), td)
        e, qv, vv, vb, wb = orc.update_states(st2)  # the refresh of every env that ends the reset
        assert same(npy(g["robot_euler_angles"]), R.euler(st2[:, 3:7]))
        assert same(npy(g["robot_body_linvel"]), vb) and same(npy(g["robot_vehicle_orientation"]), qv)
        steps = npy(env.sim_steps)
        assert (steps[want_mask] == 0).all() and (steps[~want_mask] > 0).all()
    assert resets == 5 and np.isfinite(npy(g["robot_state_tensor"])).all()


TRACE_STEPS, TRACE_N = 20, 65


def trace_masks(n):
    """the reset sets of the default-mode trace, by step: a few envs of the first wave and the one env of the second (the wave hands
    the draws out lane by lane), a random third (more than eight of a wave: every lane for itself), all, env 64 alone, six envs of the first wave"""
    rng = np.random.default_rng(12)
    m = {t: np.zeros(n, bool) for t in (3, 7, 11, 15, 19)}
    m[3][[1, 17, 40, 64]] = True
    m[7] = rng.random(n) < 0.33
    m[11][:] = True
    m[15][64] = True
    m[19][[5, 9, 22, 33, 47, 58]] = True
    assert m[7][:64].sum() > 8 and 0 < m[19][:64].sum() <= 8
    return m


def default_mode_trace(robot_name, orc, monkeypatch):
    """20 steps of env.step + post_reward_calculation_step in the default (device-generator) mode at n = 65, truncations written on the
    device every fourth step, both calls under the no-sync guard -> the library calls of every step.  For base_rov every reset is
    checked: see the test below."""
    from aerial_gym_simulator_amd import _lib

    n = TRACE_N
    env = build(robot_name=robot_name, n=n, seed=9)
    rob = env.robot_manager.robot
    rov = robot_name == "base_rov"
    g, mm, ctrl = env.get_obs(), rob.control_allocator.motor_model, rob.controller
    env.reset()
    masks = trace_masks(n)
    masks_dev = {t: torch.from_numpy(m).to(DEV) for t, m in masks.items()}
    gen = torch.Generator(device=DEV).manual_seed(4)
    acts = [actions(n, gen) for _ in range(TRACE_STEPS)]
    cfg = rob.cfg.init_config
    calls, log, real = [], [], _lib.check

    def check(code, what=""):
        log.append(what)
        return real(code, what)

    monkeypatch.setattr(_lib, "check", check)
    gains_of = lambda: np.concatenate([npy(x) for x in (ctrl.K_pos_tensor_current, ctrl.K_linvel_tensor_current, ctrl.K_rot_tensor_current,  # noqa: E731
                                                        ctrl.K_angvel_tensor_current)], axis=1)
    motors_of = lambda: [npy(x) for x in (mm.current_motor_thrust, mm.motor_time_constants_increasing, mm.motor_time_constants_decreasing)]  # noqa: E731
    resets = 0
    for t in range(TRACE_STEPS):
        del log[:]
        with no_host_sync():
            env.step(acts[t])
        st, motors, gains, episodes = npy(g["robot_state_tensor"]), motors_of(), gains_of(), npy(g["episode_count"])
        assert np.isfinite(st).all() and all(np.isfinite(x).all() for x in motors), t
        with no_host_sync():
            if t in masks_dev:
                g["truncations"].logical_or_(masks_dev[t])  # a device-side write: no synchronisation
            env.post_reward_calculation_step()
        calls.append(list(log))
        mask = masks.get(t, np.zeros(n, bool))
        st2, motors2, gains2 = npy(g["robot_state_tensor"]), motors_of(), gains_of()
        assert np.array_equal(npy(g["reset_mask"]).astype(bool), mask), t
        assert np.isfinite(st2).all() and np.isfinite(npy(g["robot_euler_angles"])).all(), t
        assert same(st2[~mask], st[~mask]) and same(gains2[~mask], gains[~mask]), t  # envs outside the mask: untouched
        steps = npy(env.sim_steps)
        assert (steps[mask] == 0).all() and (steps[~mask] > 0).all(), t
        if not mask.any() or not rov:
            continue
        resets += 1
        for before, after in zip(motors, motors2):  # thrusts and time constants of EVERY env, the reset ones included
            assert same(after, before), t
        lo, hi = npy(g["env_bounds_min"]), npy(g["env_bounds_max"])
        p, v = st2[mask, 0:3], st2[mask, 7:13]
        assert (st2[mask] != st[mask]).any(axis=1).all(), t
        assert (p >= lo[mask]).all() and (p <= hi[mask]).all() and (np.abs(v) <= 0.2).all(), t
        assert np.abs(np.linalg.norm(st2[mask, 3:7], axis=1) - 1).max() < 1e-6
        # the device generator's draws are a function of (seed, env, episode, stream): the oracle's restatement of the same streams
        u_state = orc.rng_fill(env.rng_seed, episodes, orc.RNG_STATE, 13)
        u_gains = orc.rng_fill(env.rng_seed, episodes, orc.RNG_GAINS, 12)
        assert same(st2, R.reset(mask, st, u_state, cfg.min_init_state, cfg.max_init_state, lo, hi)), t
        assert same(gains2, R.reset_gains(mask, gains, u_gains, ctrl.gains_min, ctrl.gains_max)), t
        assert np.array_equal(npy(g["episode_count"]), episodes + mask), t
        e, qv, vv, vb, wb = orc.update_states(st2)  # the refresh of every env that ends the reset
        assert same(npy(g["robot_euler_angles"]), R.euler(st2[:, 3:7])) and same(npy(g["robot_body_linvel"]), vb) and same(npy(g["robot_body_angvel"]), wb)
    monkeypatch.setattr(_lib, "check", real)
    buf = C.create_string_buffer(128)
    assert env._lib.agx_env_step_kernel(env._params, env._buffers, n, 1, None, buf, 128) == 0
    euler = npy(g["robot_euler_angles"])
    return calls, buf.value.decode(), euler, resets


def test_default_mode_trace_resets_on_the_device_and_is_the_octarotors_launch_list(orc, monkeypatch):
    """The trace of the strict test in the default mode: outputs finite on every step, no host synchronisation, and on every one of the
    five resets (partial masks of both draw paths of the wave, the full batch, the lone env of the second wave) motor thrusts and
    time constants of all envs as they were, the reset envs' state re-drawn inside the env bounds -- bit for bit the restatement on
    the device generator's draws --, their gains re-drawn, sim_steps zeroed, everybody else untouched.  The library calls of every
    step are exactly those of an octarotor + fully_actuated_control step recorded the same way."""
    rov, kernel, euler, resets = default_mode_trace("base_rov", orc, monkeypatch)
    octa, kernel_octa, _, _ = default_mode_trace("base_octarotor", orc, monkeypatch)
    print("base_rov step:", rov[-1], kernel)
    assert resets == 5 and len(rov) == TRACE_STEPS
    assert rov == octa and all(c == ["agx_env_step", "agx_reset_set", "agx_reset_masked"] for c in rov), (rov, octa)
    # (the ROV kind runs the one-lane kernel at every batch size; the drag-free octarotor of this size its lane-quad loop)
    assert kernel.startswith("k_env_step_rov<7,true,true>_") and kernel_octa.startswith("k_env_step_quad_loop<8,7>_")
    assert euler.min() >= 0 and (euler > np.pi).any()  # [0, 2 pi), not wrapped


def test_subclass_overriding_step_runs_per_sub_step_and_flies_like_the_fused_step():
    """a registered BaseROV subclass whose step() calls super().step(): once per physics sub-step through agx_robot_step ->
    agx_net_body_wrench -> integration, within 2e-5 of the fused step from the same state"""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.registry.robot_registry import robot_registry
    from aerial_gym_simulator_amd.robots.base_rov import BaseROV

    class ToyROV(BaseROV):
        calls = 0

        def step(self, action_tensor):
            super().step(action_tensor)
            type(self).calls += 1

    robot_registry.register("toy_passthrough_rov", ToyROV, robot_registry.get_robot_config("base_rov"))
    n = 83
    envs = [build(robot_name=r, n=n, seed=9) for r in ("base_rov", "toy_passthrough_rov")]
    assert envs[1].robot_manager.robot.external_robot and not envs[0].robot_manager.robot.external_robot
    for e in envs:
        e.reset()
    assert torch.equal(envs[0].global_tensor_dict["robot_state_tensor"], envs[1].global_tensor_dict["robot_state_tensor"])
    # an ROV's reset leaves the motor model alone: the time constants are still what each constructor drew from torch's generator
    mm0, mm1 = (e.robot_manager.robot.control_allocator.motor_model for e in envs)
    mm1.motor_time_constants_increasing.copy_(mm0.motor_time_constants_increasing)
    mm1.motor_time_constants_decreasing.copy_(mm0.motor_time_constants_decreasing)
    gen = torch.Generator(device=DEV).manual_seed(1)
    for t in range(4):
        envs[1].global_tensor_dict["robot_state_tensor"].copy_(envs[0].global_tensor_dict["robot_state_tensor"])  # the same state into every step
        envs[1].robot_manager.robot.control_allocator.motor_model.current_motor_thrust.copy_(
            envs[0].robot_manager.robot.control_allocator.motor_model.current_motor_thrust)
        a = actions(n, gen)
        for e in envs:
            e.step(a)
        s0, s1 = (e.global_tensor_dict["robot_state_tensor"] for e in envs)
        assert float((s0 - s1).abs().max()) <= SPLIT_GATE, (t, float((s0 - s1).abs().max()))
        assert torch.equal(envs[0].global_tensor_dict["robot_euler_angles"], envs[1].global_tensor_dict["robot_euler_angles"])
        assert torch.equal(*(e.robot_manager.robot.control_allocator.motor_model.current_motor_thrust for e in envs))
    assert ToyROV.calls == 4 and float(envs[1].global_tensor_dict["robot_force_tensor"][:, 9:, 2].abs().max()) > 0
