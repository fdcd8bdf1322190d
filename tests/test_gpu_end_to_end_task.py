"""GPU: the end-to-end motor-command set-point task -- the agx_end_to_end_* kernels through the C ABI against the reference's own
numbers (tests/golden/end_to_end_cr/*.npz) and the restatement tests/end_to_end_ref.py (pinned to the reference by
tests/test_end_to_end_task.py), bit for bit; agx_post_step_end_to_end against the composition of the launches it replaces; the
device generator's noise; tinyprop's dynamics (the first airframe with products of inertia) against the oracle; the task through the
Task API, default and strict_rng."""
import copy

import end_to_end_ref as R
import numpy as np
import pytest
import torch
from task_test_util import DEV, Buffers, RecordingSource, config_restored, dev, host, load_golden, offset_consumed_by, rows, soa
from task_test_util import same_bits_nan as same

pytestmark = pytest.mark.gpu
CR = "end_to_end_cr"  # the fixtures made by the reference's code with correctly rounded elementary functions
CONFIG_KEYS = ("seed", "num_envs", "headless", "device", "use_warp", "args", "episode_len_steps", "return_state_before_reset", "crash_dist",
               "process_actions_for_task")
NAME = "position_setpoint_task_sim2real_end_to_end"
SIZES = (1, 63, 64, 65, 83, 333)  # one lane, a partial wave, the exact wave, one over, a partial second block, more than five blocks


def reward_constants():
    from aerial_gym_simulator_amd.task.position_setpoint_task_sim2real_end_to_end import reward_constants as rc

    return rc("end_to_end")


@pytest.mark.parametrize("n", SIZES)
def test_pre_step_kernel_equals_the_restatement_bit_for_bit(n):
    """the rescale on the glue fixture's actions (beyond +-1 among them) plus a NaN, -0.0 and the exact limits; prev_position"""
    g = load_golden("end_to_end_glue", CR)
    a = rows(g["action_in"].reshape(-1, 4), n)
    a[0] = [np.nan, -0.0, 1.0, -1.0]
    pos = rows(g["pre_position"].reshape(-1, 3), n)
    H = Buffers(n, pos, rows(g["robot_orientation"].reshape(-1, 4), n))
    p = H._lib.dptr
    L = H._lib.AgxEndToEndLimits()
    for j in range(4):
        L.min[j], L.max[j] = 0.2, 1.2
    a_in = dev(a)
    out, prev_position = torch.full((n, 4), -7.0, device=DEV), torch.full((3, n), -7.0, device=DEV)
    H._lib.check(H.lib.agx_end_to_end_pre_step(H.B, n, p(a_in), L, p(out), p(prev_position), H.stream()), "agx_end_to_end_pre_step")
    torch.cuda.synchronize()
    assert same(host(out), R.rescale(a)) and np.isnan(host(out)[0, 0]) and same(host(a_in), a)  # the caller's tensor is not changed
    assert same(host(prev_position).T, pos)
    assert same(R.rescale(g["action_in"][3]), g["actions"][3])


@pytest.mark.parametrize("n", SIZES)
def test_reward_kernel_equals_the_reference_bit_for_bit(n):
    g = load_golden("end_to_end_reward", CR)
    G = lambda name: rows(g[name], n)  # noqa: E731
    episode_len = 4
    sim_steps = (np.arange(n) * 3) % 9
    H = Buffers(n, G("position"), G("orientation"), linvel=G("linvel"), body_angvel=G("body_angvel"), crashes=G("crashes_in"), sim_steps=sim_steps)
    p = H._lib.dptr
    target, act, pact, ppe = soa(G("target")), dev(G("actions")), dev(G("prev_actions")), soa(G("prev_pos_error"))
    rew = torch.zeros(n, device=DEV)
    H._lib.check(H.lib.agx_end_to_end_reward(H.B, n, p(target), p(act), p(pact), p(ppe), reward_constants(), float(g["crash_dist"]),
                                             episode_len, 1, p(rew), H.stream()), "agx_end_to_end_reward")
    torch.cuda.synchronize()
    assert same(host(rew), G("reward"))
    crashes = G("crashes_out").astype(bool)
    assert np.array_equal(host(H.crashes), crashes)
    trunc = sim_steps > episode_len
    assert np.array_equal(host(H.truncations), trunc)
    assert np.array_equal(host(H.reset_mask), (crashes | trunc).astype(np.uint8))
    assert host(H.reset_flag).tolist() == [0, int((crashes | trunc).any())]  # the flag word of this step's parity only
    assert same(host(act), G("actions")) and same(host(ppe).T, G("prev_pos_error"))  # inputs untouched
    r = R.reward(G("target"), G("position"), G("orientation"), G("linvel"), G("body_angvel"), G("crashes_in"), sim_steps, G("actions"),
                 G("prev_actions"), G("prev_pos_error"), episode_len)
    assert same(host(rew), r["reward"]) and np.array_equal(host(H.reset_mask), r["reset_mask"].astype(np.uint8))


@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("reset_on_collision", [0, 1])
def test_reward_kernel_on_both_flag_parities_with_and_without_reset_on_collision(parity, reset_on_collision):
    g = load_golden("end_to_end_reward", CR)
    n = 65
    G = lambda name: rows(g[name], n)  # noqa: E731
    H = Buffers(n, G("position"), G("orientation"), linvel=G("linvel"), body_angvel=G("body_angvel"), crashes=G("crashes_in"), parity=parity)
    p = H._lib.dptr
    target, act, pact, ppe = soa(G("target")), dev(G("actions")), dev(G("prev_actions")), soa(G("prev_pos_error"))
    rew = torch.zeros(n, device=DEV)
    H._lib.check(H.lib.agx_end_to_end_reward(H.B, n, p(target), p(act), p(pact), p(ppe), reward_constants(), float(g["crash_dist"]), 600,
                                             reset_on_collision, p(rew), H.stream()), "agx_end_to_end_reward")
    torch.cuda.synchronize()
    crashes = G("crashes_out").astype(bool)
    assert same(host(rew), G("reward")) and crashes.any() and np.array_equal(host(H.crashes), crashes)
    want = crashes if reset_on_collision else np.zeros(n, bool)
    flag = [0, 0]
    flag[parity] = int(want.any())
    assert np.array_equal(host(H.reset_mask), want.astype(np.uint8)) and host(H.reset_flag).tolist() == flag


@pytest.mark.parametrize("n", SIZES)
def test_obs_kernel_with_host_noise_equals_the_reference_bit_for_bit(n):
    """the NaN rows included (n >= 12: one ulp outside +-1 gives NaN at the reference's positions)"""
    g = load_golden("end_to_end_obs", CR)
    G = lambda name: rows(g[name], n)  # noqa: E731
    s = G("state")
    H = Buffers(n, s[:, 0:3], s[:, 3:7], linvel=s[:, 7:10], body_angvel=G("body_angvel"))
    p = H._lib.dptr
    z = dev(np.stack([rows(g["z"][j], n) for j in range(4)]))
    target = soa(G("target"))
    obs = torch.zeros(n, 15, device=DEV)
    H._lib.check(H.lib.agx_end_to_end_obs(H.B, n, p(target), p(z), p(obs), H.stream()), "agx_end_to_end_obs")
    torch.cuda.synchronize()
    assert same(host(obs), G("obs"))
    assert same(host(obs), R.observation(G("target"), s[:, 0:3], s[:, 3:7], s[:, 7:10], G("body_angvel"), host(z)))
    if n >= 12:
        assert np.isnan(host(obs)[8:12, 3:9]).all() and not np.isnan(host(obs)[0:8]).any()
    assert same(host(H.state).T[:, 0:10], s[:, 0:10])  # nothing is stored back
    # exchange rows are not written for the 15-D observation: refused, not ignored
    H.B.step_rows[0] = H.B.step_rows[1] = p(obs)
    assert H.lib.agx_end_to_end_obs(H.B, n, p(target), p(z), p(obs), H.stream()) != 0
    assert "step_rows" in H.lib.agx_last_error().decode()


def device_normals(lib_mod, lib, B, n):
    z = torch.full((4, n, 3), 9.0, device=DEV)
    lib_mod.check(lib.agx_end_to_end_noise(B, n, lib_mod.dptr(z), lib_mod.current_stream(DEV)), "agx_end_to_end_noise")
    torch.cuda.synchronize()
    return host(z)


def test_device_noise_is_a_pure_function_of_seed_global_env_and_step():
    g = load_golden("end_to_end_obs", CR)
    z = {}
    for n, base, step, seed in ((83, 0, 5, 1234), (333, 0, 5, 1234), (33, 50, 5, 1234), (83, 0, 6, 1234), (83, 0, 5, 1235)):
        s = rows(g["state"], n)
        H = Buffers(n, s[:, 0:3], s[:, 3:7], linvel=s[:, 7:10], body_angvel=rows(g["body_angvel"], n))
        H.B.rng_seed, H.B.env_index_base, H.B.step_counter = seed, base, step
        z[(n, base, step, seed)] = device_normals(H._lib, H.lib, H.B, n)
        if n == 83 and step == 5 and seed == 1234:  # the observation with the device generator == with those normals handed in
            p = H._lib.dptr
            target, zz = soa(rows(g["target"], n)), dev(z[(n, base, step, seed)])
            o1, o2 = torch.zeros(n, 15, device=DEV), torch.zeros(n, 15, device=DEV)
            H._lib.check(H.lib.agx_end_to_end_obs(H.B, n, p(target), None, p(o1), H.stream()), "agx_end_to_end_obs")
            H._lib.check(H.lib.agx_end_to_end_obs(H.B, n, p(target), p(zz), p(o2), H.stream()), "agx_end_to_end_obs")
            torch.cuda.synchronize()
            assert same(host(o1), host(o2))
    a = z[(83, 0, 5, 1234)]
    assert np.isfinite(a).all() and same(a, z[(333, 0, 5, 1234)][:, :83]) and same(z[(33, 50, 5, 1234)], a[:, 50:83])
    assert not (a == z[(83, 0, 6, 1234)]).any() and not (a == z[(83, 0, 5, 1235)]).any()
    assert len(np.unique(a)) == a.size  # twelve different normals per env, different between envs


def test_device_noise_statistics():
    """333 envs x 50 steps: mean and standard deviation of each of the four noise groups (as they enter the observation: from an
    all-zero state the position, velocity and rate columns ARE the scaled noise; the orientation group from the normals times its
    sigma) within five standard errors of 0 and of the group's sigma (N = 49 950 per group: SE(mean) = sigma / sqrt(N),
    SE(std) = sigma / sqrt(2 N))."""
    n, steps = 333, 50
    q = np.tile(np.array([0, 0, 0, 1], np.float32), (n, 1))
    H = Buffers(n, np.zeros((n, 3), np.float32), q)
    H.B.rng_seed = 20251018
    p = H._lib.dptr
    target = torch.zeros(3, n, device=DEV)
    obs = torch.zeros(n, 15, device=DEV)
    groups = {k: [] for k in ("pos", "euler", "linvel", "angvel")}
    for t in range(steps):
        H.B.step_counter = t
        H._lib.check(H.lib.agx_end_to_end_obs(H.B, n, p(target), None, p(obs), H.stream()), "agx_end_to_end_obs")
        o = host(obs)
        z = device_normals(H._lib, H.lib, H.B, n)
        assert same(o[:, 0:3], z[0] * R.STD_POS) and same(o[:, 9:12], z[2] * R.STD_LINVEL) and same(o[:, 12:15], z[3] * R.STD_ANGVEL)
        groups["pos"].append(o[:, 0:3]); groups["linvel"].append(o[:, 9:12]); groups["angvel"].append(o[:, 12:15])  # noqa: E702
        groups["euler"].append(z[1] * R.STD_EULER)
    for name, sigma in (("pos", 0.001), ("euler", np.pi / 1032), ("linvel", 0.002), ("angvel", 0.001)):
        x = np.concatenate(groups[name]).astype(np.float64).ravel()
        N = x.size
        assert N == n * steps * 3
        print("device noise", name, "mean / sigma %.4f  std / sigma %.5f" % (x.mean() / sigma, x.std() / sigma))
        assert abs(x.mean()) <= 5 * sigma / np.sqrt(N) and abs(x.std() - sigma) <= 5 * sigma / np.sqrt(2 * N), name


def make_task(n, strict=False, seed=11, **overrides):
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    cfg = task_registry.get_task_config(NAME)
    cfg.args = dict(overrides.pop("args", {}), strict_rng=strict)
    for k, v in overrides.items():
        setattr(cfg, k, v)
    return task_registry.make_task(NAME, seed=seed, num_envs=n, headless=True)


MASKS = ("none", "one_in_the_last_partial_wave", "all", "random")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mask_kind", MASKS)
def test_post_step_equals_the_composition_of_the_launches_it_replaces(mask_kind, n):
    """agx_post_step_end_to_end == agx_reset_masked -> (some env resets: target of every env = 0) -> agx_end_to_end_obs -> torch
    bookkeeping, on the same inputs and the same generator coordinates, bit-identical in EVERY buffer.  With no env resetting the
    derived tensors stay as stale as they were; with one env resetting every env's are refreshed."""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    with config_restored(task_registry.get_task_config(NAME), CONFIG_KEYS):
        task = make_task(n)
        env, g = task.sim_env, task.obs_dict
        mm = env.robot_manager.robot.control_allocator.motor_model
        rng = np.random.default_rng(100 + n)
        mask = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "random": rng.random(n) < 0.3}.get(mask_kind)
        if mask is None:
            mask = np.zeros(n, bool)
            mask[n - 1] = True
        tensors = dict(state=g["robot_state_soa"], derived=g["robot_derived_soa"], thrust=mm.thrust_soa, kT=mm.kT_soa, bmin=env.bounds_soa[0],
                       bmax=env.bounds_soa[1], sim_steps=g["sim_steps"], episode_count=g["episode_count"], reset_mask=g["reset_mask"],
                       reset_flag=g["reset_flag"], crashes=g["crashes"], truncations=g["truncations"], target=task.target_soa,
                       obs=task.task_obs["observations"], actions=task.actions, prev_actions=task.prev_actions,
                       prev_pos_error=task.prev_pos_error_soa)
        q = rng.standard_normal((n, 4)).astype(np.float32)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        state = np.concatenate([rng.standard_normal((n, 3)), q, rng.standard_normal((n, 6))], axis=1).astype(np.float32)
        tensors["state"].copy_(soa(state))
        tensors["derived"].copy_(dev(rng.standard_normal((16, n)).astype(np.float32)))  # stale on purpose: nothing the state would give
        tensors["thrust"].copy_(dev(rng.random((4, n)).astype(np.float32)))
        tensors["sim_steps"].copy_(dev(rng.integers(0, 50, n).astype(np.int32)))
        tensors["episode_count"].copy_(dev(rng.integers(0, 5, n).astype(np.int32)))
        tensors["reset_mask"].copy_(dev(mask.astype(np.uint8)))
        tensors["target"].copy_(dev(rng.standard_normal((3, n)).astype(np.float32)))
        tensors["actions"].copy_(dev(rng.random((n, 4)).astype(np.float32)))
        tensors["prev_actions"].fill_(-7.0)
        tensors["prev_pos_error"].fill_(-7.0)
        tensors["obs"].fill_(-7.0)
        B = env._buffers
        B.env_index_base, B.step_counter = 1000, 7
        parity = B.flag_parity
        flags = [1, 1]  # the next step's word must come out cleared
        flags[parity] = int(mask.any())
        tensors["reset_flag"].copy_(dev(np.array(flags, np.int32)))
        start = {k: v.clone() for k, v in tensors.items()}
        p, st = _lib.dptr, env._stream()
        # -- the composition
        _lib.check(env._lib.agx_reset_masked(env._params, B, n, env._reset_args, st), "agx_reset_masked")
        if mask.any():
            task.target_soa.zero_()
        _lib.check(env._lib.agx_end_to_end_obs(B, n, p(task.target_soa), None, p(tensors["obs"]), st), "agx_end_to_end_obs")
        tensors["prev_actions"].copy_(tensors["actions"])
        torch.sub(task.target_soa, g["robot_state_soa"][0:3], out=tensors["prev_pos_error"])
        torch.cuda.synchronize()
        composed = {k: host(v).copy() for k, v in tensors.items()}
        # -- the one launch, from the same start
        for k, v in tensors.items():
            v.copy_(start[k])
        _lib.check(env._lib.agx_post_step_end_to_end(env._params, B, n, env._reset_args, p(task.target_soa), None, p(tensors["obs"]),
                                                     p(tensors["actions"]), p(tensors["prev_actions"]), p(tensors["prev_pos_error"]), st),
                   "agx_post_step_end_to_end")
        torch.cuda.synchronize()
        for k, v in tensors.items():
            assert same(host(v), composed[k]), k
        s0 = {k: host(v) for k, v in start.items()}
        assert composed["reset_flag"][parity ^ 1] == 0 and composed["reset_flag"][parity] == flags[parity]
        assert np.isfinite(composed["obs"]).all() and not (composed["obs"] == -7.0).any() and same(composed["prev_actions"], s0["actions"])
        if not mask.any():
            for k in ("state", "derived", "thrust", "sim_steps", "episode_count", "target"):
                assert same(composed[k], s0[k]), k  # nobody resets: the reference does not touch anything, the derived tensors stay stale
        else:
            assert not composed["target"].any() and not (composed["derived"] == s0["derived"]).all(axis=0).any()  # EVERY env refreshed
            assert same(composed["state"][:, ~mask], s0["state"][:, ~mask]) and (composed["sim_steps"][mask] == 0).all()
            assert (composed["state"][0:3][:, mask] != s0["state"][0:3][:, mask]).all()
            assert np.array_equal(composed["episode_count"], s0["episode_count"] + mask)
        # with the strict mode's host noise the launch takes the normals it is handed
        z = dev(rng.standard_normal((4, n, 3)).astype(np.float32))
        for k, v in tensors.items():
            v.copy_(start[k])
        _lib.check(env._lib.agx_post_step_end_to_end(env._params, B, n, env._reset_args, p(task.target_soa), p(z), p(tensors["obs"]),
                                                     p(tensors["actions"]), p(tensors["prev_actions"]), p(tensors["prev_pos_error"]), st),
                   "agx_post_step_end_to_end")
        torch.cuda.synchronize()
        sa = host(g["robot_state_soa"]).T
        want = R.observation(host(task.target_soa).T, sa[:, 0:3], sa[:, 3:7], sa[:, 7:10], host(g["robot_derived_soa"]).T[:, 13:16], host(z))
        assert same(host(tensors["obs"]), want) and same(host(g["robot_state_soa"]), composed["state"])
        task.close()


def test_tinyprop_dynamics_substep_equals_the_oracle_bit_for_bit(orc):
    """83 envs, two sub-steps of tinyprop + no_control through the one-lane kernel against the C oracle: the first device test with
    non-zero products of inertia (attitudes over the whole sphere, body rates of a few rad/s: the gyroscopic term and J^-1 see every
    entry).  Mutation: with P.inertia[1] zeroed the same launch no longer equals the oracle.
    Then the same launch on the inputs of the reference's own BaseMultirotor.step recorded with correctly rounded functions
    (tests/golden/end_to_end_cr/step_*tinyprop_no_control.npz, rows wrapped to 83): thrusts, derived tensors, next state."""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd.config.robot_config import TinyPropCfg
    from aerial_gym_simulator_amd.config.sim_config import BaseSimConfig
    from aerial_gym_simulator_amd.robots.robot_model import robot_params_dict
    from gpu_harness import DynHarness

    n = 83
    pd = robot_params_dict(TinyPropCfg, None, "none", BaseSimConfig)
    pd["controller"] = "no_control"
    assert pd["inertia"][1] != 0 and pd["inertia"][2] != 0 and pd["inertia"][5] != 0
    rng = np.random.default_rng(83)
    q = rng.standard_normal((n, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    state0 = np.concatenate([rng.standard_normal((n, 3)), q, rng.standard_normal((n, 3)), 3.0 * rng.standard_normal((n, 3))], axis=1).astype(np.float32)
    thrust0 = (0.2 + rng.random((n, 4))).astype(np.float32)
    kT = np.full((n, 4), 0.00001286412, np.float32)
    tau = np.full((n, 4), 0.047, np.float32)
    zeros3 = np.zeros((n, 3), np.float32)
    actions = [(0.2 + rng.random((n, 4))).astype(np.float32), (rng.random((n, 4)) * 2.0 - 0.3).astype(np.float32)]  # the second beyond both limits

    def run(pd_device):
        H = DynHarness(pd_device, n)
        name = ctypes_kernel_name(_lib, H)
        H.set(kT=kT, tau_inc=tau, tau_dec=tau, state=state0, thrust=thrust0)
        out = []
        for a in actions:
            H.substeps(a, 1)
            out.append((H.get("state"), H.get("thrust"), H.get("derived")))
        return name, out

    name, got = run(pd)
    assert name.startswith("k_env_step<4,0,")  # the one-lane kernel
    P = orc.make_params(pd)
    st, th = state0.copy(), thrust0.copy()
    for k, a in enumerate(actions):
        o = orc.substep(P, st, a, th, kT, tau, tau, zeros3, zeros3, zeros3, zeros3, integrate=True)
        gs, gt, gd = got[k]
        assert same(gs, st) and same(gt, th), k
        for name, got_d, want in (("qveh", gd[:, 3:7], o.qveh), ("vveh", gd[:, 7:10], o.vveh), ("vbody", gd[:, 10:13], o.vbody),
                                  ("wbody", gd[:, 13:16], o.wbody)):
            assert np.array_equal(got_d, want), (k, name)  # (equal values: the vehicle quaternion's zeros may differ in sign)
    assert np.isfinite(st).all() and np.abs(st[:, 10:13] - state0[:, 10:13]).max() > 1e-3
    mutant = copy.deepcopy(pd)
    mutant["inertia"][1] = 0.0
    _, bad = run(mutant)
    assert not same(bad[0][0], got[0][0]) and not same(bad[1][0], st)
    for case in ("step_tinyprop_no_control", "step_edge_tinyprop_no_control"):
        g = load_golden(case, CR)
        H = DynHarness(pd, n)
        H.set(kT=rows(g["kT"], n), tau_inc=rows(g["tau_inc"], n), tau_dec=rows(g["tau_dec"], n))
        K = g["state"].shape[0]
        for k in range(K):
            H.set(state=rows(g["state"][k], n), thrust=rows(g["thrust_in"][k], n))
            H.substeps(rows(g["action"][k], n), 1)
            gd = H.get("derived")
            assert np.array_equal(H.get("thrust"), rows(g["thrust_out"][k], n)), (case, k)
            for name, got_d in (("qveh", gd[:, 3:7]), ("vveh", gd[:, 7:10]), ("vbody", gd[:, 10:13]), ("wbody", gd[:, 13:16])):
                assert np.array_equal(got_d, rows(g[name][k], n)), (case, k, name)
            if k + 1 < K:
                assert np.array_equal(H.get("state"), rows(g["state"][k + 1], n)), (case, k)


def ctypes_kernel_name(_lib, H):
    import ctypes

    buf = ctypes.create_string_buffer(128)
    _lib.check(H.lib.agx_env_step_kernel(H.P, H.B, H.n, 1, None, buf, 128), "agx_env_step_kernel")
    return buf.value.decode()


def reference_call_list(n, resets):
    """what the reference's step draws from the torch generator on tinyprop / no_control / empty_env: on a step in which some env
    resets TWO full sets of reset draws (post_reward_calculation_step's reset, then the task's own reset_idx: :180-182), each env
    bounds lo / hi, robot state, motor tau_inc / tau_dec / thrust / kT; then the four normal fills of the observation"""
    one = [("rand", (n, 3), "bounds_lo"), ("rand", (n, 3), "bounds_hi"), ("rand", (n, 13), "robot_state"), ("rand", (n, 4), "tau_inc"),
           ("rand", (n, 4), "tau_dec"), ("rand", (n, 4), "thrust"), ("rand", (n, 4), "kT")]
    noise = [("normal", (n, 3), "end_to_end_obs_noise_" + w) for w in ("pos", "orientation", "linvel", "angvel")]
    return (one + one if resets else []) + noise


@pytest.mark.parametrize("strict", [False, True])
def test_task_trace_equals_the_restatement_on_the_dict_tensors(strict):
    """83 envs, 40 steps, episodes of 12 steps in two phases (truncation resets in some steps, none in others), four targets moved
    8 m away at step 17 (distance crashes: the targets go back to zero with the reset).  Everything task.step() leaves behind equals
    tests/end_to_end_ref.py applied to the tensors the kernels read, driven by the same normals, bit for bit."""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    n, steps, episode_len, crash_dist = 83, 40, 12, 6.0
    rs = RecordingSource(DEV)
    with config_restored(task_registry.get_task_config(NAME), CONFIG_KEYS):
        task = make_task(n, strict=strict, args={"random_source": rs}, episode_len_steps=episode_len, crash_dist=crash_dist)
        env, d = task.sim_env, task.obs_dict
        launches = []
        for name in ("agx_end_to_end_pre_step", "agx_env_step", "agx_end_to_end_reward", "agx_post_step_end_to_end", "agx_end_to_end_obs",
                     "agx_reset_masked"):
            launches_of(env, name, launches)
        snap = {}
        real_reward = task.compute_rewards_and_crashes

        def hooked_reward(obs_dict):
            snap["reward"] = {key: host(d[key]).copy() for key in ("robot_position", "robot_orientation", "robot_linvel", "robot_body_angvel",
                                                                   "crashes")}
            snap["reward"]["sim_steps"] = host(env.sim_steps).copy()
            return real_reward(obs_dict)

        task.compute_rewards_and_crashes = hooked_reward
        task.reset()
        env.sim_steps[: n // 2] += 5
        ref = R.TaskRef(n)
        for name in ("actions", "prev_actions", "prev_pos_error", "prev_position"):
            assert not host(getattr(task, name)).any(), name  # zero before the first step; reset() does not touch them
        gen = torch.Generator().manual_seed(5)
        gpu_gen = torch.cuda.default_generators[0]
        seen = {"trunc": 0, "crash": 0, "reset_steps": 0}
        for t in range(steps):
            if t == 17:
                task.target_position[3:7, 0] = 8.0
            a = torch.rand(n, 4, generator=gen) * 3.0 - 1.5  # beyond +-1 in a third of the entries: the clamp
            handed = a.to(DEV)
            ref.target = host(task.target_position).copy()
            pre_position = host(d["robot_position"]).copy()
            del rs.normals[:], rs.calls[:], launches[:]
            offset = gpu_gen.get_offset()
            obs, rew, term, trunc, info = task.step(handed)
            torch.cuda.synchronize()
            consumed = gpu_gen.get_offset() - offset
            assert launches == ["agx_end_to_end_pre_step", "agx_env_step", "agx_end_to_end_reward", "agx_post_step_end_to_end"], (t, launches)
            # -- step()'s first lines
            ref.pre_step(pre_position, a.numpy())
            assert same(host(task.actions), ref.actions) and same(host(task.prev_position), ref.prev_position) and same(host(handed), a.numpy()), t
            assert same(host(d["robot_actions"]), ref.actions), t
            # -- reward, flags, reset set on the tensors as EnvManager.step left them
            s = snap["reward"]
            r = ref.reward(s["robot_position"], s["robot_orientation"], s["robot_linvel"], s["robot_body_angvel"], s["crashes"], s["sim_steps"],
                           episode_len, crash_dist, env.cfg.env.reset_on_collision)
            assert same(host(rew), r["reward"]), (t, np.abs(host(rew) - r["reward"]).max())
            assert np.array_equal(host(term), r["crashes"]) and np.array_equal(host(trunc), r["truncations"]), t
            assert np.array_equal(host(d["reset_mask"]), r["reset_mask"].astype(np.uint8)) and info == {}, t
            resets = bool(r["reset_mask"].any())
            ref.after_reset(resets)
            assert same(host(task.target_position), ref.target), t
            # -- observation of the post-reset tensors, with the normals the step used
            if strict:
                z = host(torch.stack(rs.normals))
                assert [(c[0], c[1], c[2]) for c in rs.calls] == reference_call_list(n, resets), (t, rs.calls)
                assert consumed == offset_consumed_by(reference_call_list(n, resets)), t
            else:
                assert rs.calls == [] and consumed == 0, t
                z = device_normals(_lib, env._lib, env._buffers, n)
            post = {key: host(d[key]).copy() for key in ("robot_position", "robot_orientation", "robot_linvel", "robot_body_angvel")}
            o = ref.observation(post["robot_position"], post["robot_orientation"], post["robot_linvel"], post["robot_body_angvel"], z)
            assert same(host(obs["observations"]), o), (t, np.nanmax(np.abs(host(obs["observations"]) - o)))
            assert obs["rewards"] is task.rewards and obs["terminations"] is task.terminations and obs["truncations"] is task.truncations
            if resets:
                m = r["reset_mask"]
                assert (post["robot_position"][m] != s["robot_position"][m]).any(axis=1).all() and (host(env.sim_steps)[m] == 0).all(), t
                assert same(post["robot_position"][~m], s["robot_position"][~m]), t
            # -- end of step
            ref.end_of_step(post["robot_position"])
            assert same(host(task.prev_actions), ref.prev_actions) and same(host(task.prev_pos_error), ref.prev_pos_error), t
            assert not host(task.action_history).any()
            seen["trunc"] += int(r["truncations"].sum())
            seen["crash"] += int((r["crashes"] & ~s["crashes"].astype(bool)).sum())
            seen["reset_steps"] += int(resets)
        print("end-to-end trace", "strict" if strict else "default", seen)
        assert seen["trunc"] >= 2 * n and seen["crash"] >= 4 and 4 <= seen["reset_steps"] <= steps - 10, seen
        task.close()


def launches_of(env, name, log):
    """count the calls of one entry point of the loaded library as the task issues them"""
    real = getattr(env._lib, name)

    class Lib:
        def __init__(self, inner):
            self._inner = inner

        def __getattr__(self, key):
            return getattr(self._inner, key)

    if not isinstance(env._lib, Lib):
        env._lib = Lib(env._lib)

    def counted(*args):
        log.append(name)
        return real(*args)

    setattr(env._lib, name, counted)


def test_general_path_state_before_reset_explicit_reset_and_a_user_rescale():
    """return_state_before_reset: the observation is of the pre-reset state (stand-alone launch, the env manager's own reset) and the
    bookkeeping still sees the post-reset position; get_return_tuple() by hand launches once more and serves nothing stale; a rescale
    the user put into the config runs as torch code instead of the pre-step launch."""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    n = 65
    calls = []

    def user_rescale(actions, lo, hi):
        calls.append(tuple(actions.shape))
        return torch.clamp(actions, -1, 1) * 0.25 + 0.75

    with config_restored(task_registry.get_task_config(NAME), CONFIG_KEYS) as cfg:
        task = make_task(n, return_state_before_reset=True, episode_len_steps=3, crash_dist=50.0)
        env, d = task.sim_env, task.obs_dict
        launches = []
        for name in ("agx_end_to_end_pre_step", "agx_end_to_end_reward", "agx_post_step_end_to_end", "agx_end_to_end_obs", "agx_reset_masked"):
            launches_of(env, name, launches)
        task.reset()
        assert launches == ["agx_reset_masked", "agx_end_to_end_obs"]
        ref = R.TaskRef(n)
        for t in range(6):
            del launches[:]
            a = torch.rand(n, 4, device=DEV) * 2 - 1
            if t == 4:
                cfg.process_actions_for_task = staticmethod(user_rescale)
            obs = task.step(a)[0]["observations"]
            torch.cuda.synchronize()
            want = (["agx_end_to_end_pre_step"] if t < 4 else []) + ["agx_end_to_end_reward", "agx_end_to_end_obs", "agx_reset_masked"]
            assert launches == want, (t, launches)
            z = device_normals(_lib, env._lib, env._buffers, n)
            resets = bool(host(d["reset_mask"]).any())
            assert resets == (t == 3)
            if not resets:  # (nothing moved since the observation was taken)
                o = R.observation(host(task.target_position), host(d["robot_position"]), host(d["robot_orientation"]), host(d["robot_linvel"]),
                                  host(d["robot_body_angvel"]), z)
                assert same(host(obs), o), t
            else:  # the observation is of the state BEFORE the reset: its position error is not the post-reset one
                assert np.abs(host(obs)[:, 0:3] - host(task.prev_pos_error)).max() > 0.2
                assert (np.abs(host(obs)[:, 0:3] + host(task.prev_position)).max() < 0.2)  # ... but one step from prev_position
            assert same(host(task.prev_actions), host(task.actions))
            assert same(host(task.prev_pos_error), host(task.target_position) - host(d["robot_position"]))
            if t >= 4:
                assert calls[-1] == (n, 4) and same(host(task.actions), host(torch.clamp(a, -1, 1) * 0.25 + 0.75))
        del launches[:]
        task.get_return_tuple()
        task.get_return_tuple()
        assert launches == ["agx_end_to_end_obs"] * 2
        task.close()


def test_make_task_through_the_alias_steps_with_finite_outputs():
    from aerial_gym.config.task_config.position_setpoint_task_sim2real_end_to_end_config import task_config
    from aerial_gym.registry.task_registry import task_registry

    with config_restored(task_config, CONFIG_KEYS):
        task = task_registry.make_task(NAME, num_envs=64)
        assert task.action_limit_max.device.type == "cuda" and task_config.action_limit_max.device.type == "cpu"
        obs = task.reset()[0]
        for _ in range(10):
            obs, rew, term, trunc, info = task.step(torch.rand(64, 4, device=DEV) * 2 - 1)
        torch.cuda.synchronize()
        assert obs["observations"].shape == (64, 15) and torch.isfinite(obs["observations"]).all() and torch.isfinite(rew).all()
        assert rew.shape == (64,) and term.dtype == torch.bool and trunc.dtype == torch.bool and info == {}
        strided = torch.zeros(4, 64, device=DEV).t()
        assert not strided.is_contiguous()
        task.step(strided)  # copied: the tensor is not kept
        for bad in (torch.zeros(64, 4, device=DEV, dtype=torch.float64), torch.zeros(64, 3, device=DEV), torch.zeros(64, 4), [[0.0] * 4] * 64):
            with pytest.raises(ValueError, match="float32 tensor of shape"):
                task.step(bad)
        # exchange rows are refused for the 15-D observation
        rows_ = torch.zeros(2, 64, 18, device=DEV)
        task.sim_env.bind_step_rows(rows_, task.rewards)
        with pytest.raises(RuntimeError, match="step_rows"):
            task.step(torch.zeros(64, 4, device=DEV))
        task.close()


def test_hover_thrust_holds_a_level_tinyprop():
    """64 envs from a level, at-rest start with equal motor thrusts: equal commands of m g / 4 per motor keep |a_z| below 0.05 m/s^2
    once the motors have settled (after 1 s) and every body rate below 1e-3 rad/s.  Loose by construction: the motor model's steady
    state is exact and the products of inertia couple only under rotation."""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    n = 64
    with config_restored(task_registry.get_task_config(NAME), CONFIG_KEYS):
        task = make_task(n, crash_dist=1000.0)
        env, d = task.sim_env, task.obs_dict
        task.reset()
        state = torch.zeros(13, n, device=DEV)
        state[6] = 1.0
        d["robot_state_soa"].copy_(state)
        env.robot_manager.robot.control_allocator.motor_model.thrust_soa.fill_(0.5)
        P = env._params
        hover = P.mass * 9.81 / 4.0
        a = torch.full((n, 4), (hover - 0.7) / 0.5, device=DEV)
        dt = float(d["dt"])
        for _ in range(int(round(1.0 / dt))):
            task.step(a)
        v0 = d["robot_linvel"][:, 2].clone()
        rates = torch.zeros(n, device=DEV)
        k = 20
        for _ in range(k):
            task.step(a)
            rates = torch.maximum(rates, d["robot_angvel"].abs().max(dim=1).values)
        az = (d["robot_linvel"][:, 2] - v0) / (k * dt)
        torch.cuda.synchronize()
        print("hover: |a_z| max %.5f m/s^2  body rate max %.2e rad/s  thrust command %.5f N" % (float(az.abs().max()), float(rates.max()), hover))
        assert not host(d["reset_mask"]).any() and float(az.abs().max()) < 0.05 and float(rates.max()) < 1e-3
        task.close()
