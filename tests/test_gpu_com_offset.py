"""GPU: agx_env_step_com -- the env step of a multirotor whose centre of mass is off the base-link origin (base_random) -- through the
C ABI and through EnvManager, against the restatement of its two pieces on top of the oracle (tests/com_offset_ref.py, pinned by
tests/test_com_offset.py) and against agx_env_step where the two must coincide."""
import copy
import json

import com_offset_ref as CR
import numpy as np
import pytest
import torch
from rov_ref import same
from task_test_util import DEV, derived_of, harness, no_host_sync, npy, split_step, tile
from task_test_util import com_offset as offset
from test_com_offset import RECORDS, load

pytestmark = pytest.mark.gpu
SIZES = (1, 64, 65, 83)
SPLIT_GATE = 2e-5  # fused step against the split path, per step (tests/test_gpu_robot_plugin.py)
GAINS = ("kT", "tau_inc", "tau_dec", "Kp", "Kv", "KR", "Kw")


def step_com(H, action, k, c, P=None):
    from aerial_gym_simulator_amd import _lib

    a = torch.from_numpy(np.ascontiguousarray(action, np.float32)).to(DEV)
    _lib.check(H.lib.agx_env_step_com(P or H.P, H.B, H.n, _lib.dptr(a), k, None, offset(c), H.stream()), "agx_env_step_com")
    torch.cuda.synchronize()


def check_against_restatement(orc, g, pd, n, K, c, label):
    """K = 1: each sub-step of the record on its own; K = 2: both in one launch (the k-loop instance)"""
    P = orc.make_params(pd)
    gains = [tile(g[x], n) for x in GAINS]
    for k0 in ((0, 1) if K == 1 else (0,)):
        dist = np.stack([tile(g["disturb"][k0 + j], n) for j in range(K)])
        H, _ = harness(g, n, k0, pd, dist=dist if dist.any() else None)
        a = tile(g["action"][k0], n)
        step_com(H, a, K, c)
        st, th = tile(g["state"][k0], n).copy(), tile(g["thrust_in"][k0], n).copy()
        for j in range(K):
            o = CR.substep(orc, P, pd, st, a, th, *gains, disturb=dist[j] if dist[j].any() else None, disturb_max=g["disturb_max"], com=c)
        assert same(H.get("state"), st), (label, n, K, k0, float(np.abs(H.get("state") - st).max()))
        assert same(H.get("thrust"), th), (label, n, K, k0)
        for key, got in derived_of(H).items():  # of the last sub-step's pre-physics state
            assert same(got, getattr(o, key)), (label, n, K, k0, key)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", RECORDS)
def test_env_step_com_equals_restatement_plus_oracle_bit_for_bit(orc, name, n):
    """base_random under lee_position_control, lee_attitude_control and no_control, non-zero drag, host disturbance draws, nominal and
    edge records; 1 and 2 fused sub-steps: state, motor thrusts and derived tensors bit for bit"""
    g = load(name, cr=True)
    pd = json.loads(str(g["params_json"]))
    c = CR.com_of(pd)
    assert np.abs(c).max() > 0.02 and g["disturb"].any() and any(pd["lin_drag_quadratic"])
    for K in (1, 2):
        check_against_restatement(orc, g, pd, n, K, c, name)


@pytest.mark.parametrize("n", SIZES)
def test_root_link_mode_with_a_hand_made_offset_on_four_motors(orc, n):
    """the allocator's whole wrench at the root body (root_link_mode), drag and disturbance on top: F_root is the net force; four
    motors, c = (30, -20, 10) mm; 1 and 2 fused sub-steps"""
    from conftest import load_golden

    g = dict(load_golden("step_quad_position", cr=True))
    pd = json.loads(str(g["params_json"]))
    pd.update(root_link_mode=1, lin_drag_linear=[0.031, 0.047, 0.059], lin_drag_quadratic=[0.023, 0.037, 0.053],
              ang_drag_linear=[0.0011, 0.0017, 0.0023], ang_drag_quadratic=[0.0007, 0.0013, 0.0019])
    rng = np.random.default_rng(21)
    d = rng.random(g["disturb"].shape).astype(np.float32)
    d[..., 0] = (d[..., 0] < 0.5).astype(np.float32)
    g["disturb"], g["disturb_max"] = d, np.array([0.75, 0.75, 0.75, 0.004, 0.004, 0.004], np.float32)
    c = np.array([0.03, -0.02, 0.01], np.float32)
    for K in (1, 2):
        check_against_restatement(orc, g, pd, n, K, c, "root_link")
    # the offset is felt: the ordinary entry ends elsewhere
    H, _ = harness(g, n, 0, pd)
    H.substeps(tile(g["action"][0], n), 1)
    H2, _ = harness(g, n, 0, pd)
    step_com(H2, tile(g["action"][0], n), 1, c)
    assert (H.get("state") != H2.get("state")).any(axis=1).all()


@pytest.mark.parametrize("name", ("step_edge_quad_position", "step_edge_octarotor_position", "step_edge_octarotor_fully_actuated", "step_edge_quad_no_control"))
def test_zero_offset_through_the_new_entry_equals_agx_env_step(name):
    """c = 0 means the ordinary dynamics: base_quadrotor and base_octarotor on the edge table, 65 envs, 2 sub-steps in one launch,
    state, thrusts, derived tensors and action tensors bit for bit those of agx_env_step"""
    from conftest import load_golden

    g = load_golden(name, cr=True)
    n = 65
    dist = np.stack([tile(g["disturb"][j], n) for j in range(2)])
    outs = []
    for com in (None, np.zeros(3, np.float32)):
        H, _ = harness(g, n, 0, dist=dist if dist.any() else None)
        a = tile(g["action"][0], n)
        if com is None:
            H.substeps(a, 2)
        else:
            step_com(H, a, 2, com)
        outs.append({k: H.get(k) for k in ("state", "thrust", "derived", "actions", "prev_actions")})
    for key in outs[0]:
        assert same(outs[0][key], outs[1][key]), (name, key)
    assert np.isfinite(outs[0]["state"]).all()


@pytest.mark.parametrize("name", ("step_base_random_position", "step_base_random_no_control"))
def test_fused_step_equals_the_split_path(orc, name):
    """base_random, 83 envs, 3 steps: the one fused launch against robot step -> net body wrench about the centre of mass ->
    integration with AGX_CTRL_WRENCH; thrusts and derived tensors bit for bit, the state within 2e-5 absolute per step (the wrench
    map folded ahead of time against the per-body sum; the root body's lever arm as cross(F_root, c) against r x F with r = -c).
    The integrating launch alone equals the restatement bit for bit.  Measured on an MI355X: at most 1.4e-6."""
    from aerial_gym_simulator_amd.config.robot_config import BaseRandCfg

    n = 83
    g = load(name, cr=True)
    pd = json.loads(str(g["params_json"]))
    c = CR.com_of(pd)
    P = orc.make_params(pd)
    rng = np.random.default_rng(3)
    st, th = tile(g["state"][0], n), tile(g["thrust_in"][0], n)
    for t in range(3):
        a = tile(g["action"][t % 2], n)
        dist = rng.random((1, n, 7)).astype(np.float32)
        dist[..., 0] = (dist[..., 0] < 0.5).astype(np.float32)
        hs = []
        for _ in range(2):
            H, _pd = harness(g, n, 0, pd, dist=dist)
            H.set(state=st, thrust=th)
            hs.append(H)
        Hf, Hs = hs
        step_com(Hf, a, 1, c)
        net = split_step(Hs, BaseRandCfg, a, n, c)
        want = st.copy()
        CR.body_wrench_substep(orc, P, want, net, c)
        assert same(Hs.get("state"), want), t
        assert same(Hf.get("thrust"), Hs.get("thrust")), t
        for key, got in derived_of(Hf).items():
            assert same(got, derived_of(Hs)[key]), (t, key)
        err = float(np.abs(Hf.get("state") - Hs.get("state")).max())
        print("fused vs split", name, "step", t, "max |state difference| %.3e" % err)
        assert err <= SPLIT_GATE, (name, t, err)
        st, th = Hf.get("state"), Hf.get("thrust")


def test_collision_flag_follows_the_base_link_sphere(orc):
    """2 envs, one tiny box each (collision_cases' shapes: a 1 mm box of random orientation placed by the point it touches): env 0's is
    reached by the sphere about the base-link origin p and not by one about the mass centre, env 1's the other way round.  The
    flag is the oracle's predicate at p: 1, 0."""
    from collision_cases import _box, _rand_quat, obb_distance64

    g = load("step_base_random_position", cr=True)
    pd = json.loads(str(g["params_json"]))
    c, r = CR.com_of(pd), np.float32(pd["collision_radius"])
    n = 2
    rows = np.argsort(-np.abs(g["state"][0][:, 10:13]).max(axis=1))[:n]  # two tumbling envs of the record
    sub = {k: np.ascontiguousarray(g[k][rows]) for k in GAINS}
    st, th = np.ascontiguousarray(g["state"][0][rows]), np.ascontiguousarray(g["thrust_in"][0][rows])
    a, dist = np.ascontiguousarray(g["action"][0][rows]), np.ascontiguousarray(g["disturb"][0][rows])
    after = st.copy()
    CR.substep(orc, orc.make_params(pd), pd, after, a, th.copy(), *[sub[k] for k in GAINS], disturb=dist, disturb_max=g["disturb_max"])
    p1 = after[:, 0:3].astype(np.float64)
    com1 = p1 + CR.quat_rotate(after[:, 3:7], np.broadcast_to(c, (n, 3))).astype(np.float64)
    d = (com1 - p1) / np.linalg.norm(com1 - p1, axis=1, keepdims=True)
    assert abs(np.linalg.norm(com1 - p1, axis=1) - np.linalg.norm(c)).max() < 1e-6
    reach = float(r) - 0.006
    touch = np.stack([p1[0] - d[0] * reach, com1[1] + d[1] * reach])  # behind the base link; beyond the mass centre
    rng = np.random.default_rng(8)
    h = np.full((n, 3), 1e-3)
    boxes = _box(touch, _rand_quat(rng, n), h, np.zeros((n, 3)))[:, None, :]  # [n, 1, 10], centred on the touched point
    dp, dc = obb_distance64(p1, boxes[:, 0]), obb_distance64(com1, boxes[:, 0])
    assert dp[0] < r - 0.003 and dc[0] > r + 0.01 and dp[1] > r + 0.01 and dc[1] < r - 0.003, (dp, dc, r)
    want = np.zeros(n, np.uint8)
    orc.collide_sphere_boxes(float(r), after, np.ascontiguousarray(boxes, np.float32), want)
    assert want.tolist() == [1, 0]
    from gpu_harness import DynHarness

    H = DynHarness(pd, n)
    H.set(state=st, thrust=th, kT=sub["kT"], tau_inc=sub["tau_inc"], tau_dec=sub["tau_dec"])
    H.set_gains(*(sub[x] for x in ("Kp", "Kv", "KR", "Kw")))
    H.set_disturb(dist[None], g["disturb_max"])
    H.set_boxes(boxes)
    step_com(H, a, 1, c)
    assert same(H.get("state"), after)
    assert npy(H.crashes).astype(np.uint8).tolist() == [1, 0]


def test_entry_refuses_what_it_does_not_carry():
    """the ROV bit, six motors, an IMU force buffer, the lean step, no offset: AGX_E_ARG with a message, nothing launched (the state
    stays what it was)"""
    from aerial_gym_simulator_amd import _lib
    from conftest import golden_params, load_golden

    g = load("step_base_random_position", cr=True)
    n = 8
    H, pd = harness(g, n, 0)
    c = CR.com_of(pd)
    a = tile(g["action"][0], n)
    before = H.get("state")
    H.B.launch_flags = _lib.LAUNCH_ROV
    with pytest.raises(RuntimeError, match=r"\(-1\).*agx_env_step_com.*AGX_LAUNCH_ROV"):
        step_com(H, a, 1, c)
    H.B.launch_flags = _lib.LAUNCH_LEAN
    with pytest.raises(RuntimeError, match=r"\(-1\).*agx_env_step_com.*AGX_LAUNCH_LEAN"):
        step_com(H, a, 1, c)
    H.B.launch_flags = 0
    force = torch.zeros(3, n, device=DEV)
    H.B.body_force = _lib.dptr(force)
    with pytest.raises(RuntimeError, match=r"\(-1\).*agx_env_step_com.*body_force"):
        step_com(H, a, 1, c)
    H.B.body_force = None
    P6 = copy.copy(H.P)
    P6.num_motors = 6
    with pytest.raises(RuntimeError, match=r"\(-1\).*agx_env_step_com.*num_motors == 4 or 8 \(got 6\)"):
        step_com(H, a, 1, c, P=P6)
    ad = torch.from_numpy(a).to(DEV)
    assert H.lib.agx_env_step_com(H.P, H.B, n, _lib.dptr(ad), 1, None, None, H.stream()) == -1
    torch.cuda.synchronize()
    assert same(H.get("state"), before) and not force.any()
    step_com(H, a, 1, c)  # ... and with none of these it runs
    assert (H.get("state") != before).any()
    q = load_golden("step_quad_no_control")
    assert golden_params(q)["num_motors"] == 4  # (four motors are carried: the root-link test above)


# ---- through EnvManager and the task -----------------------------------------------------------------------------------------
def task_trace(robot_name, monkeypatch, steps=20, n=64):
    """position_setpoint_task with this robot under lee_position_control, device generator: `steps` task steps under the no-sync
    guard, truncations written on the device every fifth step -> (library calls per step, task, states after every step)"""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd.config.task_config import position_setpoint_task_config as cfg
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    saved = (cfg.robot_name, cfg.controller_name, cfg.device)
    cfg.robot_name, cfg.controller_name, cfg.device = robot_name, "lee_position_control", DEV
    try:
        task = task_registry.make_task("position_setpoint_task", seed=3, num_envs=n, headless=True)
    finally:
        cfg.robot_name, cfg.controller_name, cfg.device = saved
    task.reset()
    env = task.sim_env
    g = env.get_obs()
    gen = torch.Generator(device=DEV).manual_seed(6)
    acts = [torch.rand(n, 4, device=DEV, generator=gen) * 2 - 1 for _ in range(steps)]
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask[[1, 17, 40, 63]] = True
    calls, log, real, states = [], [], _lib.check, []

    def check(code, what=""):
        log.append(what)
        return real(code, what)

    monkeypatch.setattr(_lib, "check", check)
    try:
        for t in range(steps):
            del log[:]
            with no_host_sync():
                if t % 5 == 4:
                    env.sim_steps.masked_fill_(mask, int(task.task_config.episode_len_steps) + 1)  # a device-side write: these envs time out in this step
                obs, rew, term, trunc, info = task.step(acts[t])
            calls.append(list(log))
            states.append(npy(g["robot_state_tensor"]))
            if t % 5 == 4:
                steps_now = npy(env.sim_steps)
                assert (steps_now[[1, 17, 40, 63]] == 0).all() and (np.delete(steps_now, [1, 17, 40, 63]) > 0).all(), t  # reset in this step
            assert np.isfinite(npy(rew)).all() and np.isfinite(npy(obs["observations"])).all(), t
    finally:
        monkeypatch.setattr(_lib, "check", real)
    return calls, task, np.stack(states)


def test_position_task_on_base_random_takes_the_general_path_without_host_synchronisation(monkeypatch):
    """position_setpoint_task, robot_name="base_random", lee_position_control, 64 envs, 20 steps with four resets, device generator: no
    host synchronisation; no step plan (neither the two-launch nor the single-launch one) -- the library calls of every step are
    the general path's, those of the same task on base_octarotor with the config's disturbance enabled, with agx_env_step_com in
    place of agx_env_step; the state stays finite and inside a bound"""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config.robot_config import BaseOctarotorCfg
    from aerial_gym_simulator_amd.registry.robot_registry import robot_registry
    from aerial_gym_simulator_amd.robots.base_multirotor import BaseMultirotor

    calls, task, states = task_trace("base_random", monkeypatch)
    env = task.sim_env
    assert task._plan is None and env._com is not None and env.robot_manager.robot.com_offset is env._com
    assert len(calls) == 20 and all("agx_env_step_com" in c and "agx_env_step" not in c and "agx_position_task_step" not in c for c in calls), calls[:2]

    class OctarotorDisturbedCfg(BaseOctarotorCfg):  # the general path of a robot without an offset: disturbance on, like base_random's
        class disturbance(BaseOctarotorCfg.disturbance):
            enable_disturbance = True

    robot_registry.register("toy_octarotor_disturbed", BaseMultirotor, OctarotorDisturbedCfg)
    calls_octa, task_octa, _ = task_trace("toy_octarotor_disturbed", monkeypatch)
    assert task_octa._plan is None and task_octa.sim_env._com is None
    assert [[w.replace("agx_env_step_com", "agx_env_step") for w in c] for c in calls] == calls_octa, (calls[:5], calls_octa[:5])
    print("base_random task step:", calls[0], "| with resets:", calls[4])
    assert np.isfinite(states).all()
    assert np.abs(states[:, :, 0:3]).max() < 50.0 and np.abs(states[:, :, 7:10]).max() < 100.0 and np.abs(states[:, :, 10:13]).max() <= 100.0 + 1e-3
    assert np.abs(np.linalg.norm(states[:, :, 3:7], axis=2) - 1).max() < 1e-5
