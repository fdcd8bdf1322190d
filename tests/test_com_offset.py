"""CPU: the airframes base_random and lmf1 as config data against the composites of the reference's URDFs, and the restatement of the
env step about a centre of mass off the base-link origin (tests/com_offset_ref.py, the comparator of tests/test_gpu_com_offset.py):
it conserves what it must, reduces to the oracle's step at c = 0, and carries the fixtures' states from one sub-step to the next."""
import json
import os

import com_offset_ref as CR
import numpy as np
import pytest
from rov_ref import disturb_of, same

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
RECORDS = ("step_base_random_position", "step_base_random_attitude", "step_base_random_no_control", "step_edge_base_random_position",
           "step_edge_base_random_attitude")


def load(name, cr=False):
    return np.load(os.path.join(GOLDEN, *(["com_cr"] if cr else []), name + ".npz"))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def test_base_random_is_the_composite_of_its_urdf():
    """BaseRandCfg.robot_model (data) == composite of resources/robots/random/random.urdf, in float64 to 1e-12 relative: mass, centre
    of mass (22.44, 1.75, -2.63) mm off the base-link origin, inertia, the 6 x 8 wrench map about the centre of mass; and the
    numbers of the config"""
    from aerial_gym_simulator_amd.config.robot_config import BaseRandCfg
    from aerial_gym_simulator_amd.robots.robot_model import composite_body, motor_wrench_map

    r = np.load(os.path.join(GOLDEN, "robot_base_random.npz"))
    m, com, J = composite_body(BaseRandCfg.robot_model)
    assert abs(m - float(r["mass"])) <= 1e-12 * float(r["mass"]) and rel(com, r["com"]) <= 1e-12 and rel(J, r["inertia"]) <= 1e-12
    assert np.allclose(com, [0.02243687, 0.00175, -0.002625], atol=5e-9) and abs(m - 0.25) < 1e-15
    ca, mm = BaseRandCfg.control_allocator_config, BaseRandCfg.control_allocator_config.motor_model_config
    W = motor_wrench_map(BaseRandCfg.robot_model, ca.motor_directions, mm.thrust_to_torque_ratio, com)
    assert rel(W, r["wrench_map"]) <= 1e-12
    assert BaseRandCfg.robot_model.collision_sphere_radius == float(r["collision_radius"])
    assert list(r["application_mask"]) == list(ca.application_mask) and list(r["motor_directions"]) == list(ca.motor_directions)
    assert str(r["force_application_level"]) == ca.force_application_level == "motor_link"
    assert np.array_equal(r["alloc"], np.array(ca.allocation_matrix, np.float64))
    assert list(r["motor_model"]) == [mm.motor_thrust_constant_min, mm.motor_thrust_constant_max, mm.motor_time_constant_increasing_min,
                                      mm.motor_time_constant_increasing_max, mm.motor_time_constant_decreasing_min,
                                      mm.motor_time_constant_decreasing_max, mm.max_thrust, mm.min_thrust, mm.max_thrust_rate, mm.thrust_to_torque_ratio]
    assert json.loads(str(r["motor_model_flags"])) == dict(use_rps=False, use_discrete_approximation=True, integration_scheme=None)
    assert not mm.use_rps and mm.use_discrete_approximation
    assert np.array_equal(r["min_init_state"], np.array(BaseRandCfg.init_config.min_init_state, np.float64))
    assert np.array_equal(r["max_init_state"], np.array(BaseRandCfg.init_config.max_init_state, np.float64))
    assert np.array_equal(r["min_state_ratio"], np.array(BaseRandCfg.robot_asset.min_state_ratio, np.float64))
    assert np.array_equal(r["max_state_ratio"], np.array(BaseRandCfg.robot_asset.max_state_ratio, np.float64))
    d = BaseRandCfg.disturbance
    assert list(r["disturbance"]) == [float(d.enable_disturbance), d.prob_apply_disturbance] + list(d.max_force_and_torque_disturbance)
    assert d.enable_disturbance and not r["drag_coefficients"].any() and not r["sensors"].any()
    assert list(r["damping"]) == [BaseRandCfg.robot_asset.linear_damping, BaseRandCfg.robot_asset.angular_damping]
    a = json.loads(str(r["asset"]))
    assert (a["file"], a["name"]) == (BaseRandCfg.robot_asset.file, BaseRandCfg.robot_asset.name)


def test_base_random_allocation_matrix_is_the_wrench_map_about_the_base_link_origin():
    """the reference computed BaseRandCfg.allocation_matrix about the base-link ORIGIN, not the centre of mass: equal to the URDF's
    wrench map with arms = the joint xyz to 1e-7 absolute (the config prints eight decimals; measured 4.9e-10, all six rows) -- and
    NOT equal to the map about the centre of mass, which is what the airframe flies by"""
    from aerial_gym_simulator_amd.config.robot_config import BaseRandCfg
    from aerial_gym_simulator_amd.robots.robot_model import composite_body, motor_wrench_map

    r = np.load(os.path.join(GOLDEN, "robot_base_random.npz"))
    ca = BaseRandCfg.control_allocator_config
    A = np.array(ca.allocation_matrix, np.float64)
    W0 = motor_wrench_map(BaseRandCfg.robot_model, ca.motor_directions, ca.motor_model_config.thrust_to_torque_ratio, np.zeros(3))
    print("max |allocation_matrix - wrench map about the origin| per row:", np.abs(A - W0).max(axis=1))
    assert np.abs(A - W0).max() <= 1e-7 and np.abs(A - r["wrench_map_origin"]).max() <= 1e-7
    _, com, _ = composite_body(BaseRandCfg.robot_model)
    W = motor_wrench_map(BaseRandCfg.robot_model, ca.motor_directions, ca.motor_model_config.thrust_to_torque_ratio, com)
    assert np.abs(A[0:3] - W[0:3]).max() <= 1e-7 and np.abs(A[3:6] - W[3:6]).max() > 1e-2  # |c| = 22.6 mm of lever arm


def test_lmf1_is_the_composite_of_its_urdf_and_its_mass_centre_is_the_base_link():
    from aerial_gym_simulator_amd.config.robot_config import LMF1Cfg
    from aerial_gym_simulator_amd.config.sim_config import BaseSimConfig
    from aerial_gym_simulator_amd.robots.robot_model import composite_body, motor_wrench_map, pack_com_offset, robot_params_dict

    r = np.load(os.path.join(GOLDEN, "robot_lmf1.npz"))
    m, com, J = composite_body(LMF1Cfg.robot_model)
    assert abs(m - float(r["mass"])) <= 1e-12 * float(r["mass"]) and rel(J, r["inertia"]) <= 1e-12
    assert not com.any() and not r["com"].any()  # exactly 0
    ca, mm = LMF1Cfg.control_allocator_config, LMF1Cfg.control_allocator_config.motor_model_config
    W = motor_wrench_map(LMF1Cfg.robot_model, ca.motor_directions, mm.thrust_to_torque_ratio, com)
    assert rel(W, r["wrench_map"]) <= 1e-12 and np.array_equal(np.array(LMF1Cfg.robot_model.motor_xyz), r["motor_pos"])
    assert list(r["application_mask"]) == list(ca.application_mask) == [4, 1, 3, 2] and list(r["motor_directions"]) == list(ca.motor_directions)
    assert np.array_equal(r["alloc"], np.array(ca.allocation_matrix, np.float64)) and str(r["force_application_level"]) == ca.force_application_level
    assert list(r["motor_model"]) == [mm.motor_thrust_constant_min, mm.motor_thrust_constant_max, mm.motor_time_constant_increasing_min,
                                      mm.motor_time_constant_increasing_max, mm.motor_time_constant_decreasing_min,
                                      mm.motor_time_constant_decreasing_max, mm.max_thrust, mm.min_thrust, mm.max_thrust_rate, mm.thrust_to_torque_ratio]
    assert json.loads(str(r["motor_model_flags"]))["use_discrete_approximation"] is False and not mm.use_discrete_approximation
    assert np.array_equal(r["min_init_state"], np.array(LMF1Cfg.init_config.min_init_state, np.float64))
    assert np.array_equal(r["max_init_state"], np.array(LMF1Cfg.init_config.max_init_state, np.float64))
    assert np.array_equal(r["min_state_ratio"], np.array(LMF1Cfg.robot_asset.min_state_ratio, np.float64))
    assert np.array_equal(r["max_state_ratio"], np.array(LMF1Cfg.robot_asset.max_state_ratio, np.float64))
    assert not r["disturbance"].any() and not LMF1Cfg.disturbance.enable_disturbance and not r["sensors"].any()
    assert list(r["damping"]) == [LMF1Cfg.robot_asset.linear_damping, LMF1Cfg.robot_asset.angular_damping] == [0.02, 0.02]
    pd = robot_params_dict(LMF1Cfg, None, "none", BaseSimConfig)
    assert pd["com"] == [0.0, 0.0, 0.0] and pack_com_offset(pd) is None and pd["root_link_mode"] == 0


def test_registry_params_and_the_offset_handed_out():
    import aerial_gym_simulator_amd as ag
    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd.config.robot_config import BaseRandCfg, LMF1Cfg
    from aerial_gym_simulator_amd.config.sim_config import BaseSimConfig
    from aerial_gym_simulator_amd.robots.base_multirotor import BaseMultirotor
    from aerial_gym_simulator_amd.robots.robot_model import composite_body, pack_com_offset, robot_params_dict

    from aerial_gym.config.robot_config.base_random_config import BaseRandCfg as alias_rand  # the reference's import paths
    from aerial_gym.config.robot_config.lmf1_config import LMF1Cfg as alias_lmf1

    assert alias_rand is BaseRandCfg and alias_lmf1 is LMF1Cfg
    assert ag.robot_registry.get_robot_config("base_random") is BaseRandCfg and ag.robot_registry.get_robot_config("lmf1") is LMF1Cfg
    assert ag.robot_registry.get_robot_class("base_random") is BaseMultirotor is ag.robot_registry.get_robot_class("lmf1")
    pd = robot_params_dict(BaseRandCfg, None, "none", BaseSimConfig)
    _, com, _ = composite_body(BaseRandCfg.robot_model)
    assert same(np.float32(pd["com"]), com.astype(np.float32))  # float64, rounded to fp32 once
    C = pack_com_offset(pd)
    assert isinstance(C, _lib.AgxComOffset) and list(C.c) == pd["com"] and C.reserved == 0.0
    g = load("step_base_random_position", cr=True)
    fx = json.loads(str(g["params_json"]))
    for key in ("com", "mass", "inertia", "inertia_inv", "wrench_map", "alloc", "min_thrust", "max_thrust", "cq", "use_rps", "num_motors",
                "root_link_mode", "linear_damping", "angular_damping", "collision_radius", "use_discrete_approximation"):
        assert same(np.float32(pd[key]), np.float32(fx[key])), key
    header = open(os.path.join(os.path.dirname(HERE), "include", "aerial_gym_hip.h")).read()
    assert "int agx_env_step_com(" in header and "agx_env_step_com" in _lib.EXPORTED_SYMBOLS and _lib.ABI_VERSION >= 19


def test_task_less_build_env_on_the_cpu_and_the_refused_combinations():
    """base_random builds like any multirotor (17 bodies, 8 motors, the offset on the robot); an IMU on it, an ROV with an offset and
    the lean step are refused in words"""
    import torch
    from aerial_gym.sim.sim_builder import SimBuilder

    import aerial_gym_simulator_amd as ag
    from aerial_gym_simulator_amd.config.robot_config import BaseRandCfg, BaseROVCfg
    from aerial_gym_simulator_amd.config.sensor_config import BaseImuConfig
    from aerial_gym_simulator_amd.robots.base_multirotor import BaseMultirotor
    from aerial_gym_simulator_amd.robots.base_rov import BaseROV

    def build(robot, controller="lee_position_control", sim="base_sim"):
        return SimBuilder().build_env(sim_name=sim, env_name="empty_env", robot_name=robot, controller_name=controller, device="cpu", args=None,
                                      num_envs=4, headless=True, use_warp=False)

    env = build("base_random")
    rob = env.robot_manager.robot
    assert rob.com_offset is not None and rob.params.num_motors == 8 and env.get_obs()["robot_force_tensor"].shape == (4, 17, 3)
    assert not rob.external_robot and not rob.external_controller
    with pytest.raises(RuntimeError, match="HIP device"):
        env.step(torch.zeros(4, 4))
    assert build("lmf1").robot_manager.robot.com_offset is None

    class RandWithImuCfg(BaseRandCfg):
        class sensor_config(BaseRandCfg.sensor_config):
            enable_imu = True
            imu_config = BaseImuConfig

    ag.robot_registry.register("toy_base_random_with_imu", BaseMultirotor, RandWithImuCfg)
    with pytest.raises(ValueError, match="enable_imu.*lever-arm"):
        build("toy_base_random_with_imu")

    class OffCentreROVCfg(BaseROVCfg):
        class robot_model(BaseROVCfg.robot_model):
            links = list(getattr(BaseROVCfg.robot_model, "links", None) or []) + [
                dict(name="payload", parent="base_link", mass=0.5, xyz=[0.1, 0.0, 0.0], rpy=[0.0, 0.0, 0.0], inertia=[[0.0] * 3] * 3)]

    ag.robot_registry.register("toy_off_centre_rov", BaseROV, OffCentreROVCfg)
    with pytest.raises(ValueError, match="BaseROV.*centre of mass"):
        build("toy_off_centre_rov", "fully_actuated_control", "base_sim_no_gravity")


def tumbling(orc, c, steps=200):
    """200 steps of a free body (no wrench, no gravity, no damping) tumbling at |w| = 10 rad/s -> (states [steps + 1, 13] of the
    restatement in fp32, base-link positions of its float64 twin [steps + 1, 3])"""
    from aerial_gym_simulator_amd.config.robot_config import BaseRandCfg
    from aerial_gym_simulator_amd.config.sim_config import BaseSimConfig
    from aerial_gym_simulator_amd.robots.robot_model import robot_params_dict

    pd = dict(robot_params_dict(BaseRandCfg, None, "none", BaseSimConfig))
    pd.update(controller="no_control", gravity=[0.0, 0.0, 0.0], linear_damping=0.0, angular_damping=0.0)
    P = orc.make_params(pd)
    w = np.array([3.0, 8.0, 5.0]) / np.linalg.norm([3.0, 8.0, 5.0]) * 10.0
    st = np.zeros((1, 13), np.float32)
    st[0, 0:3], st[0, 6], st[0, 7:10], st[0, 10:13] = [0.3, -0.7, 1.1], 1.0, [0.9, -0.4, 0.25], w
    states = [st.copy()]
    for _ in range(steps):
        CR.body_wrench_substep(orc, P, st, np.zeros((1, 6), np.float32), c)
        states.append(st.copy())
    states = np.concatenate(states)
    # the float64 twin: the same recursion p += v dt + (R(q) c - R(q') c) on the attitudes of the fp32 run, every operation in float64
    q = states[:, 3:7].astype(np.float64)
    Rc = rotate64(q, np.asarray(c, np.float64))
    v, dt = states[:, 7:10].astype(np.float64), np.float64(np.float32(pd["dt"]))
    p64 = [states[0, 0:3].astype(np.float64)]
    for k in range(steps):
        p64.append((p64[-1] + v[k + 1] * dt) + (Rc[k] - Rc[k + 1]))
    return states, np.array(p64), Rc, dt


def rotate64(q, c):
    """R(q) c in float64, q xyzw [K, 4] (normalised here: the fp32 attitudes are unit to 1e-7)"""
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    u, w = q[:, 0:3], q[:, 3:4]
    cc = np.broadcast_to(c, u.shape)
    t = 2.0 * np.cross(u, cc)
    return cc + w * t + np.cross(u, t)


@pytest.mark.parametrize("scale", (1.0, 100.0))
def test_restatement_moves_the_mass_centre_in_a_straight_line(orc, scale):
    """No wrench, no gravity, no damping, |w| = 10 rad/s, c of base_random and 100 times it: over 200 steps the mass centre
    p + R(q) c advances by sum v dt while the base-link origin p circles it.  Bound: the accumulated fp32 rounding of the recursion,
    measured here as the distance of the fp32 run from its float64 twin (the same sum in float64 on the same attitudes), times 4 --
    the twin shares the formula, so a formula that does not conserve fails against the straight line, not against the twin.
    Measured: rounding 1.10e-5 m at c (|c| = 22.7 mm), 1.15e-5 m at 100 c (|c| = 2.27 m) -- mostly the biased rounding of the
    constant v dt added to p = 1 .. 2 m, which the ordinary step has too; the mass centre's distance from the straight line is the
    same 1.10e-5 / 1.15e-5 m; p itself leaves the line by 45 mm / 4.5 m (2 |c|)."""
    from aerial_gym_simulator_amd.config.robot_config import BaseRandCfg
    from aerial_gym_simulator_amd.robots.robot_model import composite_body

    c = composite_body(BaseRandCfg.robot_model)[1].astype(np.float32) * np.float32(scale)
    states, p64, Rc, dt = tumbling(orc, c)
    steps = len(states) - 1
    p32 = states[:, 0:3].astype(np.float64)
    assert same(states[:, 7:10], np.broadcast_to(states[0, 7:10], (steps + 1, 3)))  # nothing accelerates the mass centre
    rounding = float(np.abs(p32 - p64).max())
    line = (p32[0] + Rc[0])[None, :] + np.arange(steps + 1)[:, None] * (states[0, 7:10].astype(np.float64) * dt)[None, :]
    off_line = float(np.abs((p32 + Rc) - line).max())
    wander = float(np.linalg.norm(p32 - (p32[0][None, :] + (line - line[0])), axis=1).max())
    print("scale %g: fp32 rounding of the recursion %.3e m, mass centre off the straight line %.3e m, base link off it %.3e m (|c| = %.4f m)"
          % (scale, rounding, off_line, wander, np.linalg.norm(c)))
    # what fp32 can do to such a sum at most: per step three roundings of numbers below max |p| + 2 |c|, each half an ulp
    assert 0 < rounding <= steps * 3 * 2.0 ** -24 * (np.abs(p32).max() + 2 * np.abs(c).max())
    assert off_line <= 4 * rounding
    assert wander > np.linalg.norm(c)  # ... while p does not: it circles the mass centre


def test_zero_offset_is_the_oracles_step_bit_for_bit(orc):
    for name in RECORDS:
        g = load(name, cr=True)
        pd = json.loads(str(g["params_json"]))
        P = orc.make_params(pd)
        for k in range(g["state"].shape[0]):
            dist = disturb_of(g, k)
            args = [g[x] for x in ("kT", "tau_inc", "tau_dec", "Kp", "Kv", "KR", "Kw")]
            s0, t0 = g["state"][k].copy(), g["thrust_in"][k].copy()
            s1, t1 = s0.copy(), t0.copy()
            orc.substep(P, s0, g["action"][k], t0, *args, disturb=dist, disturb_max=g["disturb_max"], integrate=True)
            CR.substep(orc, P, pd, s1, g["action"][k], t1, *args, disturb=dist, disturb_max=g["disturb_max"], com=np.zeros(3, np.float32))
            assert same(s0, s1) and same(t0, t1), (name, k)


def test_restatement_carries_the_fixtures_from_one_sub_step_to_the_next(orc):
    """the fixtures' second state is the first advanced from the REFERENCE's per-body force and torque tensors (motor links' sum, root
    body's entry with its lever arm); the restatement gets there from the oracle's wrench: bit for bit on the correctly rounded
    records, and what the reference's robot stored on the way (thrusts, derived tensors, clipped action) bit for bit too.  The
    offset matters: with c = 0 the same step ends elsewhere in every row."""
    for name in RECORDS:
        g = load(name, cr=True)
        pd = json.loads(str(g["params_json"]))
        assert np.abs(pd["com"]).max() > 0.02
        P = orc.make_params(pd)
        args = [g[x] for x in ("kT", "tau_inc", "tau_dec", "Kp", "Kv", "KR", "Kw")]
        for k in range(g["state"].shape[0]):
            dist = disturb_of(g, k)
            st, th = g["state"][k].copy(), g["thrust_in"][k].copy()
            o = CR.substep(orc, P, pd, st, g["action"][k], th, *args, disturb=dist, disturb_max=g["disturb_max"])
            for key, got in (("euler", o.euler), ("qveh", o.qveh), ("vveh", o.vveh), ("vbody", o.vbody), ("wbody", o.wbody)):
                assert same(got, g[key][k]), (name, k, key)
            assert same(th, g["thrust_out"][k]) and same(o.action_clipped, g["action_after"][k]), (name, k)
            assert same(CR.root_force(o.vbody, pd, dist, g["disturb_max"]), g["force"][k][:, 0, :]), (name, k)
            if k + 1 < g["state"].shape[0]:
                assert same(st, g["state"][k + 1]), (name, k)
                plain = g["state"][k].copy()
                orc.substep(P, plain, g["action"][k], g["thrust_in"][k].copy(), *args, disturb=dist, disturb_max=g["disturb_max"], integrate=True)
                moving = np.abs(g["state"][k][:, 10:13]).max(axis=1) > 0
                assert (plain[moving, 0:3] != st[moving, 0:3]).any(axis=1).all() and moving.sum() > 32, name
