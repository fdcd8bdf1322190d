"""CPU: pins the C oracle against golden vectors produced by the REFERENCE's own torch code
(tests/golden/*.npz, oracle/gen_golden.py).  Tolerances are relative to 1 + max|ref|."""
import numpy as np
import pytest
from conftest import golden_params, load_golden, rel_err
from edge_cases_util import EDGE_CASES, gates_vs_reference

STEP_CASES = ["quad_position", "quad_velocity", "quad_attitude", "quad_acceleration", "quad_no_control",
              "octarotor_position", "octarotor_velocity", "octarotor_fully_actuated", "quad_rates", "quad_velocity_steering"]


def test_math_helpers(orc):
    g = load_golden("math_utils")
    n = g["q"].shape[0]
    assert rel_err(orc.quat_mul(g["q"], g["q2"]), g["quat_mul"]) < 1e-6
    assert rel_err(orc.quat_from_euler(g["e"]), g["quat_from_euler"]) < 1e-6
    assert rel_err(orc.tf_apply(g["q"], g["t"], g["v"]), g["tf_apply"]) < 1e-6
    state = np.zeros((n, 13), np.float32)
    state[:, 3:7], state[:, 7:10], state[:, 10:13] = g["q"], g["v"], g["v"]
    euler, qveh, vveh, vbody, wbody = orc.update_states(state)
    # angles are compared modulo 2 pi (ssa wraps at +-pi)
    d = np.abs(euler - g["ssa_euler"])
    assert np.minimum(d, 2 * np.pi - d).max() < 2e-6
    assert rel_err(qveh, g["vehicle_quat"]) < 1e-6
    assert rel_err(vbody, g["quat_rotate_inverse"]) < 1e-6
    assert rel_err(wbody, g["quat_rotate_inverse"]) < 1e-6


@pytest.mark.parametrize("case", STEP_CASES + EDGE_CASES)
def test_substep_matches_reference(orc, case):
    """BaseMultirotor.step of the reference vs orc_substep (rows a1-a14)."""
    g = load_golden("step_" + case)
    pd = golden_params(g)
    P = orc.make_params(pd)
    W = np.array(pd["wrench_map"], np.float32).reshape(6, -1)
    mask = g["application_mask"]
    for k in range(g["state"].shape[0]):
        st, th = g["state"][k].copy(), g["thrust_in"][k].copy()
        dist = g["disturb"][k] if g["disturb"][k].any() else None
        o = orc.substep(P, st, g["action"][k], th, g["kT"], g["tau_inc"], g["tau_dec"], g["Kp"], g["Kv"], g["KR"],
                        g["Kw"], disturb=dist, disturb_max=g["disturb_max"], integrate=False)
        d = np.abs(o.euler - g["euler"][k])
        assert np.minimum(d, 2 * np.pi - d).max() < 2e-6
        for name, got in (("qveh", o.qveh), ("vveh", o.vveh), ("vbody", o.vbody), ("wbody", o.wbody)):
            assert rel_err(got, g[name][k]) < 1e-6, (case, k, name)
        if "no_control" not in case:
            assert rel_err(o.wrench_cmd, g["wrench_cmd"][k]) < 2e-6, (case, k)
        assert rel_err(th, g["thrust_out"][k]) < 5e-6, (case, k)
        assert rel_err(o.action_clipped, g["action_after"][k]) < 1e-7, (case, k)
        u = g["force"][k][:, mask, 2]
        bw = u @ W.T
        bw[:, 0:3] += g["force"][k][:, 0, :]
        bw[:, 3:6] += g["torque"][k][:, 0, :]
        assert rel_err(o.body_wrench, bw) < 3e-6, (case, k)
        # per-motor force / torque tensors of control_allocation.py:103-114
        cq, md = pd["cq"], np.array(pd["motor_dir"], np.float32)[: pd["num_motors"]]
        assert rel_err(g["torque"][k][:, mask, 2], -cq * md[None, :] * th) < 5e-6


@pytest.mark.parametrize("case", STEP_CASES + EDGE_CASES)
def test_robot_step_per_body_tensors_match_reference(orc, parity, case):
    """VERDICT r05 missing-5: robot_force_tensor / robot_torque_tensor as the reference's BaseMultirotor.step leaves them
    (base_multirotor.py:236-285, recorded by oracle/gen_golden.py as `force` / `torque`: [K][N][bodies][3]) vs orc.robot_step --
    the function the GPU's agx_robot_step is pinned to bit for bit (tests/test_gpu_robot_plugin.py) -- ENTRY BY ENTRY."""
    g = load_golden("step_" + case)
    pd = golden_params(g)
    P = orc.make_params(pd)
    mask = [int(b) for b in g["application_mask"]]
    NB = g["force"].shape[2]
    worst = 0.0
    for k in range(g["state"].shape[0]):
        th = g["thrust_in"][k].copy()
        dist = g["disturb"][k] if g["disturb"][k].any() else None
        o, F, T = orc.robot_step(P, g["state"][k].copy(), g["action"][k], th, g["kT"], g["tau_inc"], g["tau_dec"], g["Kp"], g["Kv"], g["KR"], g["Kw"],
                                 NB, mask, disturb=dist, disturb_max=g["disturb_max"])
        assert F.shape == g["force"][k].shape and T.shape == g["torque"][k].shape
        for got, ref in ((F, g["force"][k]), (T, g["torque"][k])):
            err = float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())
            worst = max(worst, err)
            assert err <= 1e-5, (case, k, err)
            assert np.array_equal(got == 0.0, ref == 0.0) or err <= 1e-7  # the same bodies carry a wrench
        assert rel_err(th, g["thrust_out"][k]) < 5e-6
    parity.record("robot_step_per_body_vs_reference[%s]" % case, worst, 1e-5)


@pytest.mark.parametrize("case", EDGE_CASES)
def test_edge_table_is_defined_by_the_reference(orc, parity, case):
    """The edge fixtures (every attitude, controller edge inputs: tests/edge_cases_util.py) with the oracle in the kernels' place:
    every element within 1e-5 max(1, |x|) of the reference's recorded answer, no non-finite value on either side, and at most
    1 % of any array where the reference's own answer is not defined to that gate -- the table the GPU tests run the kernels on
    (tests/test_gpu_dynamics_edge_states.py) is one the reference decides."""
    g = load_golden("step_" + case)
    pd = golden_params(g)
    P = orc.make_params(pd)
    fs = max(abs(pd["max_thrust"]), abs(pd["min_thrust"]))
    assert g["state"].shape[:2] == (2, 96)
    for k in range(g["state"].shape[0]):
        st, th = g["state"][k].copy(), g["thrust_in"][k].copy()
        dist = g["disturb"][k] if g["disturb"][k].any() else None
        o = orc.substep(P, st, g["action"][k], th, g["kT"], g["tau_inc"], g["tau_dec"], g["Kp"], g["Kv"], g["KR"],
                        g["Kw"], disturb=dist, disturb_max=g["disturb_max"], integrate=True)
        got = dict(euler=o.euler, qveh=o.qveh, vveh=o.vveh, vbody=o.vbody, wbody=o.wbody, wrench=o.wrench_cmd, thrust=th, next_state=st)
        for name, x in got.items():
            assert np.isfinite(x).all() and np.isfinite(g["euler"][k]).all(), (case, k, name)
        gates_vs_reference(parity, "oracle_edge_substep", case, g, k, got, fs)


def test_edge_table_holds_the_rows_it_is_made_for():
    """what the generator asserted when it wrote the fixtures, re-read from them: the exact-clamp rows have |sinp| >= 1 in float32
    (one above 1), the rows next to them sit one ulp under 1, and some row has cosr_cosp == 0 / cosy_cosp == 0 exactly"""
    g = load_golden("step_edge_quad_position")
    q = g["state"][0][:, 3:7]
    x, y, z, w = (q[:, i] for i in range(4))
    sinp = np.float32(2.0) * (w * y - z * x)
    assert sinp.dtype == np.float32 and sinp[7] == 1.0 and sinp[8] == -1.0 and sinp[9] > 1.0
    assert sinp[5] == np.nextafter(np.float32(1), np.float32(0)) and sinp[6] == -sinp[5]
    cosr_cosp, cosy_cosp = w * w - x * x - y * y + z * z, w * w + x * x - y * y - z * z
    assert (cosr_cosp[:24] == 0).any() and (cosy_cosp[:24] == 0).any()
    assert ((cosr_cosp < 0) & (cosy_cosp < 0)).sum() >= 8  # inverted attitudes: both atan2 denominators negative
    v, w_ = np.abs(g["state"][0][:, 7:10]).max(1), np.abs(g["state"][0][:, 10:13]).max(1)
    assert (v == 0).sum() >= 16 and (v > 5).sum() >= 16 and (w_ == 0).sum() >= 16 and (w_ > 5).sum() >= 16
    go = load_golden("step_edge_octarotor_velocity")
    pd = golden_params(go)
    th = go["thrust_in"][0]
    assert (th == pd["min_thrust"]).any() and (th == pd["max_thrust"]).any() and (th == 0).any() and ((th < 0) & (th > -0.2)).any()


def test_hover_equilibrium_kat(orc):
    """KAT: Lee position control at the setpoint, level, at rest => thrust = m g, torque = 0."""
    g = load_golden("step_quad_position")
    pd = golden_params(g)
    P = orc.make_params(pd)
    n = 4
    st = np.zeros((n, 13), np.float32)
    st[:, 6] = 1.0
    th = np.full((n, 4), 0.6, np.float32)
    o = orc.substep(P, st, np.zeros((n, 4), np.float32), th, g["kT"][:n], g["tau_inc"][:n], g["tau_dec"][:n],
                    g["Kp"][:n], g["Kv"][:n], g["KR"][:n], g["Kw"][:n], integrate=False)
    assert np.allclose(o.wrench_cmd[:, 2], 0.25 * 9.81, rtol=1e-6)
    assert np.abs(o.wrench_cmd[:, 3:]).max() < 1e-7


def test_allocation_identity_kat(orc):
    """A A+ w = w on the quad's rank-4 subspace (control_allocation.py:32-34 warns rank 4)."""
    pd = golden_params(load_golden("step_quad_position"))
    A = np.array(pd["alloc"], np.float64).reshape(6, 4)
    Ap = np.array(pd["alloc_pinv"], np.float64).reshape(4, 6)
    w = np.array([0, 0, 2.4, 0.01, -0.02, 0.003])
    assert np.allclose(A @ (Ap @ w), w, atol=1e-7)


def test_octarotor_wrench_map_differs_from_allocation():
    """The octarotor config's allocation matrix embeds cq = 0.1 while the motor model applies
    cq = 0.01 at the links: the physically applied wrench (URDF frames) is NOT A u."""
    r = load_golden("robot_octarotor")
    assert np.abs(r["wrench_map"][:3] - r["alloc"][:3]).max() < 1e-7
    assert np.abs(r["wrench_map"][3:] - r["alloc"][3:]).max() > 0.05
    q = load_golden("robot_quad")
    assert np.abs(q["wrench_map"] - q["alloc"]).max() < 1e-12


def test_position_reward_and_obs(orc):
    g = load_golden("reward_position")
    crashes = g["crashes_in"].astype(np.uint8)
    r = orc.reward_position(g["state"], g["qveh"], g["wbody"], g["target"], crashes)
    assert rel_err(r, g["reward"]) < 2e-6
    assert np.array_equal(crashes.astype(bool), g["crashes_out"])
    assert np.array_equal(orc.obs_position(g["state"], g["vbody"], g["wbody"], g["target"]), g["obs"])


def test_navigation_reward(orc):
    g = load_golden("reward_navigation")
    pe = np.ascontiguousarray(g["prev_pos_err"]).copy()  # becomes "current" inside, then prev <- cur
    ppe = np.zeros_like(pe)
    r = orc.reward_navigation(g["state"], g["qveh"], g["target"], g["action"], g["prev_action"],
                              float(g["curriculum_progress"]), g["rp"], pe, ppe, g["crashes"].astype(np.uint8))
    assert rel_err(pe, g["pos_err"]) < 1e-6
    assert rel_err(ppe, g["prev_pos_err"]) == 0.0
    assert rel_err(r, g["reward"]) < 3e-6


from trace_util import TRACES, run_trace_against  # noqa: E402


@pytest.mark.parametrize("tag", list(TRACES))
def test_trace_config1(orc, tag):
    """BASELINE config 1 (64 envs, empty_env): oracle loop vs the trace assembled from the reference's control /
    reward / reset code (+ oracle integrator).  `position_long` is SURVEY 8d's 1000-step trace with the task's real
    episode length: 500 steps at the zero set-point (gated at 1e-4), the truncation reset of all envs, then 500 steps
    of U(-1, 1) set-points held for 25 steps each, where fp32 rounding differences (~1e-6 per step in the body rates)
    are amplified by the manoeuvres: that half reports its first-divergence step."""
    from conftest import max_abs
    from oracle_env import OraclePositionEnv

    name, gate_steps, tail_gate = TRACES[tag]
    g = load_golden(name)
    pd = golden_params(g)
    n = g["init_state"].shape[0]
    ranges = dict(tau_inc=(0.04, 0.04), tau_dec=(0.04, 0.04), thrust=(0.0, 2.0), kT=(0.00000926312, 0.00001826312))
    env = OraclePositionEnv(pd, n, int(g["episode_len"]), (g["Kp"], g["Kv"], g["KR"], g["Kw"]),
                            g["min_init_state"], g["max_init_state"], ranges)
    env.reset_masked(np.ones(n, np.uint8), g["init_u_state"], g["init_u_tau_inc"], g["init_u_tau_dec"],
                     g["init_u_thrust"], g["init_u_kT"])
    assert max_abs(env.state, g["init_state"]) < 1e-6
    assert rel_err(env.thrust, g["init_thrust"]) < 1e-6
    assert rel_err(env.kT, g["init_kT"]) < 1e-6
    first_state = []

    def step(t, action, draws):
        obs, rew, crashes, trunc, reset_mask, state_after = env.step(action, draws)
        if t == 0:
            first_state.append(state_after)
        assert t >= gate_steps or np.array_equal(reset_mask.astype(bool), g["reset_mask"][t]), t
        return obs, rew, crashes, trunc

    run_trace_against(step, g, gate_steps, tail_gate, f"oracle_vs_reference_trace[{tag}]")
    if "action_q8" not in g.files:  # one step from the identical initial state: the per-step bound
        assert max_abs(first_state[0], g["state_after_step"][0]) < 1e-5


# ---------------------------------------------------------------- LiDAR navigation task
def test_magpie_robot_model_matches_urdf():
    """MagpieCfg.robot_model (data) == composite of resources/robots/magpie/model.urdf."""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config.robot_config import MagpieCfg
    from aerial_gym_simulator_amd.robots.robot_model import composite_body

    r = load_golden("robot_magpie")
    mass, com, J = composite_body(MagpieCfg.robot_model)
    assert abs(mass - r["mass"]) < 1e-12 and np.abs(com - r["com"]).max() < 1e-12 and np.abs(J - r["inertia"]).max() < 1e-12
    assert np.array_equal(np.array(MagpieCfg.control_allocator_config.allocation_matrix), r["alloc"])


@pytest.mark.parametrize("name,cfg_name,ctrl_name", [("lmf2", "LMF2Cfg", "lmf2_controller_config"),
                                                    ("base_quad_root_link_control", "BaseQuadRootLinkControlCfg", None)])
def test_root_link_robot_configs_match_the_reference(name, cfg_name, ctrl_name):
    """lmf2 (the robot of the reference's default navigation recipe, navigation_task_config.py:9-10) and
    base_quad_root_link_control as config data: rigid-body constants == composite of the reference's URDF, allocation matrix,
    motor model, init state, disturbance and controller gain ranges == the reference's config classes (tests/golden/robot_*.npz,
    written by oracle/gen_golden_lidar_nav.py from /root/reference)."""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config import controller_config, robot_config
    from aerial_gym_simulator_amd.registry.controller_registry import controller_registry
    from aerial_gym_simulator_amd.registry.robot_registry import robot_registry
    from aerial_gym_simulator_amd.robots.robot_model import composite_body

    r = load_golden("robot_" + name)
    cfg = getattr(robot_config, cfg_name)
    mass, com, J = composite_body(cfg.robot_model)
    assert abs(mass - r["mass"]) < 1e-12 and np.abs(com - r["com"]).max() < 1e-12 and np.abs(J - r["inertia"]).max() < 1e-12
    ca, mm = cfg.control_allocator_config, cfg.control_allocator_config.motor_model_config
    assert np.array_equal(np.array(ca.allocation_matrix, np.float64), r["alloc"])
    assert ca.force_application_level == str(r["force_application_level"]) != "motor_link"
    assert abs(cfg.robot_model.collision_sphere_radius - float(r["collision_radius"])) < 1e-12
    got = [mm.motor_thrust_constant_min, mm.motor_thrust_constant_max, mm.motor_time_constant_increasing_min, mm.motor_time_constant_increasing_max,
           mm.motor_time_constant_decreasing_min, mm.motor_time_constant_decreasing_max, mm.max_thrust, mm.min_thrust, mm.max_thrust_rate,
           mm.thrust_to_torque_ratio]
    assert np.array_equal(np.array(got, np.float64), r["motor_model"])
    assert np.array_equal(np.array(cfg.init_config.min_init_state, np.float64), r["min_init_state"])
    assert np.array_equal(np.array(cfg.init_config.max_init_state, np.float64), r["max_init_state"])
    d = cfg.disturbance
    assert np.array_equal(np.array([float(d.enable_disturbance), d.prob_apply_disturbance] + list(d.max_force_and_torque_disturbance), np.float64), r["disturbance"])
    assert robot_registry.get_robot_config(name) is cfg
    if ctrl_name:
        c = getattr(controller_config, ctrl_name)
        table = np.array([c.K_pos_tensor_min, c.K_pos_tensor_max, c.K_vel_tensor_min, c.K_vel_tensor_max, c.K_rot_tensor_min, c.K_rot_tensor_max,
                          c.K_angvel_tensor_min, c.K_angvel_tensor_max], np.float64)
        assert np.array_equal(table, r["gains"]) and bool(c.randomize_params) == bool(r["randomize_params"])
        for kind in ("position", "velocity", "attitude", "rates", "acceleration"):  # control/__init__.py:91-93
            assert controller_registry.get_controller_config(f"lmf2_{kind}_control") is c


def test_magpie_root_link_substep_matches_reference(orc):
    """BaseMultirotor.step with force_application_level = "base_link": the allocator's wrench A u is
    applied to the root body (base_multirotor.py:152-159, control_allocation.py:53-79)."""
    g = load_golden("step_magpie_acceleration")
    pd = golden_params(g)
    assert pd["root_link_mode"] == 1
    P = orc.make_params(pd)
    for k in range(g["state"].shape[0]):
        st, th = g["state"][k].copy(), g["thrust_in"][k].copy()
        o = orc.substep(P, st, g["action"][k], th, g["kT"], g["tau_inc"], g["tau_dec"], g["Kp"], g["Kv"], g["KR"], g["Kw"],
                        disturb=g["disturb"][k] if g["disturb"][k].any() else None, disturb_max=g["disturb_max"], integrate=False)
        assert rel_err(o.wrench_cmd, g["wrench_cmd"][k]) < 2e-6, k
        assert rel_err(th, g["thrust_out"][k]) < 5e-6, k
        assert rel_err(o.action_clipped, g["action_after"][k]) < 1e-7, k
        bw = np.concatenate([g["force"][k][:, 0, :], g["torque"][k][:, 0, :]], axis=1)
        assert rel_err(o.body_wrench, bw) < 3e-6, k


def test_lidar_navigation_reward_matches_reference(orc):
    g = load_golden("reward_lidar_navigation")
    r = orc.reward_lidar_navigation(g["pos_err"], g["vveh"], g["wbody"], g["yaw_error"], g["crashes"], g["action"],
                                    g["prev_action"], g["time_to_collision"], float(g["curriculum_progress"]), g["rp"])
    assert rel_err(r, g["reward"]) < 2e-6
    assert (g["reward"] == -10.0).sum() == g["crashes"].sum()


def test_lidar_image_observation_matches_reference(orc):
    g = load_golden("lidar_image_obs")
    pc = g["pointcloud"][:, 0]
    ttc, ds = orc.lidar_image_obs(pc, g["robot_position"], g["robot_linvel"])
    assert rel_err(ttc, g["clean_ttc"]) < 2e-6 and rel_err(ds, g["clean_ds"]) < 2e-6
    assert ttc[0] == 10.0  # robot at rest: nothing approaches
    low = lambda a: np.concatenate([np.zeros((a.shape[0], 10, 20), np.float32), a], axis=1)  # noqa: E731  ds[:, 10:] rows
    ttc2, ds2 = orc.lidar_image_obs(pc, g["robot_position"], g["robot_linvel"], noise_mask=g["noise_mask"],
                                    noise_val=g["noise_val"], max_mask=g["max_mask"], low_mask=low(g["low_mask"]),
                                    low_val=low(g["low_val"]))
    assert rel_err(ds2, g["noisy_ds"]) < 2e-6 and np.array_equal(ttc2, ttc)
    assert (g["noisy_ds"] != g["clean_ds"]).sum() > 50


def test_lidar_navigation_obs_matches_reference(orc):
    g = load_golden("obs_lidar_navigation")
    obs = orc.obs_lidar_navigation(g["state"], g["euler"], g["qveh"], g["vbody"], g["wbody"], g["actions"], g["target"],
                                   g["target_yaw"], g["u_vec"], g["u_euler"], g["downsampled"])
    assert obs.shape == (96, 337)
    d = np.abs(obs[:, 6] - g["obs"][:, 6])
    assert np.minimum(d, 2 * np.pi - d).max() < 3e-6  # yaw error wraps at +-pi
    keep = np.r_[0:6, 7:337]
    assert rel_err(obs[:, keep], g["obs"][:, keep]) < 2e-6


@pytest.mark.parametrize("frame", ["body", "world"])
def test_imu_matches_reference(orc, frame):
    """sensors/imu_sensor.py: reset_idx + a chain of update() calls (bias random walk, noise, clamps)."""
    g = load_golden("imu_sensor")
    n = g["body_force"].shape[1]
    bias, sq = np.zeros((n, 6), np.float32), np.zeros((n, 4), np.float32)
    orc.imu_reset(np.ones(n, np.uint8), g[frame + "_u_bias"], g[frame + "_u_rot"], g["max_bias_init"], np.deg2rad(g["min_rot_deg"]),
                  np.deg2rad(g["max_rot_deg"]), bias, sq)
    assert rel_err(bias, g[frame + "_bias0"]) < 1e-6 and rel_err(sq, g[frame + "_sensor_quat"]) < 1e-6
    sqrt_dt = np.float32(np.sqrt(0.01))
    for k in range(g[frame + "_force"].shape[0]):
        meas = orc.imu_update(float(g["mass"]), [0.0, 0.0, -9.81], sqrt_dt, frame == "world", 1, 1, g["bias_std"], g["noise_std"],
                              g["max_value"], g[frame + "_force"][k], g[frame + "_quat"][k], g[frame + "_wbody"][k],
                              g[frame + "_sensor_quat"], g[frame + "_z_noise"][k], g[frame + "_z_bias"][k], bias)
        assert rel_err(meas, g[frame + "_meas"][k]) < 2e-6, k
    assert rel_err(bias, g[frame + "_bias_end"]) < 1e-6
    assert np.abs(g[frame + "_meas"][-1][:8, 0:3]).max() == 100.0  # the clamp was exercised


@pytest.mark.parametrize("frame", ["body", "world"])
def test_imu_gravity_compensation_matches_reference(orc, frame):
    """gravity_compensation = True under a tilted gravity: g_world = 0, so the reference returns the force sensor's reading over the
    mass, rotated into the sensor frame, with nothing subtracted (imu_sensor.py:61-63, 89-106).  Handing the oracle the fixture's
    gravity instead of zero is off by |gravity| = 9.3 m/s^2."""
    g = load_golden("imu_sensor_gravity_compensation")
    bias = g[frame + "_bias0"].copy()
    sqrt_dt = np.float32(np.sqrt(0.01))
    args = (g["bias_std"], g["noise_std"], g["max_value"])
    for k in range(g[frame + "_force"].shape[0]):
        rest = (g[frame + "_force"][k], g[frame + "_quat"][k], g[frame + "_wbody"][k], g[frame + "_sensor_quat"], g[frame + "_z_noise"][k],
                g[frame + "_z_bias"][k])
        wrong = orc.imu_update(float(g["mass"]), g["gravity"], sqrt_dt, frame == "world", 1, 1, *args, *rest, bias.copy())
        meas = orc.imu_update(float(g["mass"]), [0.0, 0.0, 0.0], sqrt_dt, frame == "world", 1, 1, *args, *rest, bias)
        assert rel_err(meas, g[frame + "_meas"][k]) < 2e-6, k
        d = np.linalg.norm((wrong - g[frame + "_meas"][k])[:, :3].astype(np.float64), axis=1)
        assert np.abs(d - np.linalg.norm(g["gravity"].astype(np.float64))).max() < 1e-4, k  # (no entry of this chain reaches a clamp)
    assert rel_err(bias, g[frame + "_bias_end"]) < 1e-6
    assert np.abs(g[frame + "_meas"][:, :, :3]).max() < 100.0


def _compare_fixture_dirs(made_dir, committed_dir, names=None):
    import os

    made = sorted(os.listdir(made_dir))
    for name in (made if names is None else names):
        new, old = np.load(os.path.join(made_dir, name)), np.load(os.path.join(committed_dir, name))
        assert set(new.files) == set(old.files), name
        for k in new.files:
            a, b = new[k], old[k]
            if a.dtype.kind in "US":
                assert str(a) == str(b), (name, k)
            else:
                assert a.shape == b.shape and np.array_equal(a, b), (name, k)
    return made


def test_goldens_are_reproducible_from_the_reference(tmp_path):
    """Provenance of tests/golden/: running the committed generator scripts against the reference's own code
    (/root/reference, present in the build container only) reproduces every generated fixture bit for bit."""
    import os
    import subprocess
    import sys

    from conftest import ROOT

    if not os.path.isdir("/root/reference/aerial_gym"):
        pytest.skip("the reference tree is not on this machine")
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import gen_golden as gg\n"
        "gg.OUT = %r\n"
        "gg.main()\n"
        "import gen_golden_imu as gi, gen_golden_lidar_nav as gl, gen_golden_sensors as gs, gen_golden_assets as ga\n"
        "import gen_golden_nav_glue as gn, gen_golden_policy as gp\n"
        "[m.main() for m in (gi, gl, gs, ga, gn, gp) if hasattr(m, 'main')]\n" % (os.path.join(ROOT, "oracle"), str(tmp_path))
    )
    subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, timeout=600)
    made = _compare_fixture_dirs(str(tmp_path), os.path.join(ROOT, "tests", "golden"))
    assert len(made) >= 25 and "policy_attitude_actor.npz" in made


def test_cr_goldens_are_reproducible_and_torchscript_changes_no_bit(tmp_path):
    """tests/golden/cr/ (the reference with correctly rounded elementary functions, oracle/cr_torch.py) is reproduced bit
    for bit by `gen_golden.py` in CR mode.  The generators switch TorchScript off (PYTORCH_JIT=0) so that the switchable
    patch reaches the scripted functions: with TorchScript ON (AGX_GOLDEN_JIT=1) every array of the ordinary fixtures that
    does not need the patch comes out bit-identical, so the switch changes nothing the reference computes."""
    import os
    import subprocess
    import sys

    from conftest import ROOT

    if not os.path.isdir("/root/reference/aerial_gym"):
        pytest.skip("the reference tree is not on this machine")
    code = ("import sys; sys.path.insert(0, %r)\nimport gen_golden as gg\ngg.OUT = %%r\nimport os; os.makedirs(gg.OUT, exist_ok=True)\n"
            "gg.main()\n" % os.path.join(ROOT, "oracle"))
    cr_dir, jit_dir = str(tmp_path / "cr"), str(tmp_path / "jit")
    subprocess.run([sys.executable, "-c", code % cr_dir], check=True, capture_output=True, timeout=600,
                   env=dict(os.environ, AGX_GOLDEN_CR="1"))
    made = _compare_fixture_dirs(cr_dir, os.path.join(ROOT, "tests", "golden", "cr"))
    # the folder holds those 26 and the five fixtures of gen_golden_lidar_nav.py (tests/test_lidar_navigation_task.py regenerates them)
    lidar_nav = [n + ".npz" for n in ("reward_lidar_navigation", "reward_frames_lidar_navigation", "lidar_image_obs", "obs_lidar_navigation",
                                      "step_magpie_acceleration")]
    assert len(made) == 26 and sorted(made + lidar_nav) == sorted(os.listdir(os.path.join(ROOT, "tests", "golden", "cr")))
    subprocess.run([sys.executable, "-c", code % jit_dir], check=True, capture_output=True, timeout=600,
                   env=dict(os.environ, AGX_GOLDEN_JIT="1"))
    n = 0
    for name in sorted(os.listdir(jit_dir)):
        new, old = np.load(os.path.join(jit_dir, name)), np.load(os.path.join(ROOT, "tests", "golden", name))
        assert set(old.files) - set(new.files) <= {"thrust_out_cr", "wrench_cmd_cr", "wbody_cr", "state_next_cr"}, name
        for k in new.files:
            assert str(new[k]) == str(old[k]) if new[k].dtype.kind in "US" else np.array_equal(new[k], old[k]), (name, k)
        n += 1
    assert n >= 18


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_asset_reset_matches_the_reference_asset_manager(orc, tag):
    """AssetManager.reset_idx of the reference, driven as EnvManager.reset_idx drives it (full reset of the reset
    envs + half-obstacle resample of a bernoulli subset), vs orc_reset_assets on the replayed draws: which envs
    change, parked obstacles at -1000 m, positions inside the env bounds, orientations (oracle/gen_golden_assets.py)."""
    g = load_golden("asset_reset")
    num_obstacles, num_keep = (int(x) for x in g[f"{tag}_params"])
    mask, sel = g[f"{tag}_mask"], g[f"{tag}_sel"]
    u = np.where(sel[:, None, None] > 0, g[f"{tag}_u2"], g[f"{tag}_u1"])  # the draw each env ends up with
    state = g["state_before"].copy()
    orc.reset_assets(mask, u, sel, g["min_ratio"], g["max_ratio"], g["bounds_min"], g["bounds_max"], num_obstacles, num_keep, state)
    ref = g[f"{tag}_state_after"]
    assert np.array_equal(state[mask == 0], g["state_before"][mask == 0])          # untouched envs
    assert np.array_equal(ref[mask == 0], g["state_before"][mask == 0])
    assert np.array_equal(state[..., 0:3] == -1000.0, ref[..., 0:3] == -1000.0)   # the same obstacles are parked
    assert (ref[mask > 0][..., 0] == -1000.0).any() or num_obstacles >= ref.shape[1]
    assert np.array_equal(state[..., 0:3], ref[..., 0:3])                         # positions: bit for bit
    assert np.abs(state[..., 3:7] - ref[..., 3:7]).max() < 2e-7                    # quat_from_euler: 1 ulp (libm vs torch sin/cos)
    assert np.array_equal(state[..., 7:], ref[..., 7:])                            # velocities are not touched


def test_navigation_glue_matches_the_reference_task():
    """tests/golden/navigation_glue.npz: 60 steps of the reference's REAL NavigationTask (constructor, step, reset_idx,
    curriculum) on a scripted simulator (oracle/gen_golden_nav_glue.py).  Checked here: the flag definitions the
    bookkeeping kernel implements, the host mirror's curriculum rule, and the target resampling formula."""
    import types

    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.task.navigation_task import NavigationTask

    g = load_golden("navigation_glue")
    T, n = g["position"].shape[0], g["position"].shape[1]
    cur = g["curriculum"]

    class curriculum:
        min_level, max_level, check_after_log_instances = int(cur[0]), int(cur[1]), int(cur[2])
        increase_step, decrease_step = int(cur[3]), int(cur[4])
        success_rate_for_increase, success_rate_for_decrease = float(cur[5]), float(cur[6])

    me = types.SimpleNamespace(task_config=types.SimpleNamespace(curriculum=curriculum), curriculum_level=int(g["initial_level"]),
                               obs_dict={}, success_aggregate=0, crashes_aggregate=0, timeouts_aggregate=0,
                               curriculum_progress_fraction=0.0)
    me._update_progress = types.MethodType(NavigationTask._update_progress, me)
    target = g["initial_target"].copy()
    lo, hi = g["target_min_ratio"], g["target_max_ratio"]
    levels = set()
    for t in range(T):
        assert np.array_equal(g["target_before"][t], target), t
        trunc = g["sim_steps"][t] > int(g["episode_len_steps"])
        assert np.array_equal(trunc, g["truncations"][t]), t
        d = (target - g["position"][t]).astype(np.float32)
        dist = np.sqrt((d * d).sum(axis=1, dtype=np.float32))
        crashes = g["crashes"][t].astype(bool)
        succ = trunc & (dist < 1.0) & ~crashes
        tout = trunc & ~succ & ~crashes
        edge = np.abs(dist - 1.0) < 1e-6  # torch.norm may round the last bit differently
        assert np.array_equal(succ[~edge], g["successes"][t].astype(bool)[~edge]), t
        assert np.array_equal(tout[~edge], g["timeouts"][t].astype(bool)[~edge]), t
        # curriculum: the mirror's rule on the reference's own flags
        me.success_aggregate += int(g["successes"][t].sum())
        me.crashes_aggregate += int(crashes.sum())
        me.timeouts_aggregate += int(g["timeouts"][t].sum())
        NavigationTask._curriculum_decision(me, me.success_aggregate, me.crashes_aggregate, me.timeouts_aggregate)
        assert me.curriculum_level == int(g["level"][t]), t
        assert abs(me.curriculum_progress_fraction - float(g["progress"][t])) < 1e-7, t
        assert [me.success_aggregate, me.crashes_aggregate, me.timeouts_aggregate] == g["aggregates"][t].tolist(), t
        levels.add(me.curriculum_level)
        # reset_idx: targets of the envs the simulator reset, inside their NEW bounds
        m = g["reset_mask"][t] > 0
        assert np.array_equal(m, trunc | crashes), t
        ratio = (hi - lo) * g["u_target"][t] + lo
        new = g["bounds_min"][t] + (g["bounds_max"][t] - g["bounds_min"][t]) * ratio
        target = np.where(m[:, None], new, target).astype(np.float32)
        assert np.array_equal(target, g["target_after"][t]), t
    assert len(levels) >= 4 and g["successes"].sum() > 100 and g["timeouts"].sum() > 100
