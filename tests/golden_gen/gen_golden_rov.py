"""TEST INFRASTRUCTURE -- golden vectors of the fully actuated ROV (base_rov), produced by running the REFERENCE's own BaseROV, BaseROVCfg
and resources/robots/BlueROV/rov.urdf (needs the reference tree, ref_shells.REFERENCE_ROOT; uses the helpers under oracle/ by path).

    python tests/golden_gen/gen_golden_rov.py [--cr] [--out DIR]

writes, into tests/golden/ (tests/golden/rov_cr/ with --cr: the same code with correctly rounded elementary functions,
oracle/cr_torch.py):

  step_base_rov_fully_actuated.npz        BaseROV.step recorded by oracle/gen_golden.py's gen_step, 64 envs x 2 sub-steps, with NON-ZERO
  step_edge_base_rov_fully_actuated.npz   drag coefficients, distinct per axis (DAMPING below; the config's own are all zero and
  step_base_rov_no_control.npz            exercise nothing).  Nominal source: every body velocity has three non-zero components, so
                                          the per-axis law and the multirotor's norm law differ in every row.  Edge source
                                          (ROVEdgeSource): gen_golden.EdgeSource with body velocities along one axis (rows 0-4, where
                                          the two laws coincide), at rest, and at +-100 m/s / +-100 rad/s; attitudes with every Euler
                                          angle negative, at 0 and at +-pi (what ssa() would wrap); actions at exactly +-10 and beyond
  step_base_rov_default_fully_actuated.npz  the same with the config's default all-zero coefficients
  rov_reset.npz                           BaseROV.reset_idx on four masks (none; one env of the last partial wave; all; random) of 83
                                          envs: state, derived tensors, motor thrusts, motor constants and gains before and after,
                                          the uniform draws (replayed from the same seed and checked against the generator's next
                                          output), and how many values the generator gave out
  robot_base_rov.npz                      composite mass, centre of mass, inertia, 6 x 8 wrench map of rov.urdf and the numbers of
                                          BaseROVCfg, in the keys of robot_lmf2.npz (plain run only: no elementary function in it)
"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg  # noqa: E402  FIRST: it switches TorchScript off before torch is imported (cr_torch.py)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_shells  # noqa: E402

OUT = (sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
       else os.path.join(ROOT, "tests", "golden", *(["rov_cr"] if gg.CR else [])))
CONTROLLER = "rov_fully_actuated_control"
DAMPING = dict(linvel_linear_damping_coefficient=[0.31, 0.47, 0.59], linvel_quadratic_damping_coefficient=[0.23, 0.37, 0.53],
               angular_linear_damping_coefficient=[0.011, 0.017, 0.023], angular_quadratic_damping_coefficient=[0.007, 0.013, 0.019])
N_RESET = 83
SINGLE_AXIS_ROWS = 5   # edge rows 0-4: attitudes that rotate an axis vector exactly (identity, w = -1, half turns about x, y, z)
MAX_ROWS = (40, 48)    # edge rows at the velocity limits of the asset (max_linear_velocity / max_angular_velocity = 100)
EULER_ROWS = (24, 40)  # edge rows whose attitude is built from the Euler table below


def rov_cfg():
    return ref_shells.ref("config.robot_config.base_rov_config").BaseROVCfg


def damped_cfg():
    base = rov_cfg()

    class BaseROVDampedCfg(base):
        class damping(base.damping):
            pass

    for k, v in DAMPING.items():
        setattr(BaseROVDampedCfg.damping, k, list(v))
    return BaseROVDampedCfg


def rov_links():
    return gg.parse_urdf(os.path.join(ref_shells.REFERENCE_ROOT, "resources", "robots", "BlueROV", "rov.urdf"))


def rov_constants(cfg):
    links = rov_links()
    mass, com, J = gg.composite(links)
    ca = cfg.control_allocator_config
    cq = ca.motor_model_config.thrust_to_torque_ratio
    W = np.zeros((6, ca.num_motors))
    for i in range(ca.num_motors):
        link = links["motor_%d" % i]
        ez = link["R"][:, 2]  # a thruster pushes along its link's z axis, at the link's position
        W[0:3, i] = ez
        W[3:6, i] = np.cross(link["xyz"] - com, ez) - cq * ca.motor_directions[i] * ez
    return dict(mass=np.float64(mass), com=com, inertia=J, wrench_map=W, alloc=np.array(ca.allocation_matrix, dtype=np.float64),
                collision_radius=np.float64(links["base_link"]["radius"]))


def make_ref_rov(robot_cfg, controller_name, n, consts, seed):
    """the reference's BaseROV on the CPU over a hand-made global tensor dict (what gen_golden.make_ref_robot does for BaseMultirotor)"""
    from aerial_gym.config.env_config.empty_env import EmptyEnvCfg

    mod = ref_shells.ref("robots.base_rov")
    ref_shells.ref("control")  # registers the controllers
    EmptyEnvCfg.env.num_envs = n
    torch.manual_seed(seed)
    robot = mod.BaseROV(robot_cfg, controller_name, EmptyEnvCfg, "cpu")
    bodies = 1 + 2 * robot_cfg.control_allocator_config.num_motors
    state = torch.zeros(n, 13)
    state[:, 6] = 1.0
    gtd = {
        "dt": 0.01, "gravity": torch.tensor([0.0, 0.0, -9.81]).expand(n, -1),
        "robot_state_tensor": state, "robot_position": state[:, 0:3], "robot_orientation": state[:, 3:7],
        "robot_linvel": state[:, 7:10], "robot_angvel": state[:, 10:13],
        "robot_force_tensor": torch.zeros(n, bodies, 3), "robot_torque_tensor": torch.zeros(n, bodies, 3),
        "env_bounds_min": -torch.ones(n, 3), "env_bounds_max": torch.ones(n, 3),
        "robot_mass": torch.full((n,), float(np.float32(consts["mass"]))),
        "robot_inertia": torch.tensor(consts["inertia"], dtype=torch.float32).expand(n, 3, 3).contiguous(),
    }
    robot.init_tensors(gtd)
    return robot, gtd


class ROVNominalSource(gg.NominalSource):
    def check(self, c, out):
        assert (out["vbody"] != 0).sum(axis=2).min() >= 2  # the per-axis and the norm law differ in every row


def euler_table():
    """attitudes ssa() would change or that sit on its seams: each angle negative, at 0 and at +-pi next to two ordinary ones, all
    three negative, all three at 0 / pi"""
    pi = math.pi
    rows = []
    for axis in range(3):
        for value in (0.0, pi, -pi, -0.7):
            e = [-0.3, 0.4, -2.0]
            e[axis] = value
            rows.append(e)
    rows += [[-0.5, -0.4, -2.5], [pi, pi, pi], [-pi, -pi, -pi], [-3.0, -1.2, -0.1]]
    assert len(rows) == EULER_ROWS[1] - EULER_ROWS[0]
    return torch.tensor(rows, dtype=torch.float32)


class ROVEdgeSource(gg.EdgeSource):
    def initial(self, c):
        m = ref_shells.ref("utils.math")
        s, th = super().initial(c)
        lo, hi = EULER_ROWS
        s[lo:hi, 3:7] = m.quat_from_euler_xyz_tensor(euler_table())
        # rows 0-4 (identity, w = -1, half turns about x, y, z: an axis vector stays one, exactly): velocities along ONE body axis
        for row in range(SINGLE_AXIS_ROWS):
            s[row, 7:13] = 0.0
            s[row, 7 + row % 3] = (-1.0) ** row * (0.7 + 0.6 * row)
            s[row, 10 + (row + 1) % 3] = (-1.0) ** (row + 1) * (0.4 + 0.3 * row)
        a, b = MAX_ROWS
        for row in range(a, b):
            sign = 1.0 if row % 2 == 0 else -1.0
            d = torch.nn.functional.normalize(torch.randn(3, generator=c.rng), dim=0)
            if row < a + 4:
                d = torch.eye(3)[row % 3]
            s[row, 7:10] = sign * 100.0 * d
            s[row, 10:13] = -sign * 100.0 * d.roll(1)
        return s, th

    def action(self, c, k):
        a = super().action(c, k)
        a[3, 0:3] = torch.tensor([10.0, -10.0, 10.0])    # exactly at the clip
        a[4, 0:7] = torch.tensor([-10.0, 10.0, -10.0, 10.0, -10.0, 10.0, -10.0])
        a[5, 0:3] = torch.tensor([10.5, -300.0, 1e6])    # beyond it
        return a

    def check(self, c, out):
        super().check(c, out)
        vb, e = out["vbody"][0], out["euler"][0]
        assert ((vb[:SINGLE_AXIS_ROWS] != 0).sum(axis=1) == 1).all(), vb[:SINGLE_AXIS_ROWS]
        assert ((out["wbody"][0][:SINGLE_AXIS_ROWS] != 0).sum(axis=1) == 1).all()
        assert ((vb == 0).all(axis=1)).sum() >= 8                                        # at rest
        assert (np.abs(np.linalg.norm(out["state"][0][MAX_ROWS[0]:MAX_ROWS[1], 7:10], axis=1) - 100.0) < 1e-3).all()
        assert (e >= 0).all() and (e < np.float32(2 * math.pi) + 1e-6).all() and (e > math.pi).sum() > 30  # not wrapped to (-pi, pi]
        assert (np.abs(out["action"]) == 10.0).sum() >= 10 and (np.abs(out["action"]) > 10.0).sum() > 50


def gen_steps():
    cfg, damped = rov_cfg(), damped_cfg()
    consts = rov_constants(cfg)
    assert all(v == [0.0, 0.0, 0.0] for k, v in vars(cfg.damping).items() if k.endswith("coefficient"))
    gg.OUT = OUT  # (gen_step writes next to the other fixtures of this generator)
    gg.make_ref_robot = make_ref_rov  # gen_step builds its robot through this name: the reference's BaseROV instead of BaseMultirotor
    gg.gen_step("base_rov", damped, CONTROLLER, "fully_actuated", consts, n=64, K=2, seed=7, source=ROVNominalSource())
    gg.gen_step("base_rov", damped, CONTROLLER, "fully_actuated", consts, n=64, K=2, seed=11, source=ROVEdgeSource())
    gg.gen_step("base_rov", damped, "no_control", "no_control", consts, n=64, K=2, seed=13, source=ROVNominalSource())
    gg.gen_step("base_rov_default", cfg, CONTROLLER, "fully_actuated", consts, n=64, K=2, seed=17, source=ROVNominalSource())


def snapshot(robot, gtd):
    mm = robot.control_allocator.motor_model
    c = robot.controller
    return dict(state=gtd["robot_state_tensor"], euler=robot.robot_euler_angles, qveh=robot.robot_vehicle_orientation,
                vveh=robot.robot_vehicle_linvel, vbody=robot.robot_body_linvel, wbody=robot.robot_body_angvel,
                thrust=mm.current_motor_thrust, tau_inc=mm.motor_time_constants_increasing, tau_dec=mm.motor_time_constants_decreasing,
                gains=torch.cat([c.K_pos_tensor_current, c.K_linvel_tensor_current, c.K_rot_tensor_current, c.K_angvel_tensor_current], dim=1))


def gen_reset():
    n = N_RESET
    cfg = rov_cfg()
    consts = rov_constants(cfg)
    rng = torch.Generator().manual_seed(4242)
    random_mask = torch.rand(n, generator=rng) < 0.3
    masks = [torch.zeros(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool), torch.ones(n, dtype=torch.bool), random_mask]
    masks[1][70] = True  # one env of the last, partial wave (envs 64-82)
    assert random_mask.any() and not random_mask.all()
    rec = {}
    for case, mask in enumerate(masks):
        robot, gtd = make_ref_rov(cfg, CONTROLLER, n, consts, seed=100 + case)
        gtd["robot_state_tensor"][:] = gg.random_state(n, rng)
        robot.update_states()
        robot.control_allocator.motor_model.current_motor_thrust[:] = (torch.rand(n, 8, generator=rng) - 0.5) * 12.0
        ids = torch.nonzero(mask).squeeze(-1)
        before = {k: v.clone() for k, v in snapshot(robot, gtd).items()}
        sd = 900 + case
        torch.manual_seed(sd)
        robot.reset_idx(ids)
        probe = torch.rand(5)
        after = {k: v.clone() for k, v in snapshot(robot, gtd).items()}
        # the draws again, by the calls reset_idx makes (base_rov.py:176, base_lee_controller.py:107-118): one [N, 13] uniform for
        # the state, then four [len(env_ids), 3] for the gains -- nothing for the motors; none at all for an empty set
        torch.manual_seed(sd)
        shapes = [] if len(ids) == 0 else [[n, 13]] + [[len(ids), 3]] * 4
        draws = [torch.rand(*s) for s in shapes]
        assert torch.equal(torch.rand(5), probe), "the generator is not where the replayed calls leave it"
        u_state = draws[0] if draws else torch.zeros(n, 13)
        u_gains = torch.zeros(n, 12)
        for k in range(4):
            if draws:
                u_gains[ids, 3 * k:3 * k + 3] = draws[1 + k]
        for k in ("thrust", "tau_inc", "tau_dec"):
            assert torch.equal(before[k], after[k]), k  # base_rov.py:171-198 never touches the motor model
        untouched = ~mask
        assert torch.equal(before["state"][untouched], after["state"][untouched]) and torch.equal(before["gains"][untouched], after["gains"][untouched])
        if len(ids):
            assert not torch.equal(before["state"][mask], after["state"][mask])
        else:
            assert all(torch.equal(before[k], after[k]) for k in before)
        for k, v in before.items():
            rec.setdefault(k + "_before", []).append(v.numpy())
        for k, v in after.items():
            rec.setdefault(k + "_after", []).append(v.numpy())
        rec.setdefault("mask", []).append(mask.numpy())
        rec.setdefault("u_state", []).append(u_state.numpy())
        rec.setdefault("u_gains", []).append(u_gains.numpy())
        rec.setdefault("consumed", []).append(np.int64(sum(a * b for a, b in shapes)))
        rec.setdefault("draw_shapes", []).append(json.dumps(shapes))
    out = {k: np.stack(v) for k, v in rec.items() if k != "draw_shapes"}
    c = robot.controller
    out.update(draw_shapes=np.array(rec["draw_shapes"]), min_init_state=np.array(cfg.init_config.min_init_state, np.float64),
               max_init_state=np.array(cfg.init_config.max_init_state, np.float64),
               gains_min=torch.cat([c.K_pos_tensor_min[0], c.K_linvel_tensor_min[0], c.K_rot_tensor_min[0], c.K_angvel_tensor_min[0]]).numpy(),
               gains_max=torch.cat([c.K_pos_tensor_max[0], c.K_linvel_tensor_max[0], c.K_rot_tensor_max[0], c.K_angvel_tensor_max[0]]).numpy(),
               bounds_min=-np.ones(3, np.float32), bounds_max=np.ones(3, np.float32))
    np.savez(os.path.join(OUT, "rov_reset.npz"), **out)
    print("rov_reset: masks", [int(m.sum()) for m in masks], "values consumed", out["consumed"].tolist())


def gen_robot():
    cfg = rov_cfg()
    links = rov_links()
    consts = rov_constants(cfg)
    ca = cfg.control_allocator_config
    mm = ca.motor_model_config
    motors = ["motor_%d" % i for i in range(ca.num_motors)]
    arms = ["arm_motor_%d" % i for i in range(ca.num_motors)]
    assert set(links) == {"base_link"} | set(motors) | set(arms)
    import xml.etree.ElementTree as ET

    urdf = ET.parse(os.path.join(ref_shells.REFERENCE_ROOT, "resources", "robots", "BlueROV", "rov.urdf")).getroot()
    assert {j.find("parent").get("link") for j in urdf.findall("joint")} == {"base_link"}  # parse_urdf places links by their own joint
    out = dict(mass=consts["mass"], com=consts["com"], inertia=consts["inertia"], wrench_map=consts["wrench_map"], alloc=consts["alloc"],
               base_mass=np.float64(links["base_link"]["mass"]), base_inertia=links["base_link"]["inertia"],
               motor_mass=np.float64(links[motors[0]]["mass"]), motor_inertia=links[motors[0]]["inertia"],
               motor_masses=np.array([links[p]["mass"] for p in motors]),
               motor_pos=np.array([links[p]["xyz"] for p in motors]), motor_rpy=np.array([links[p]["rpy"] for p in motors], np.float64),
               arm_mass=np.float64(links[arms[0]]["mass"]), arm_masses=np.array([links[p]["mass"] for p in arms]),
               arm_inertia=links[arms[0]]["inertia"],
               arm_pos=np.array([links[p]["xyz"] for p in arms]), arm_rpy=np.array([links[p]["rpy"] for p in arms], np.float64),
               collision_radius=consts["collision_radius"], force_application_level=np.array(ca.force_application_level),
               application_mask=np.array(ca.application_mask), motor_directions=np.array(ca.motor_directions),
               motor_model=np.array([mm.motor_thrust_constant_min, mm.motor_thrust_constant_max, mm.motor_time_constant_increasing_min,
                                     mm.motor_time_constant_increasing_max, mm.motor_time_constant_decreasing_min,
                                     mm.motor_time_constant_decreasing_max, mm.max_thrust, mm.min_thrust, mm.max_thrust_rate,
                                     mm.thrust_to_torque_ratio], np.float64),
               motor_model_flags=np.array(json.dumps(dict(use_rps=mm.use_rps, use_discrete_approximation=mm.use_discrete_approximation,
                                                          integration_scheme=getattr(mm, "integration_scheme", None)))),
               min_init_state=np.array(cfg.init_config.min_init_state, np.float64), max_init_state=np.array(cfg.init_config.max_init_state, np.float64),
               disturbance=np.array([float(cfg.disturbance.enable_disturbance), cfg.disturbance.prob_apply_disturbance]
                                    + list(cfg.disturbance.max_force_and_torque_disturbance), np.float64),
               drag_coefficients=np.array([cfg.damping.linvel_linear_damping_coefficient, cfg.damping.linvel_quadratic_damping_coefficient,
                                           cfg.damping.angular_linear_damping_coefficient, cfg.damping.angular_quadratic_damping_coefficient], np.float64),
               sensors=np.array([cfg.sensor_config.enable_camera, cfg.sensor_config.enable_lidar, cfg.sensor_config.enable_imu]),
               damping=np.array([cfg.robot_asset.linear_damping, cfg.robot_asset.angular_damping], np.float64),
               asset=np.array(json.dumps(dict(file=cfg.robot_asset.file, name=cfg.robot_asset.name))))
    np.savez(os.path.join(OUT, "robot_base_rov.npz"), **out)
    print("robot_base_rov: mass %.9g  com %s\n%s" % (out["mass"], out["com"], out["inertia"]))


def main():
    os.makedirs(OUT, exist_ok=True)
    ref_shells.install()
    gen_steps()
    gen_reset()
    if not gg.CR:
        gen_robot()


if __name__ == "__main__":
    main()
