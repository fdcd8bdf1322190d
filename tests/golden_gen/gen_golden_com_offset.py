"""TEST INFRASTRUCTURE -- golden vectors of the two BaseMultirotor airframes base_random and lmf1, produced by running the REFERENCE's own
BaseMultirotor with BaseRandCfg / LMF1Cfg and their URDFs (needs the reference tree, ref_shells.REFERENCE_ROOT; uses the helpers under
oracle/ by path).

    python tests/golden_gen/gen_golden_com_offset.py [--cr] [--out DIR]

writes, into tests/golden/ (tests/golden/com_cr/ with --cr: the same code with correctly rounded elementary functions,
oracle/cr_torch.py):

  step_base_random_{position,attitude,no_control}.npz   BaseMultirotor.step recorded by oracle/gen_golden.py's gen_step, 64 envs x 2
  step_edge_base_random_{position,attitude}.npz         sub-steps, under lee_position_control, lee_attitude_control and no_control,
                                                        with NON-ZERO drag coefficients (DAMPING below; the config's own are zero)
                                                        and the config's own disturbance, whose draws are replayed and recorded: the
                                                        root body's entry of robot_force_tensor is non-zero in every row with a
                                                        disturbance and in every moving row.  Nominal source and gen_golden's edge
                                                        table.  The state of sub-step 1 is sub-step 0's advanced about the centre of
                                                        mass, which random.urdf puts 22.6 mm from the base-link origin: the oracle's
                                                        integrator (PhysX is a closed binary) on the motor links' sum plus the root
                                                        entry with its lever arm, and the base-link position behind it
                                                        (tests/com_offset_ref.py; DESIGN.md "integrator")
  robot_base_random.npz, robot_lmf1.npz                 composite mass, centre of mass, inertia, the 6 x M wrench map about the centre
                                                        of mass and about the base-link origin, and the numbers of the config, in the
                                                        keys of robot_lmf2.npz (plain run only: no elementary function in it)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_golden as gg  # noqa: E402  FIRST: it switches TorchScript off before torch is imported (cr_torch.py)

import numpy as np  # noqa: E402

import oracle as orc  # noqa: E402
import ref_shells  # noqa: E402
from com_offset_ref import correct_position, lever_torque  # noqa: E402

OUT = (sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
       else os.path.join(ROOT, "tests", "golden", *(["com_cr"] if gg.CR else [])))
DAMPING = dict(linvel_linear_damping_coefficient=[0.031, 0.047, 0.059], linvel_quadratic_damping_coefficient=[0.023, 0.037, 0.053],
               angular_linear_damping_coefficient=[0.0011, 0.0017, 0.0023], angular_quadratic_damping_coefficient=[0.0007, 0.0013, 0.0019])
LMF1_MOTOR_LINKS = ("front_right_prop", "back_left_prop", "front_left_prop", "back_right_prop")  # bodies 4, 1, 3, 2: LMF1Cfg.application_mask


def rand_cfg():
    return ref_shells.ref("config.robot_config.base_random_config").BaseRandCfg


def lmf1_cfg():
    return ref_shells.ref("config.robot_config.lmf1_config").LMF1Cfg


def damped_cfg():
    base = rand_cfg()

    class BaseRandDampedCfg(base):
        class damping(base.damping):
            pass

    for k, v in DAMPING.items():
        setattr(BaseRandDampedCfg.damping, k, list(v))
    return BaseRandDampedCfg


def wrench_maps(links, motors, cfg, com):
    """6 x M wrench per unit thrust of motor j (along its link's z axis, reaction torque -cq dir_j about it) about `com` and about
    the base-link origin"""
    ca = cfg.control_allocator_config
    cq = ca.motor_model_config.thrust_to_torque_ratio
    W, W0 = np.zeros((6, ca.num_motors)), np.zeros((6, ca.num_motors))
    for i, name in enumerate(motors):
        ez = links[name]["R"][:, 2]
        W[0:3, i] = W0[0:3, i] = ez
        W[3:6, i] = np.cross(links[name]["xyz"] - com, ez) - cq * ca.motor_directions[i] * ez
        W0[3:6, i] = np.cross(links[name]["xyz"], ez) - cq * ca.motor_directions[i] * ez
    return W, W0


def advance_state_com(gtd, mask, consts, P):
    """gen_golden.advance_state about a centre of mass off the base-link origin: the root body's force acts at the origin"""
    c = consts["com"].astype(np.float32)
    u = gtd["robot_force_tensor"][:, mask, 2].numpy().astype(np.float32)
    bw = gg.link_wrench(u, consts["wrench_map"].astype(np.float32))
    f_root = gtd["robot_force_tensor"][:, 0, :].numpy().astype(np.float32)
    bw[:, 0:3] += f_root
    bw[:, 3:6] += gtd["robot_torque_tensor"][:, 0, :].numpy()
    bw[:, 3:6] = bw[:, 3:6] + lever_torque(f_root, c)
    st = np.ascontiguousarray(gtd["robot_state_tensor"].numpy().astype(np.float32))
    q0 = st[:, 3:7].copy()
    orc.integrate(P, st, np.ascontiguousarray(bw))
    st[:, 0:3] = correct_position(st[:, 0:3], q0, st[:, 3:7], c)
    return st


def gen_steps():
    damped = damped_cfg()
    consts = gg.robot_constants("random", rand_cfg())
    assert np.abs(consts["com"]).max() > 0.02 and rand_cfg().disturbance.enable_disturbance
    params_dict = gg.params_dict

    def params_with_com(*a, **k):
        pd = params_dict(*a, **k)
        pd["com"] = [float(x) for x in consts["com"].astype(np.float32)]
        return pd

    gg.OUT = OUT                       # (gen_step writes next to the other fixtures of this generator)
    gg.params_dict = params_with_com   # params_json carries the offset
    gg.advance_state = advance_state_com
    try:
        gg.gen_step("base_random", damped, "lee_position_control", "position", consts, n=64, K=2, seed=7, source=gg.NominalSource())
        gg.gen_step("base_random", damped, "lee_attitude_control", "attitude", consts, n=64, K=2, seed=9, source=gg.NominalSource())
        gg.gen_step("base_random", damped, "no_control", "no_control", consts, n=64, K=2, seed=13, source=gg.NominalSource())
        gg.gen_step("base_random", damped, "lee_position_control", "position", consts, n=64, K=2, seed=11, source=gg.EdgeSource())
        gg.gen_step("base_random", damped, "lee_attitude_control", "attitude", consts, n=64, K=2, seed=15, source=gg.EdgeSource())
    finally:
        gg.params_dict = params_dict
    for name in ("step_base_random_position", "step_edge_base_random_position"):
        g = np.load(os.path.join(OUT, name + ".npz"))
        root = np.abs(g["force"][:, :, 0, :]).max(axis=2)
        print(name, "rows with a root-body force:", int((root > 0).sum()), "of", root.size, " with a disturbance:", int(g["disturb"][:, :, 0].sum()))
        assert (root > 0).sum() > root.size // 2


def gen_robot(tag, cfg, urdf, motors):
    links = gg.parse_urdf(os.path.join(ref_shells.REFERENCE_ROOT, "resources", "robots", *urdf))
    mass, com, J = gg.composite(links)
    W, W0 = wrench_maps(links, motors, cfg, com)
    ca = cfg.control_allocator_config
    mm = ca.motor_model_config
    assert all(links[m]["mass"] == links[motors[0]]["mass"] for m in motors)
    assert all(l["mass"] == 0.0 for name, l in links.items() if name != "base_link" and name not in motors)  # massless arm links
    radius = links["base_link"]["radius"]
    out = dict(mass=np.float64(mass), com=com, inertia=J, wrench_map=W, wrench_map_origin=W0, alloc=np.array(ca.allocation_matrix, np.float64),
               base_mass=np.float64(links["base_link"]["mass"]), base_inertia=links["base_link"]["inertia"],
               motor_mass=np.float64(links[motors[0]]["mass"]), motor_inertia=links[motors[0]]["inertia"],
               motor_pos=np.array([links[m]["xyz"] for m in motors]), motor_rpy=np.array([links[m]["rpy"] for m in motors], np.float64),
               collision_radius=np.float64(radius if radius is not None else np.nan),
               force_application_level=np.array(ca.force_application_level), application_mask=np.array(ca.application_mask),
               motor_directions=np.array(ca.motor_directions),
               motor_model=np.array([mm.motor_thrust_constant_min, mm.motor_thrust_constant_max, mm.motor_time_constant_increasing_min,
                                     mm.motor_time_constant_increasing_max, mm.motor_time_constant_decreasing_min,
                                     mm.motor_time_constant_decreasing_max, mm.max_thrust, mm.min_thrust, mm.max_thrust_rate,
                                     mm.thrust_to_torque_ratio], np.float64),
               motor_model_flags=np.array(json.dumps(dict(use_rps=mm.use_rps, use_discrete_approximation=mm.use_discrete_approximation,
                                                          integration_scheme=getattr(mm, "integration_scheme", None)))),
               min_init_state=np.array(cfg.init_config.min_init_state, np.float64), max_init_state=np.array(cfg.init_config.max_init_state, np.float64),
               min_state_ratio=np.array(cfg.robot_asset.min_state_ratio, np.float64), max_state_ratio=np.array(cfg.robot_asset.max_state_ratio, np.float64),
               disturbance=np.array([float(cfg.disturbance.enable_disturbance), cfg.disturbance.prob_apply_disturbance]
                                    + list(cfg.disturbance.max_force_and_torque_disturbance), np.float64),
               drag_coefficients=np.array([cfg.damping.linvel_linear_damping_coefficient, cfg.damping.linvel_quadratic_damping_coefficient,
                                           cfg.damping.angular_linear_damping_coefficient, cfg.damping.angular_quadratic_damping_coefficient], np.float64),
               sensors=np.array([cfg.sensor_config.enable_camera, cfg.sensor_config.enable_lidar, cfg.sensor_config.enable_imu]),
               damping=np.array([cfg.robot_asset.linear_damping, cfg.robot_asset.angular_damping], np.float64),
               asset=np.array(json.dumps(dict(file=cfg.robot_asset.file, name=cfg.robot_asset.name, collision_mask=cfg.robot_asset.collision_mask,
                                              collapse_fixed_joints=cfg.robot_asset.collapse_fixed_joints, armature=cfg.robot_asset.armature))))
    np.savez(os.path.join(OUT, "robot_%s.npz" % tag), **out)
    print("robot_%s: mass %.9g  com %s  max |alloc - wrench map about the origin| %.3e\n%s"
          % (tag, out["mass"], out["com"], np.abs(out["alloc"] - W0).max(), out["inertia"]))


def main():
    os.makedirs(OUT, exist_ok=True)
    ref_shells.install()
    gen_steps()
    if not gg.CR:
        gen_robot("base_random", rand_cfg(), ("random", "random.urdf"), ["motor_%d" % i for i in range(8)])
        gen_robot("lmf1", lmf1_cfg(), ("lmf1", "model.urdf"), list(LMF1_MOTOR_LINKS))


if __name__ == "__main__":
    main()
