"""GPU: BASELINE config 3 end to end at small N -- navigation task (10 sub-steps, 100 boxes + 6 walls,
64x48 depth + segmentation camera) through the Task API in the sync-free mode, checked step by step
against the CPU oracle (teacher-forced on the product's pre-step buffers, so every comparison is a
one-step prediction): dynamics, collision flags, reward, truncation, reset set, obstacle reset (device
Philox stream), scene transform, ray-cast image + segmentation, post-processing, observation."""
import numpy as np
import pytest
import torch
from conftest import max_abs, max_rel, rel_err
from task_test_util import npy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class RecordingSource:
    """TorchRandomSource that remembers every draw (by tag) so the oracle can replay it."""

    def __init__(self, device, seed):
        self.device = torch.device(device)
        self.gen = torch.Generator(device=device).manual_seed(seed)
        self.log = {}

    def _rec(self, tag, t):
        self.log.setdefault(tag, []).append(t.detach().clone())
        return t

    def rand(self, *shape, tag=""):
        return self._rec(tag, torch.rand(*shape, device=self.device, generator=self.gen))

    def rand_into(self, out, tag=""):
        out.uniform_(0.0, 1.0, generator=self.gen)
        self._rec(tag, out)
        return out

    def bernoulli(self, p, *shape, tag=""):
        return self._rec(tag, torch.bernoulli(torch.full(shape, float(p), device=self.device), generator=self.gen))

    def normal_into(self, out, tag=""):
        out.normal_(0.0, 1.0, generator=self.gen)
        self._rec(tag, out)
        return out

    def gauss(self, mean, std):
        return mean

    def last(self, tag):
        return self.log[tag][-1].cpu().numpy()


NAV_CASES = {
    # BASELINE configs[2]: quadrotor, Lee velocity control, 64 x 48 depth + segmentation camera
    "config3_camera": ("navigation_task", "navigation_task_config", 12, 45),
    # BASELINE configs[3] as written: fully-actuated octarotor (7-D command, disturbances on), 32 x 512 range + seg LiDAR
    "config4_fully_actuated_lidar": ("navigation_task_fully_actuated_lidar", "fully_actuated_lidar_navigation_task_config", 6, 30),
}


@pytest.mark.parametrize("case", list(NAV_CASES))
def test_navigation_task_step_by_step_vs_oracle(orc, parity, case):
    task_name, cfg_name, n, T = NAV_CASES[case]
    run_nav_case(orc, parity, case, task_name, cfg_name, n, T)


def run_nav_case(orc, parity, case, task_name, cfg_name, n, T, episode_len=12, all_obstacles=False, use_bvh=False, min_resets=None):
    """`use_bvh`: the oracle's ray-cast goes through its own median-split BVH (bit-identical to its brute force,
    tests/test_oracle_raycast.py) -- what makes the full-size cases of tests/test_gpu_full_size_parity.py affordable.
    `all_obstacles`: every obstacle of the scene is in the env (BASELINE configs 2/3: 100 boxes + 6 walls; bench.py's setting)
    instead of the task's curriculum start."""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config import task_config as tc
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    cfg = getattr(tc, cfg_name)
    seed = 0xC0FFEE1234
    rs = RecordingSource(DEV, 77)
    old_cfg = (cfg.episode_len_steps, cfg.args, cfg.device)
    old_cur = (cfg.curriculum.min_level, cfg.curriculum.max_level)
    if all_obstacles:
        cfg.curriculum.min_level, cfg.curriculum.max_level = 106, 107
    cfg.device, cfg.episode_len_steps = DEV, episode_len
    if case.startswith("config3_camera"):
        cfg.robot_name, cfg.controller_name = "base_quadrotor_with_camera_64x48", "lee_velocity_control"
    cfg.args = {"strict_rng": False, "random_source": rs, "rng_seed": seed}
    try:
        task = task_registry.make_task(task_name, seed=3, num_envs=n, headless=True)
        env = task.sim_env
        g, sc = env.global_tensor_dict, env.scene
        sensor = env.robot_manager.warp_sensor
        K, nk = sc.num_assets, env.keep_in_env
        P = orc.make_params(env.robot_manager.robot.params_dict)
        pd = env.robot_manager.robot.params_dict
        ctrl = env.robot_manager.robot.controller
        gains = [np.tile(((np.array(ctrl.gains_max, np.float32) + np.array(ctrl.gains_min, np.float32)) / np.float32(2))[3 * k:3 * k + 3], (n, 1))
                 for k in range(4)]
        mm = env.robot_manager.robot.control_allocator.motor_model
        tri_local, tri_asset, tri_seg, half = npy(sc.tri_local), npy(sc.tri_asset), npy(sc.tri_seg), npy(sc.half_extents)
        lo_r, hi_r = npy(g["asset_min_state_ratio"]), npy(g["asset_max_state_ratio"])
        e = env.cfg.env
        bcfg = [np.array(x, np.float32) for x in (e.lower_bound_min, e.lower_bound_max, e.upper_bound_min, e.upper_bound_max)]
        scfg = sensor.cfg
        if sensor.is_lidar:
            rays = orc.lidar_ray_table(scfg.height, scfg.width, scfg.horizontal_fov_deg_min, scfg.horizontal_fov_deg_max,
                                       scfg.vertical_fov_deg_min, scfg.vertical_fov_deg_max)
            # torch's float64 cos / sin (product) and libm's (this table) may differ in the last bit of a few entries: the
            # table itself is pinned to the reference's WarpLidar on the CPU (golden sensor_frontend); trace with the product's
            assert np.abs(rays - npy(sensor.ray_vectors)).max() < 1.2e-7
            rays = npy(sensor.ray_vectors)
        else:
            kinv, cx, cy = orc.camera_kinv(scfg.width, scfg.height, scfg.horizontal_fov_deg)
        frame = orc.quat_from_euler(np.deg2rad(np.array([scfg.euler_frame_rot_deg], np.float32)))[0]
        rp = np.array([cfg.reward_parameters[k] for k in cfg.REWARD_PARAMETER_ORDER], np.float32)
        robot = env.robot_manager.robot
        dcfg = robot.cfg.disturbance
        dmax = np.array(dcfg.max_force_and_torque_disturbance, np.float32)
        A = env.num_robot_actions
        assert A == (7 if "fully_actuated" in case else 4)

        def snapshot():
            per_env = getattr(ctrl, "_per_env_gains_bound", False)  # randomize_params: gains are re-drawn at every reset
            return dict(gains=[npy(x) for x in (ctrl.K_pos_tensor_current, ctrl.K_linvel_tensor_current, ctrl.K_rot_tensor_current,
                                                ctrl.K_angvel_tensor_current)] if per_env else gains,
                        state=npy(g["robot_state_tensor"]), thrust=npy(mm.current_motor_thrust), kT=npy(mm.motor_thrust_constant),
                        tau_inc=npy(mm.motor_time_constants_increasing), tau_dec=npy(mm.motor_time_constants_decreasing),
                        asset=npy(sc.asset_state), target=npy(task.target_position), pos_err=npy(task.pos_error_vehicle_frame),
                        actions=npy(g["robot_actions"]), steps=npy(g["sim_steps"]), ep=npy(g["episode_count"]),
                        bmin=npy(g["env_bounds_min"]), bmax=npy(g["env_bounds_max"]), tri_world=npy(sc.tri_world),
                        euler=npy(g["robot_euler_angles"]), qveh=npy(g["robot_vehicle_orientation"]),
                        vbody=npy(g["robot_body_linvel"]), wbody=npy(g["robot_body_angvel"]))

        def boxes_of(asset):
            return np.ascontiguousarray(np.concatenate([asset[..., :7], half], axis=-1))

        task.reset()
        torch.cuda.synchronize()
        agen = torch.Generator(device=DEV).manual_seed(5)
        n_resets = n_crashes = 0
        for t in range(T):
            pre = snapshot()
            action = torch.rand(n, 4, device=DEV, generator=agen) * 2 - 1
            obs, rew, term, trunc, info = task.step(action)
            torch.cuda.synchronize()
            post = snapshot()
            # ---------------- oracle: one env step from the product's pre-step buffers
            a_tr = npy(task._transform_action(action))  # what the task hands its controller (the built-in function as one launch)
            st, th = pre["state"].copy(), pre["thrust"].copy()
            crashes = np.zeros(n, np.uint8)
            boxes = boxes_of(pre["asset"])
            assert a_tr.shape == (n, A)
            step_no = env.step_counter - 1  # counter word of this env step's device RNG streams
            for sub in range(10):
                dist = None
                if dcfg.enable_disturbance:  # apply_disturbance drawn in the kernel: stream RNG_DISTURB + sub-step
                    dist = orc.rng_fill(seed, np.full(n, step_no, np.int32), (1 << 20) + sub, 7)
                    dist[:, 0] = (dist[:, 0] < np.float32(dcfg.prob_apply_disturbance)).astype(np.float32)
                o = orc.substep(P, st, a_tr.copy(), th, pre["kT"], pre["tau_inc"], pre["tau_dec"], *pre["gains"], disturb=dist, disturb_max=dmax)
                orc.collide_sphere_boxes(pd["collision_radius"], st, boxes, crashes)
            pe, ppe = pre["pos_err"].copy(), np.zeros((n, 3), np.float32)
            r_ref = orc.reward_navigation(st, o.qveh, pre["target"], a_tr, a_tr, task.curriculum_progress_fraction, rp, pe, ppe, crashes)
            trunc_ref = (pre["steps"] + 1) > cfg.episode_len_steps
            reset_ref = (crashes > 0) | trunc_ref
            assert np.array_equal(npy(term), crashes.astype(bool)), t                     # crash flags: bit-exact
            assert np.array_equal(npy(trunc), trunc_ref), t
            assert np.array_equal(npy(g["reset_mask"]).astype(bool), reset_ref), t
            parity.check(f"nav_task_reward[{case}]", max_abs(npy(rew), r_ref), 0.0, "abs (bit-exact)", t)
            keep = ~reset_ref
            if keep.any():  # 10 fused sub-steps (+ in-kernel disturbance draws): bit-exact
                parity.check(f"nav_task_state_10_substeps[{case}]", max_abs(post["state"][keep], st[keep]), 0.0, "abs (bit-exact)", t)
                parity.check(f"nav_task_thrust_10_substeps[{case}]", max_abs(post["thrust"][keep], th[keep]), 0.0, "abs (bit-exact)", t)
            n_resets += int(reset_ref.sum())
            n_crashes += int(crashes.sum())
            # ---------------- reset of the flagged envs (device Philox streams)
            asset_ref, bmin_ref, bmax_ref = pre["asset"].copy(), pre["bmin"].copy(), pre["bmax"].copy()
            if reset_ref.any():
                ub = orc.rng_fill(seed, pre["ep"], orc.RNG_BOUNDS, 6)
                nb_min = (bcfg[1] - bcfg[0]) * ub[:, :3] + bcfg[0]
                nb_max = (bcfg[3] - bcfg[2]) * ub[:, 3:] + bcfg[2]
                bmin_ref[reset_ref], bmax_ref[reset_ref] = nb_min[reset_ref], nb_max[reset_ref]
                sel = orc.rng_fill(seed, pre["ep"], orc.RNG_ASSET_SEL, 1)[:, 0] < 0.15
                u = np.stack([orc.rng_fill(seed, pre["ep"], orc.RNG_ASSETS + a, 6) for a in range(K)], axis=1)
                u = np.concatenate([u, np.zeros((n, K, 7), np.float32)], axis=2)
                orc.reset_assets(reset_ref.astype(np.uint8), u, sel.astype(np.uint8), lo_r, hi_r, nb_min.astype(np.float32),
                                 nb_max.astype(np.float32), int(g["num_obstacles_in_env"]), nk, asset_ref)
                us = orc.rng_fill(seed, pre["ep"], orc.RNG_STATE, 13)
                st_reset = post["state"].copy()
                orc.reset_robot_state(reset_ref.astype(np.uint8), us, np.array(robot.min_init_state, np.float32),
                                      np.array(robot.max_init_state, np.float32), nb_min.astype(np.float32), nb_max.astype(np.float32),
                                      st_reset)
                assert max_abs(post["state"][reset_ref], st_reset[reset_ref]) < 2e-6, t
                assert np.array_equal(post["ep"], pre["ep"] + reset_ref), t
                assert np.all(post["steps"][reset_ref] == 0)
            assert np.array_equal(post["bmin"], bmin_ref) and np.array_equal(post["bmax"], bmax_ref), t
            assert np.array_equal(post["asset"][..., :3], asset_ref[..., :3]), t            # obstacle positions: bit-exact
            assert np.abs(post["asset"][..., 3:7] - asset_ref[..., 3:7]).max() < 3e-7, t
            # ---------------- scene + sensor on the product's post-reset buffers (bit-exact path)
            tris_ref = orc.scene_transform(tri_local, tri_asset, post["asset"])
            assert np.array_equal(post["tri_world"], tris_ref), t
            lpos, lquat = npy(sensor.sensor_local_position), npy(sensor.sensor_local_orientation)
            if reset_ref.any():
                # task targets and sensor mounts of the reset envs: device streams of (env, new episode)
                f32 = np.float32
                u4 = orc.rng_fill(seed, post["ep"], orc.RNG_TARGET, 4)
                lo_t, hi_t = np.array(cfg.target_min_ratio, f32), np.array(cfg.target_max_ratio, f32)
                tgt_ref = post["bmin"] + (post["bmax"] - post["bmin"]) * ((hi_t - lo_t) * u4[:, 0:3] + lo_t)
                assert np.array_equal(post["target"][reset_ref], tgt_ref[reset_ref].astype(f32)), t
                assert np.array_equal(post["target"][~reset_ref], pre["target"][~reset_ref]), t
                um = orc.rng_fill(seed, post["ep"], orc.RNG_SENSOR_MOUNT, 6)
                sc_ = sensor.cfg
                lo_p, hi_p = np.array(sc_.min_translation, f32), np.array(sc_.max_translation, f32)
                lo_e = np.array([np.radians(v) for v in sc_.min_euler_rotation_deg], f32)
                hi_e = np.array([np.radians(v) for v in sc_.max_euler_rotation_deg], f32)
                assert np.array_equal(lpos[reset_ref, 0], ((hi_p - lo_p) * um[:, 0:3] + lo_p)[reset_ref]), t
                q_ref = orc.quat_from_euler(((hi_e - lo_e) * um[:, 3:6] + lo_e).astype(f32))
                assert np.abs(lquat[reset_ref, 0] - q_ref[reset_ref]).max() < 3e-7, t
            spos, squat = orc.sensor_pose(post["state"], lpos, lquat, frame)
            assert np.array_equal(npy(sensor.sensor_position), spos) and np.array_equal(npy(sensor.sensor_orientation), squat), t
            if sensor.is_lidar:
                px_ref, seg_ref = orc.raycast_lidar(rays, float(scfg.max_range), "range", spos, squat, tris_ref, tri_seg, use_bvh=use_bvh)
            else:
                px_ref, seg_ref = orc.raycast_camera(scfg.width, scfg.height, kinv, float(scfg.max_range), cx, cy, "depth", spos, squat,
                                                     tris_ref, tri_seg, use_bvh=use_bvh)
            px_ref = orc.sensor_postprocess(px_ref, float(scfg.min_range), float(scfg.max_range), float(scfg.far_out_of_range_value),
                                            float(scfg.near_out_of_range_value), bool(scfg.normalize_range))
            assert np.array_equal(npy(g["segmentation_pixels"]), seg_ref), t                # segmentation ids: bit-exact
            assert np.array_equal(npy(g["depth_range_pixels"]), px_ref), t                  # normalised depth: bit-exact
            # ---------------- observation (fresh derived tensors of reset steps come from update_states)
            u6 = orc.rng_fill(seed, np.full(n, env.step_counter - 1), 6, 6)  # RNG_OBS_NOISE of (env, this env step)
            obs_ref = orc.obs_navigation(post["state"], post["euler"], post["qveh"], post["vbody"], post["wbody"], post["actions"],
                                         post["target"], u6[:, 0:3], u6[:, 3:6], px_ref, cfg.observation_space_dim)
            parity.check(f"nav_task_obs[{case}]", max_abs(npy(obs["observations"]), obs_ref), 0.0, "abs (bit-exact)", t)
            # post_image_reward_addition's minimum (navigation_task.py:351-357), produced by the observation kernel's sweep
            v10 = 10.0 * px_ref.reshape(n, -1)
            v10[v10 < 0] = 10.0
            assert np.array_equal(npy(task.min_pixel_dist), v10.min(axis=1)), t
            if reset_ref.any():  # the reference refreshes EVERY env's derived tensors when any env resets
                eu, qv, vv, vb, wb = orc.update_states(post["state"])
                assert max_abs(post["vbody"], vb) < 1e-5 and max_abs(post["qveh"], qv) < 1e-5, t
        need = 2 * n if min_resets is None else min_resets
        assert n_resets >= need and (n_crashes >= 1 or "lidar" in case), (n_resets, n_crashes)  # truncations and collisions seen
        return dict(resets=n_resets, crashes=n_crashes)
    finally:
        cfg.episode_len_steps, cfg.args, cfg.device = old_cfg
        cfg.curriculum.min_level, cfg.curriculum.max_level = old_cur


@pytest.mark.parametrize("shape", [(48, 64), (32, 512), (30, 50), (270, 480), (5, 7), (64, 1024), (17, 200)])
def test_observation_min_pool_any_image_shape(orc, shape):
    """agx_obs_navigation's 8 x 8 min-pool is a coalesced sweep (64 consecutive pixels per load, cells reduced across
    lanes): every arrangement -- cell width a power of two below 64, 64 and above, not a power of two, cells that
    straddle a 64-pixel chunk, empty cells, several sensors -- gives the bits of the serial loop; min_pixel (one sensor)
    == agx_image_min."""
    from aerial_gym_simulator_amd import _lib

    lib = _lib.load()
    H, W = shape
    n, obs_dim = 5, 81
    rng = np.random.default_rng(H * 1000 + W)
    f32 = np.float32
    state = rng.normal(size=(n, 13)).astype(f32)
    state[:, 3:7] /= np.linalg.norm(state[:, 3:7], axis=1, keepdims=True)
    euler, qveh, vveh, vbody, wbody = orc.update_states(state)
    actions, target = rng.normal(size=(n, 4)).astype(f32), rng.normal(size=(n, 3)).astype(f32)
    u_vec, u_eul = rng.random((n, 3)).astype(f32), rng.random((n, 3)).astype(f32)
    for S in (1, 2):
        px = rng.uniform(-1.0, 1.0, (n, S, H, W)).astype(f32)
        px[rng.random(px.shape) < 0.3] = -1.0
        derived = np.concatenate([euler, qveh, vveh, vbody, wbody], axis=1).astype(f32)
        t = {k: torch.from_numpy(np.ascontiguousarray(v.T)).to(DEV) for k, v in (("state", state), ("derived", derived),
                                                                                 ("actions", actions), ("target", target))}
        tu, te, tpx = torch.from_numpy(u_vec).to(DEV), torch.from_numpy(u_eul).to(DEV), torch.from_numpy(px).to(DEV)
        obs, mp, mp_ref = torch.zeros(n, obs_dim, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        B = _lib.AgxEnvBuffers()
        B.state, B.derived, B.actions, B.flag_parity = _lib.dptr(t["state"]), _lib.dptr(t["derived"]), _lib.dptr(t["actions"]), 0
        st = _lib.current_stream(DEV)
        _lib.check(lib.agx_obs_navigation(B, n, _lib.dptr(t["target"]), _lib.dptr(tu), _lib.dptr(te), _lib.dptr(tpx), S, H, W, 8, 8,
                                          obs_dim, _lib.dptr(obs), _lib.dptr(mp) if S == 1 else None, st))
        ref = orc.obs_navigation(state, euler, qveh, vbody, wbody, actions, target, u_vec, u_eul, px, obs_dim)
        assert np.array_equal(obs.cpu().numpy(), ref), (shape, S)
        if S == 1:
            _lib.check(lib.agx_image_min(n, H * W, _lib.dptr(tpx), _lib.dptr(mp_ref), st))
            assert np.array_equal(mp.cpu().numpy(), mp_ref.cpu().numpy())
        else:  # several sensors: the observation covers sensor 0 only, the minimum all of them -> refused
            assert lib.agx_obs_navigation(B, n, _lib.dptr(t["target"]), _lib.dptr(tu), _lib.dptr(te), _lib.dptr(tpx), S, H, W, 8, 8,
                                          obs_dim, _lib.dptr(obs), _lib.dptr(mp), st) == -1


def test_bookkeeping_and_target_reset_kernels_vs_the_reference_task_glue():
    """agx_nav_bookkeeping / agx_nav_target_reset on the 60-step sequence recorded from the reference's REAL
    NavigationTask (tests/golden/navigation_glue.npz, oracle/gen_golden_nav_glue.py): success / timeout flags,
    the three curriculum counters, and the resampled targets (bit for bit)."""
    import ctypes as C

    from conftest import golden_params, load_golden
    from gpu_harness import DynHarness

    from aerial_gym_simulator_amd import _lib

    g = load_golden("navigation_glue")
    T, n = g["position"].shape[0], g["position"].shape[1]
    H = DynHarness(golden_params(load_golden("step_quad_position")), n)
    lib = H.lib
    target = torch.from_numpy(np.ascontiguousarray(g["initial_target"].T)).to(DEV)          # SoA [3][N]
    succ = torch.zeros(n, dtype=torch.uint8, device=DEV)
    tout = torch.zeros(n, dtype=torch.uint8, device=DEV)
    counters = torch.zeros(3, dtype=torch.int32, device=DEV)
    lo = (C.c_float * 3)(*g["target_min_ratio"].tolist())
    hi = (C.c_float * 3)(*g["target_max_ratio"].tolist())
    state = np.zeros((n, 13), np.float32)
    state[:, 6] = 1.0
    want = np.zeros(3, np.int64)
    for t in range(T):
        state[:, 0:3] = g["position"][t]
        H.set(state=state)
        H.crashes.copy_(torch.from_numpy(g["crashes"][t].astype(bool)))
        H.trunc.copy_(torch.from_numpy(g["truncations"][t].astype(bool)))
        _lib.check(lib.agx_nav_bookkeeping(H.B, n, _lib.dptr(target), 1.0, _lib.dptr(succ), _lib.dptr(tout), _lib.dptr(counters),
                                           H.stream()), "agx_nav_bookkeeping")
        d = g["target_before"][t] - g["position"][t]
        edge = np.abs(np.sqrt((d.astype(np.float64) ** 2).sum(axis=1)) - 1.0) < 1e-6
        got_s, got_t = succ.cpu().numpy().astype(bool), tout.cpu().numpy().astype(bool)
        assert np.array_equal(got_s[~edge], g["successes"][t].astype(bool)[~edge]), t
        assert np.array_equal(got_t[~edge], g["timeouts"][t].astype(bool)[~edge]), t
        want += [int(got_s.sum()), int(g["crashes"][t].sum()), int(got_t.sum())]
        assert counters.cpu().tolist() == want.tolist(), t
        # the simulator resets (new bounds), then the task resamples the targets of those envs
        mask = g["reset_mask"][t]
        H.reset_mask.copy_(torch.from_numpy(mask))
        H.reset_flag[0] = int(mask.any())
        H.set(bmin=g["bounds_min"][t], bmax=g["bounds_max"][t])
        u = torch.zeros(n, 4, device=DEV)
        u[:, 0:3] = torch.from_numpy(g["u_target"][t])
        _lib.check(lib.agx_nav_target_reset(H.B, n, 4, lo, hi, _lib.dptr(u), _lib.dptr(target), None, 0, H.stream()),
                   "agx_nav_target_reset")
        assert np.array_equal(target.cpu().numpy().T, g["target_after"][t]), t
    assert want[0] > 100 and want[2] > 100


@pytest.mark.parametrize("task_name,cfg_name", [("navigation_task", "navigation_task_config"),
                                                ("lidar_navigation_task", "lidar_navigation_task_config")])
def test_replayed_step_graph_equals_eager_stepping(task_name, cfg_name):
    """Small batches replay the step as a hipGraph (one launch instead of ~15; task/navigation_task.py `_graph_mode`): same
    seed, same actions, graph on vs off -> bit-identical observations, rewards, flags, images and states over 80 steps
    that include resets (episodes of 9 steps), both reset-flag parities, the action ring of the LiDAR task and the
    device-resident step counter behind the per-step noise streams."""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config import task_config as tc
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    cfg = getattr(tc, cfg_name)
    old = (cfg.episode_len_steps, cfg.args, cfg.device)
    n = 48
    tasks = []
    try:
        for use_graph in (False, True):
            cfg.device, cfg.episode_len_steps = DEV, 9
            cfg.args = {"rng_seed": 4242, "step_graph": use_graph}
            t = task_registry.make_task(task_name, seed=6, num_envs=n, headless=True)
            t.reset()
            tasks.append(t)
        eager, graphed = tasks
        g = torch.Generator(device=DEV).manual_seed(1)
        for step in range(80):
            a = torch.rand(n, 4, device=DEV, generator=g) * 2 - 1
            outs = [t.step(a) for t in tasks]
            torch.cuda.synchronize()
            (o0, r0, te0, tr0, _), (o1, r1, te1, tr1, _) = outs
            assert torch.equal(o0["observations"], o1["observations"]), step
            assert torch.equal(r0, r1) and torch.equal(te0, te1) and torch.equal(tr0, tr1), step
            assert torch.equal(eager.obs_dict["robot_state_tensor"], graphed.obs_dict["robot_state_tensor"]), step
            assert torch.equal(eager.obs_dict["depth_range_pixels"], graphed.obs_dict["depth_range_pixels"]), step
        assert graphed._graphs and len(graphed._graphs) >= 2  # both parities were captured and replayed
        assert eager._graphs is False
        assert int(graphed.sim_env.global_tensor_dict["episode_count"].sum()) >= 7 * n
        assert graphed.sim_env.step_counter == eager.sim_env.step_counter == 80
        assert int(graphed.sim_env._step_counter_dev[0]) == 80
    finally:
        cfg.episode_len_steps, cfg.args, cfg.device = old


@pytest.mark.parametrize("task_name,cfg_name", [("navigation_task", "navigation_task_config"),
                                                ("lidar_navigation_task", "lidar_navigation_task_config")])
def test_fused_robot_side_launch_equals_the_four_separate_launches(task_name, cfg_name, monkeypatch):
    """agx_nav_robot_side (robot reset + sensor mounts + target of the envs that reset + every sensor's pose, one launch) against
    agx_reset_masked / agx_sensor_mount_reset / agx_nav_target_reset / agx_sensor_pose (args={"fused_robot_side": False}): same seed, same
    actions -> bit-identical observations, rewards, flags, states, targets, mounts, sensor poses and images over 60 steps with
    episodes of 7 steps (resets on most steps)."""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config import task_config as tc
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    cfg = getattr(tc, cfg_name)
    old = (cfg.episode_len_steps, cfg.args, cfg.device)
    n = 40
    tasks = []
    try:
        for fused in (False, True):
            cfg.device, cfg.episode_len_steps = DEV, 7
            cfg.args = {"rng_seed": 99, "fused_robot_side": fused}
            t = task_registry.make_task(task_name, seed=3, num_envs=n, headless=True)
            t.reset()
            tasks.append(t)
        separate, fused = tasks
        g = torch.Generator(device=DEV).manual_seed(2)
        for step in range(60):
            a = torch.rand(n, 4, device=DEV, generator=g) * 2 - 1
            out0 = separate.step(a)
            out1 = fused.step(a)
            torch.cuda.synchronize()
            (o0, r0, te0, tr0, _), (o1, r1, te1, tr1, _) = out0, out1
            assert torch.equal(o0["observations"], o1["observations"]), step
            assert torch.equal(r0, r1) and torch.equal(te0, te1) and torch.equal(tr0, tr1), step
            for key in ("robot_state_tensor", "depth_range_pixels"):
                assert torch.equal(separate.obs_dict[key], fused.obs_dict[key]), (step, key)
            assert torch.equal(separate.target_soa, fused.target_soa), step
            s0, s1 = separate.sim_env.robot_manager.warp_sensor, fused.sim_env.robot_manager.warp_sensor
            for name in ("sensor_local_position", "sensor_local_orientation", "sensor_position", "sensor_orientation"):
                assert torch.equal(getattr(s0, name), getattr(s1, name)), (step, name)
        assert separate._fused_side is False and fused._fused_side not in (None, False)
        assert int(fused.sim_env.global_tensor_dict["episode_count"].sum()) >= 6 * n
    finally:
        cfg.episode_len_steps, cfg.args, cfg.device = old


@pytest.mark.parametrize("n", [40, 2304])
def test_folded_step_launches_equal_the_separate_ones(n, monkeypatch):
    """round 5: the navigation step without three of its small launches -- the success / timeout / curriculum
    bookkeeping in the env-step launch's epilogue (AgxTaskArgs.successes ...) and the obstacle reset + mask compaction inside the
    geometry refresh (agx_scene_reset_refresh: ONE launch up to 2048 envs, the three launches above) -- against the separate
    launches (args={"fused_bookkeeping": False, "fused_asset_reset": False}): same seed, same actions -> bit-identical observations, rewards,
    flags, bookkeeping, obstacle poses, triangles, trees and images, resets on most steps.  n = 2304: the large-batch form."""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config import task_config as tc
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    cfg = tc.navigation_task_config
    old = (cfg.episode_len_steps, cfg.args, cfg.device)
    tasks = []
    try:
        for fused in (False, True):
            cfg.device, cfg.episode_len_steps = DEV, 7
            cfg.args = {"rng_seed": 77, "fused_bookkeeping": fused, "fused_asset_reset": fused}
            t = task_registry.make_task("navigation_task", seed=3, num_envs=n, headless=True)
            t.reset()
            tasks.append(t)
        separate, fused = tasks
        assert fused._bookkeeping_fused and not separate._bookkeeping_fused
        g = torch.Generator(device=DEV).manual_seed(2)
        steps = 40 if n < 1000 else 12
        for step in range(steps):
            a = torch.rand(n, 4, device=DEV, generator=g) * 2 - 1
            for t in (separate, fused):
                t._out = t.step(a)
            torch.cuda.synchronize()
            (o0, r0, te0, tr0, i0), (o1, r1, te1, tr1, i1) = separate._out, fused._out
            assert torch.equal(o0["observations"], o1["observations"]), step
            assert torch.equal(r0, r1) and torch.equal(te0, te1) and torch.equal(tr0, tr1), step
            assert torch.equal(separate._successes, fused._successes) and torch.equal(separate._timeouts, fused._timeouts), step
            assert torch.equal(separate._counters, fused._counters), step
            for key in ("robot_state_tensor", "depth_range_pixels", "env_asset_state_tensor", "scene_tri_world", "scene_bvh_nodes"):
                a0, a1 = separate.obs_dict[key], fused.obs_dict[key]
                assert torch.equal(a0.view(torch.int32) if a0.is_floating_point() else a0, a1.view(torch.int32) if a1.is_floating_point() else a1), (step, key)
            assert torch.equal(separate.sim_env.scene.boxes_soa, fused.sim_env.scene.boxes_soa), step
        assert int(fused.sim_env.global_tensor_dict["episode_count"].sum()) >= (steps // 8) * n
        assert int(fused.success_aggregate + fused.crashes_aggregate + fused.timeouts_aggregate) == int(
            separate.success_aggregate + separate.crashes_aggregate + separate.timeouts_aggregate)
    finally:
        cfg.episode_len_steps, cfg.args, cfg.device = old


def test_builtin_action_transformations_as_one_launch():
    """agx_action_transform (what the tasks use when the config carries the built-in function) against the torch functions of
    config/task_config.py evaluated in float64-backed numpy: the linear columns bit for bit, sine / cosine correctly rounded
    (torch's device sin / cos are 1-2 ulp implementations; the kernels' are float64 inside, rounded once)."""
    import ctypes as C

    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd.config import task_config as tc

    lib = _lib.load()
    n = 1 << 16
    a = torch.rand(n, 4, device=DEV, generator=torch.Generator(device=DEV).manual_seed(8)) * 3.0 - 1.5
    an = np.clip(a.cpu().numpy(), -1.0, 1.0).astype(np.float32)
    f32 = np.float32
    for cfg, width in ((tc.navigation_task_config, 4), (tc.lidar_navigation_task_config, 4), (tc.fully_actuated_lidar_navigation_task_config, 7)):
        kind = cfg.action_transformation_function.agx_kind
        assert kind[1] == width
        out = torch.empty(n, width, device=DEV)
        _lib.check(lib.agx_action_transform(kind[0], n, _lib.dptr(a), _lib.dptr(out), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        got = out.cpu().numpy()
        ref_torch = cfg.action_transformation_function(a).cpu().numpy()
        assert np.abs(got - ref_torch).max() < 3e-7  # torch's own device sin / cos
        if kind[0] == 1:
            incl = (f32(np.pi / 4) * an[:, 1]).astype(f32)
            speed = (an[:, 0] + f32(1.0)).astype(f32)
            want = np.stack([speed * np.cos(incl.astype(np.float64)).astype(f32), np.zeros(n, f32),
                             speed * np.sin(incl.astype(np.float64)).astype(f32), an[:, 2] * f32(np.pi / 3)], axis=1)
        elif kind[0] == 2:
            want = np.concatenate([an[:, 0:3] * f32(2.0), (an[:, 3] * f32(np.pi / 3))[:, None]], axis=1)
        else:
            half = (f32(0.5 * np.pi) * an[:, 3]).astype(f32)
            want = np.stack([an[:, 0] * f32(5), an[:, 1] * f32(5), an[:, 2] * f32(2.5), np.zeros(n, f32), np.zeros(n, f32),
                             np.sin(half.astype(np.float64)).astype(f32), np.cos(half.astype(np.float64)).astype(f32)], axis=1)
        assert np.array_equal(got, want.astype(f32)), (kind, np.abs(got - want).max())
        # a NaN action (a diverged policy) stays NaN wherever torch.clamp + the torch function leave it NaN -- the fused launch
        # must not turn it into a valid command (fminf / fmaxf alone map NaN to -1)
        bad = a[:8].clone()
        for c in range(4):
            bad[2 * (c % 4):2 * (c % 4) + 2, c] = float("nan")
        outb = torch.zeros(8, width, device=DEV)
        _lib.check(lib.agx_action_transform(kind[0], 8, _lib.dptr(bad), _lib.dptr(outb), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        refb = cfg.action_transformation_function(bad)
        assert torch.equal(torch.isnan(outb), torch.isnan(refb)), (kind, outb, refb)
        assert torch.isnan(refb).any()


def test_action_transformation_forms_agree_on_the_device():
    """navigation_task_config.action_transformation_function (9 launches) against the reference's wording (17): equal bit for
    bit on the device too (`* 2.0 / 2.0` is exact)."""
    from aerial_gym_simulator_amd.config.task_config import navigation_task_config as cfg

    a = torch.rand(1 << 16, 4, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) * 3.0 - 1.5
    assert torch.equal(cfg.action_transformation_function(a), cfg.action_transformation_function_as_written(a))


def test_curriculum_level_change_applies_to_the_resets_of_the_check_step():
    """navigation_task.py:327-331: check_and_update_curriculum_level runs BEFORE post_reward_calculation_step, so the envs
    that reset on a check step are repopulated with the NEW level's obstacle count.  Eager stepping in the sync-free mode
    follows that order (one host read of the three counters every `curriculum_check_every` steps); only a step that is
    captured into / replayed from a hipGraph applies the level one step later."""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config.task_config import navigation_task_config as cfg
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    old = (cfg.episode_len_steps, cfg.args, cfg.device)
    n = 32
    try:
        cfg.device, cfg.episode_len_steps, cfg.args = DEV, 3, {"rng_seed": 77}
        t = task_registry.make_task("navigation_task", seed=3, num_envs=n, headless=True)
        t.reset()
        c = t.task_config.curriculum
        every = t.curriculum_check_every
        a = torch.zeros(n, 4, device=DEV)
        while t.num_task_steps % every != every - 1:  # stop one step short of a check step
            t.step(a)
        assert t.num_task_steps % every != 0
        t.step(a)
        lvl0 = t.curriculum_level
        assert t.num_task_steps % every == 0 and lvl0 + c.increase_step <= c.max_level
        pos = t.sim_env.global_tensor_dict["env_asset_state_tensor"][..., 0:3]
        count = lambda: (pos[..., 0] > -999.0).sum(dim=1).cpu().numpy()  # noqa: E731  assets not parked at -1000 m, per env
        t.sim_env.sim_steps.fill_(cfg.episode_len_steps + 1)  # every env truncates -> every env is repopulated at the old level
        t._counters.zero_()
        while t.num_task_steps % every != 0:
            t.sim_env.sim_steps.fill_(cfg.episode_len_steps + 1)
            t.step(a)
        before = count()
        # (a bernoulli(0.15) subset of the reset envs keeps only half of its obstacles, env_manager.py:283-295: the level is the maximum)
        assert t.curriculum_level == lvl0 and before.max() == lvl0 and set(before.tolist()) <= {lvl0, lvl0 // 2}
        # this step is a check step: 100 % successes on the books, and every env truncates (so every env resets in it)
        t._counters.copy_(torch.tensor([10 * c.check_after_log_instances, 0, 0], dtype=torch.int32))
        t.sim_env.sim_steps.fill_(cfg.episode_len_steps + 1)
        t.step(a)
        torch.cuda.synchronize()
        assert t.curriculum_level == lvl0 + c.increase_step
        after = count()
        new = lvl0 + c.increase_step  # the resets of THIS step used the new level
        assert after.max() == new and set(after.tolist()) <= {new, new // 2}, (before, after)
    finally:
        cfg.episode_len_steps, cfg.args, cfg.device = old
