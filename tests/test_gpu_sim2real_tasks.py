"""GPU: the two lmf2 sim2real set-point tasks -- the three agx_sim2real_* kernels through the C ABI against the reference's own
numbers (tests/golden/sim2real_cr/*.npz, bit for bit), the tasks through the Task API against tests/sim2real_ref.py applied to
snapshots of the dict tensors (bit for bit; that restatement is pinned to the reference by tests/test_sim2real_tasks.py), and
the two actors the reference trained flying task.step() on the task's own noisy observations."""
import os

import numpy as np
import pytest
import sim2real_ref as R
import torch
from task_test_util import DEV, Buffers, RecordingSource, config_restored, dev, host, load_golden, offset_consumed_by, rows, soa
from task_test_util import same_bits as same

pytestmark = pytest.mark.gpu
CR = "sim2real_cr"  # the fixtures made by the reference's code with correctly rounded elementary functions
CONFIG_KEYS = ("seed", "num_envs", "headless", "device", "use_warp", "args", "episode_len_steps")
KINDS = (("velocity", R.VELOCITY), ("acceleration", R.ACCELERATION))
NAMES = {"velocity": "position_setpoint_task_sim2real", "acceleration": "position_setpoint_task_acceleration_sim2real"}
SIZES = (1, 63, 64, 65, 257)  # a partial wave, the exact wave, one over, more than four waves


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind,k", KINDS)
def test_reward_kernel_equals_the_reference_bit_for_bit(kind, k, n):
    g = load_golden("sim2real_reward", CR)
    G = lambda name: rows(g[kind + "_" + name], n)  # noqa: E731
    episode_len = 4
    sim_steps = (np.arange(n) * 3) % 9
    H = Buffers(n, G("position"), G("orientation"), vehicle_orientation=G("vehicle_orientation"), body_linvel=G("body_linvel"),
                body_angvel=G("body_angvel"), crashes=G("crashes_in"),
                sim_steps=sim_steps)
    p = H._lib.dptr
    target, act, pact, pd = soa(G("target")), dev(G("actions")), dev(G("prev_actions")), dev(G("prev_dist"))
    pavf = dev(G("prev_actions_vehicle_frame"))
    avf = torch.full((n, 4), -7.0, device=DEV)
    rew = torch.zeros(n, device=DEV)
    H._lib.check(H.lib.agx_sim2real_reward(k, H.B, n, p(target), p(act), p(pact), p(pd), p(avf), p(pavf), episode_len, 1, p(rew), H.stream()),
                 "agx_sim2real_reward")
    torch.cuda.synchronize()
    assert same(host(rew), G("reward"))
    crashes = G("crashes_out").astype(bool)
    assert np.array_equal(host(H.crashes), crashes)
    trunc = sim_steps > episode_len
    assert np.array_equal(host(H.truncations), trunc)
    assert np.array_equal(host(H.reset_mask), (crashes | trunc).astype(np.uint8))
    assert host(H.reset_flag).tolist() == [0, int((crashes | trunc).any())]  # the flag word of this step's parity only
    if k == R.ACCELERATION:
        assert same(host(avf), G("actions_vehicle_frame"))
    else:
        assert (host(avf) == -7.0).all()
    assert same(host(act), G("actions")) and same(host(pd), G("prev_dist"))  # inputs untouched


def test_reward_kernel_without_reset_on_collision_and_on_the_other_parity():
    g = load_golden("sim2real_reward", CR)
    n, kind, k = 65, "velocity", R.VELOCITY
    G = lambda name: rows(g[kind + "_" + name], n)  # noqa: E731
    H = Buffers(n, G("position"), G("orientation"), vehicle_orientation=G("vehicle_orientation"), body_linvel=G("body_linvel"),
                body_angvel=G("body_angvel"), crashes=G("crashes_in"), parity=0)
    p = H._lib.dptr
    target, act, pact, pd = soa(G("target")), dev(G("actions")), dev(G("prev_actions")), dev(G("prev_dist"))
    rew = torch.zeros(n, device=DEV)
    H._lib.check(H.lib.agx_sim2real_reward(k, H.B, n, p(target), p(act), p(pact), p(pd), None, None, 800, 0, p(rew), H.stream()),
                 "agx_sim2real_reward")
    torch.cuda.synchronize()
    assert same(host(rew), G("reward")) and G("crashes_out").any()
    assert not host(H.reset_mask).any() and host(H.reset_flag).tolist() == [0, 0]


@pytest.mark.parametrize("n", SIZES)
def test_obs_kernel_equals_the_reference_bit_for_bit(n):
    g = load_golden("sim2real_obs", CR)
    G = lambda name: rows(g[name], n)  # noqa: E731
    s = G("state")
    H = Buffers(n, s[:, 0:3], s[:, 3:7], body_linvel=G("body_linvel"), body_angvel=G("body_angvel"), robot_actions=G("robot_actions"))
    p = H._lib.dptr
    z = dev(np.stack([rows(g["z"][j], n) for j in range(4)]))
    target = soa(G("target"))
    obs = torch.zeros(n, 17, device=DEV)
    H._lib.check(H.lib.agx_sim2real_obs(H.B, n, p(target), p(z), p(obs), H.stream()), "agx_sim2real_obs")
    torch.cuda.synchronize()
    assert same(host(obs), G("obs"))
    state = host(H.state).T
    assert same(state[:, 3:7], G("orientation_after"))  # sign(w) q stored back: zeros (signed) where w = +-0
    assert same(state[:, 0:3], s[:, 0:3]) and not state[:, 7:13].any()
    # exchange rows are not written for the 17-D observation: refused, not ignored
    H.B.step_rows[0] = H.B.step_rows[1] = p(obs)
    assert H.lib.agx_sim2real_obs(H.B, n, p(target), p(z), p(obs), H.stream()) != 0
    assert "step_rows" in H.lib.agx_last_error().decode()


def pre_step_rows(g, kind, steps):
    """inputs / outputs of step()'s first lines from the reference's real step() on the scripted simulator, steps stacked as rows"""
    G = lambda name: g[kind + "_" + name]  # noqa: E731
    before = [G("action_in")[t] if t < 7 else G("action_after")[t - 1] for t in steps]  # what task.actions read at the call
    cat = lambda name: np.concatenate([G(name)[t] for t in steps])  # noqa: E731
    d = dict(before=np.concatenate(before), **{name: cat(name) for name in ("target", "pre_position", "pre_orientation", "action_in",
                                                                            "action_after", "prev_actions", "prev_dist")})
    if kind == "acceleration":
        d["prev_actions_vehicle_frame"] = cat("prev_actions_vehicle_frame")
    return d


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("aliased", [False, True])
@pytest.mark.parametrize("kind,k", KINDS)
def test_pre_step_kernel_equals_the_reference_bit_for_bit(kind, k, aliased, n):
    """aliased: the caller reuses ONE action buffer, so task.actions and the incoming tensor are the same memory (steps 1-6 of the
    golden); otherwise the previous call's tensor is another one (all steps)."""
    g = load_golden("sim2real_glue", CR)
    d = pre_step_rows(g, kind, range(1, 7) if aliased else range(1, 12))
    D = lambda name: rows(d[name], n)  # noqa: E731
    H = Buffers(n, D("pre_position"), D("pre_orientation"))
    p = H._lib.dptr
    target, act = soa(D("target")), dev(D("action_in"))
    before = act if aliased else dev(D("before"))
    pact, pd, pavf = torch.full((n, 4), -7.0, device=DEV), torch.zeros(n, device=DEV), torch.full((n, 4), -7.0, device=DEV)
    H._lib.check(H.lib.agx_sim2real_pre_step(k, H.B, n, p(target), p(before), p(act), p(pact), p(pd), p(pavf), H.stream()),
                 "agx_sim2real_pre_step")
    torch.cuda.synchronize()
    assert same(host(pact), D("prev_actions")) and same(host(pd), D("prev_dist"))
    assert same(host(act), D("action_after"))  # doubled in place for the acceleration task, untouched otherwise
    if k == R.ACCELERATION:
        assert same(host(pavf), D("prev_actions_vehicle_frame"))
        assert same(host(act)[:, 0:3], np.float32(2.0) * D("action_in")[:, 0:3])
    else:
        assert (host(pavf) == -7.0).all()
    assert same(host(H.state).T[:, 0:7], np.concatenate([D("pre_position"), D("pre_orientation")], axis=1))


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("kind,k", KINDS)
def test_task_trace_equals_the_restatement_on_the_dict_tensors(kind, k, strict):
    """65 envs, 60 steps, episodes of 20 steps, five targets moved 11 m away at step 25: truncation resets and distance crashes.
    Everything task.step() leaves behind equals tests/sim2real_ref.py applied to the tensors the kernels read, bit for bit."""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    n, steps, episode_len = 65, 60, 20
    cfg = task_registry.get_task_config(NAMES[kind])
    rs = RecordingSource(DEV)
    with config_restored(cfg, CONFIG_KEYS):
        cfg.args = {"ray_cast_sensors": "off", "random_source": rs, "strict_rng": strict}
        cfg.episode_len_steps = episode_len
        task = task_registry.make_task(NAMES[kind], seed=11, num_envs=n, headless=True)
        env, d = task.sim_env, task.obs_dict
        snap = {}
        real_reward, real_obs = task.compute_rewards_and_crashes, task.process_obs_for_task

        def hooked_reward(obs_dict):
            snap["reward"] = {key: host(d[key]).copy() for key in ("robot_position", "robot_orientation", "robot_vehicle_orientation",
                                                                   "robot_body_linvel", "crashes")}
            snap["reward"]["sim_steps"] = host(env.sim_steps).copy()
            return real_reward(obs_dict)

        def hooked_obs():
            snap["obs"] = {key: host(d[key]).copy() for key in ("robot_position", "robot_orientation", "robot_body_linvel", "robot_body_angvel",
                                                                "robot_actions", "robot_state_tensor")}
            before = torch.cuda.default_generators[0].get_offset()
            r = real_obs()
            snap["obs_offset"] = torch.cuda.default_generators[0].get_offset() - before
            return r

        task.compute_rewards_and_crashes, task.process_obs_for_task = hooked_reward, hooked_obs
        task.reset()
        ref = R.TaskRef(k, n)
        gen = torch.Generator().manual_seed(5)
        buf = torch.zeros(n, 4, device=DEV)      # the caller's buffer, reused and overwritten for the first 30 steps ...
        buf_ref = np.zeros((n, 4), np.float32)   # ... and its mirror on the restatement's side
        ref.actions = host(task.actions).copy()
        gpu_gen = torch.cuda.default_generators[0]
        seen = {"trunc": 0, "crash": 0, "reset_steps": 0}
        for t in range(steps):
            if t == 25:
                task.target_position[3:8, 0] = 11.0
            a = torch.rand(n, 4, generator=gen) * 2.0 - 1.0
            if t < 30:
                buf.copy_(a)
                buf_ref[:] = a.numpy()
                handed, handed_ref = buf, buf_ref
            else:
                handed, handed_ref = a.to(DEV), a.numpy().copy()
            ref.target = host(task.target_position).copy()
            pre = {key: host(d[key]).copy() for key in ("robot_position", "robot_orientation")}
            del rs.normals[:], rs.calls[:]
            offset = gpu_gen.get_offset()
            obs, rew, term, trunc, _ = task.step(handed)
            torch.cuda.synchronize()
            consumed = gpu_gen.get_offset() - offset
            # -- step()'s first lines
            ref.pre_step(pre["robot_position"], pre["robot_orientation"], handed_ref)
            assert task.actions is handed and same(host(handed), handed_ref), t
            assert same(host(task.prev_actions), ref.prev_actions) and same(host(task.prev_dist), ref.prev_dist), t
            # -- reward, flags, reset set on the tensors as EnvManager.step left them
            s = snap["reward"]
            r = ref.reward(s["robot_position"], s["robot_orientation"], s["robot_vehicle_orientation"], s["robot_body_linvel"], s["crashes"],
                           s["sim_steps"], episode_len, env.cfg.env.reset_on_collision)
            assert same(host(rew), r["reward"]), (t, np.abs(host(rew) - r["reward"]).max())
            assert np.array_equal(host(term), r["crashes"]) and np.array_equal(host(trunc), r["truncations"]), t
            assert np.array_equal(host(d["reset_mask"]), r["reset_mask"].astype(np.uint8)), t
            assert same(host(task.actions_vehicle_frame), ref.actions_vehicle_frame), t
            assert same(host(task.prev_actions_vehicle_frame), ref.prev_actions_vehicle_frame), t
            # -- observation on the post-reset tensors, with the normals the task drew
            z = torch.stack(rs.normals) if strict else rs.normals[0]
            assert tuple(z.shape) == (4, n, 3) and [c[0] for c in rs.calls].count("normal") == (4 if strict else 1)
            s = snap["obs"]
            o, q = ref.observation(s["robot_position"], s["robot_orientation"], s["robot_body_linvel"], s["robot_body_angvel"],
                                   s["robot_actions"], host(z))
            assert same(host(obs["observations"]), o), (t, np.abs(host(obs["observations"]) - o).max())
            state = s["robot_state_tensor"].copy()
            state[:, 3:7] = q
            assert same(host(d["robot_state_tensor"]), state), t  # the quaternion write-back and nothing else
            assert (host(d["robot_orientation"])[:, 3] >= 0).all()
            if strict:  # the torch stream moves by exactly the calls the random source saw, in the reference's shapes
                normal_calls = [c for c in rs.calls if c[0] == "normal"]
                assert [(c[1], c[2]) for c in normal_calls] == [((n, 3), "sim2real_obs_noise_" + w) for w in ("euler", "pos", "linvel", "angvel")]
                assert consumed == offset_consumed_by(rs.calls), t
                # the task's own share is four [n, 3] normal fills on every step (lmf2 has disturbances enabled: the env step
                # draws a bernoulli and two uniforms per sub-step like the reference, so the step as a whole consumes more)
                assert snap["obs_offset"] == offset_consumed_by([("normal", (n, 3), "")] * 4), t
            seen["trunc"] += int(r["truncations"].sum())
            seen["crash"] += int((r["crashes"] & ~s_crashes(snap)).sum())
            seen["reset_steps"] += int(r["reset_mask"].any())
        assert seen["trunc"] >= 2 * (n - 5) and seen["crash"] >= 5 and 0 < seen["reset_steps"] < steps, seen
        task.close()


def s_crashes(snap):
    return snap["reward"]["crashes"].astype(bool)


def test_trainer_default_env_name_builds_and_steps_through_the_alias():
    """rl_games' ppo_aerial_quad.yaml of the reference trains `position_setpoint_task_sim2real`, made through the aerial_gym names"""
    from aerial_gym.config.task_config.position_setpoint_task_sim2real_config import task_config
    from aerial_gym.registry.task_registry import task_registry

    with config_restored(task_config, CONFIG_KEYS):
        task = task_registry.make_task("position_setpoint_task_sim2real", num_envs=128, headless=True)
        obs = task.reset()[0]
        for _ in range(3):
            obs, rew, term, trunc, info = task.step(torch.zeros(128, 4, device=DEV))
        torch.cuda.synchronize()
        assert obs["observations"].shape == (128, 17) and torch.isfinite(obs["observations"]).all() and torch.isfinite(rew).all()
        assert rew.shape == (128,) and term.dtype == torch.bool and trunc.dtype == torch.bool and info == {}
        with pytest.raises(ValueError, match="contiguous float32"):
            task.step(torch.zeros(128, 4, device=DEV, dtype=torch.float64))
        task.close()


@pytest.mark.parametrize("kind", ["acceleration", "velocity"])
def test_reference_trained_lmf2_policies_fly_the_tasks_on_their_own_noisy_observations(kind):
    """The closed loop of test_gpu_policy_transfer.py::fly_lmf2 through make_task: the actor the reference trained reads the task's
    noisy 17-D observation and task.step() takes its output (the acceleration task doubles it itself).  Same set-point criteria
    as there (set on noise-free runs with about 2x room; the 0.03 m observation noise is below them).  The mean episode return is
    printed next to the one rl_games logged for the network; it is not gated (the integrator is unpinned against PhysX)."""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.registry.task_registry import task_registry
    from test_gpu_policy_transfer import GOLDEN, LMF2, Actor

    n, steps = 2048, 800
    g = np.load(os.path.join(os.path.dirname(GOLDEN), LMF2[kind][0]))
    actor = Actor(g).to(DEV).eval()
    cfg = task_registry.get_task_config(NAMES[kind])
    with config_restored(cfg, CONFIG_KEYS):
        task = task_registry.make_task(NAMES[kind], seed=42, num_envs=n, headless=True)
        d = task.obs_dict
        obs = task.reset()[0]
        d0 = d["robot_position"].norm(dim=1).clone()
        ret = torch.zeros(n, device=DEV)
        dist, speed, crashed = [], [], torch.zeros(n, dtype=torch.bool, device=DEV)
        with torch.no_grad():
            for t in range(steps):
                a = actor(obs["observations"]).clamp(-1.0, 1.0).contiguous()
                obs, rew, term, trunc, _ = task.step(a)
                ret += rew
                crashed |= term
                if t >= steps - 100:
                    dist.append(d["robot_position"].norm(dim=1).clone())
                    speed.append(d["robot_linvel"].norm(dim=1).clone())
        dd = torch.stack(dist)
        r = {"start_dist_mean": float(d0.mean()), "dist_late_mean": float(dd.mean()), "dist_late_p95": float(dd.flatten().quantile(0.95)),
             "dist_late_max": float(dd.max()), "speed_late_mean": float(torch.stack(speed).mean()), "crashed": int(crashed.sum()),
             "truncated": int(trunc.sum()), "finite": bool(torch.isfinite(d["robot_state_tensor"]).all()),
             "mean_episode_return": float(ret.mean()), "logged_return": float(g["last_mean_rewards"])}
        print("policy transfer lmf2 through task.step():", kind, r)
        task.close()
    assert r["finite"] and r["crashed"] == 0 and r["truncated"] == 0
    assert r["start_dist_mean"] > 0.5
    assert r["dist_late_mean"] < 0.2 and r["dist_late_p95"] < 0.35 and r["speed_late_mean"] < 0.2
