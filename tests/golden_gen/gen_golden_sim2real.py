"""TEST INFRASTRUCTURE -- golden vectors of the two lmf2 sim2real set-point tasks, produced by running the REFERENCE's own
code (needs the reference tree, ref_shells.REFERENCE_ROOT; uses the helpers under oracle/ by path).

    python tests/golden_gen/gen_golden_sim2real.py [--cr] [--out DIR]

writes, into tests/golden/ (tests/golden/sim2real_cr/ with --cr: the same code with correctly rounded elementary functions,
oracle/cr_torch.py; tests/golden/cr/ is the fixed file set of oracle/gen_golden.py, which a test lists):

  sim2real_reward.npz   per kind (`velocity_*`, `acceleration_*`), n = 768: inputs and outputs of compute_rewards_and_crashes
                        (position_setpoint_task_sim2real.py:230-259 + :286-339, ..._acceleration_sim2real.py:239-273 + :300-356)
                        called as an unbound method on a stand-in object
  sim2real_obs.npz      n = 256: process_obs_for_task (:202-228) the same way; the four randn_like tensors it draws are re-drawn
                        from the same seed in the same order and stored; rows with w < 0, w = +0.0, w = -0.0, yaw next to +-pi
  sim2real_glue.npz     the real step() of both classes (their own constructor, reset, step) for 12 steps on a scripted stand-in
                        for the simulator: what the simulator would produce is scripted, everything the task derives is recorded
  sim2real_config.npz   the scalar values of the two task configs (JSON)
"""
import json
import math
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg  # noqa: E402  FIRST: it switches TorchScript off before torch is imported (cr_torch.py)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_shells  # noqa: E402

OUT = (sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
       else os.path.join(ROOT, "tests", "golden", *(["sim2real_cr"] if gg.CR else [])))
KINDS = {
    "velocity": ("position_setpoint_task_sim2real", "PositionSetpointTaskSim2Real"),
    "acceleration": ("position_setpoint_task_acceleration_sim2real", "PositionSetpointTaskAccelerationSim2Real"),
}
CONFIG_KEYS = ("seed", "sim_name", "env_name", "robot_name", "controller_name", "num_envs", "use_warp", "headless", "device",
               "observation_space_dim", "privileged_observation_space_dim", "action_space_dim", "episode_len_steps",
               "return_state_before_reset")


def task_module(kind):
    pkg, _ = KINDS[kind]
    name = "aerial_gym.task." + pkg
    if name not in sys.modules:  # (task/__init__.py registers every task: ref_shells bypasses it, sub-package by sub-package)
        sp = types.ModuleType(name)
        sp.__path__ = [os.path.join(ref_shells.REFERENCE_ROOT, "aerial_gym", "task", pkg)]
        sys.modules[name] = sp
    return ref_shells.ref("task.%s.%s" % (pkg, pkg))


def task_class(kind):
    return getattr(task_module(kind), KINDS[kind][1])


def unit_quats(n, rng):
    q = torch.randn(n, 4, generator=rng)
    return q / q.norm(dim=1, keepdim=True)


def gen_reward(rng):
    m = ref_shells.ref("utils.math")
    n = 768
    out = {}
    for kind in KINDS:
        cls = task_class(kind)
        # error lengths: ~10 % inside 0.2 m, a few percent beyond 10 m, the rest within a few metres
        u = torch.rand(n, generator=rng)
        length = torch.where(u < 0.1, torch.rand(n, generator=rng) * 0.2,
                             torch.where(u > 0.96, 10.0 + torch.rand(n, generator=rng) * 3.0 - 0.5, torch.rand(n, generator=rng) * 6.0))
        d = torch.randn(n, 3, generator=rng)
        err = d / d.norm(dim=1, keepdim=True) * length.unsqueeze(1)
        target = (torch.rand(n, 3, generator=rng) - 0.5) * 2.0
        position = target - err
        q = gg.random_state(n, rng)[:, 3:7]
        q[::5] = unit_quats(n, rng)[::5]  # any attitude, either sign of w
        qveh = m.vehicle_frame_quat_from_quat(q)
        vbody = torch.randn(n, 3, generator=rng)
        vbody[::6] *= 0.05
        wbody = torch.randn(n, 3, generator=rng)
        crashes = torch.rand(n, generator=rng) < 0.1
        prev_dist = (target - position).norm(dim=1) + torch.randn(n, generator=rng) * 0.05  # on both sides of dist
        actions = (torch.rand(n, 4, generator=rng) - 0.5) * 6.0
        prev_actions = (torch.rand(n, 4, generator=rng) - 0.5) * 6.0
        pavf = (torch.rand(n, 4, generator=rng) - 0.5) * 6.0
        fake = types.SimpleNamespace(target_position=target, prev_dist=prev_dist, actions=actions, prev_actions=prev_actions,
                                     actions_vehicle_frame=torch.zeros(n, 4), prev_actions_vehicle_frame=pavf, device="cpu",
                                     task_config=types.SimpleNamespace(reward_parameters={}))
        obs_dict = {"robot_position": position, "robot_orientation": q, "robot_vehicle_orientation": qveh, "robot_body_linvel": vbody,
                    "robot_body_angvel": wbody, "crashes": crashes.clone()}
        reward, crashes_out = cls.compute_rewards_and_crashes(fake, obs_dict)
        rec = dict(target=target, position=position, orientation=q, vehicle_orientation=qveh, body_linvel=vbody, body_angvel=wbody,
                   crashes_in=crashes, prev_dist=prev_dist, actions=actions, prev_actions=prev_actions,
                   prev_actions_vehicle_frame=pavf, actions_vehicle_frame=fake.actions_vehicle_frame, reward=reward,
                   crashes_out=crashes_out)
        for k, v in rec.items():
            out[kind + "_" + k] = v.numpy().copy()
        dist = (target - position).norm(dim=1)
        print("sim2real_reward %-12s mean %.3f  inside 0.2 m: %d  beyond 10 m: %d  crashed: %d -> %d  closer: %d of %d" % (
            kind, float(reward.mean()), int((dist < 0.2).sum()), int((dist > 10).sum()), int(crashes.sum()), int(crashes_out.sum()),
            int((dist < prev_dist).sum()), n))
    np.savez(os.path.join(OUT, "sim2real_reward.npz"), **out)


def gen_obs(rng):
    n = 256
    cls = task_class("velocity")
    assert open(task_module("velocity").__file__).read().count("randn_like") == 4
    state = gg.random_state(n, rng, spread=3.0)
    q = state[:, 3:7]
    q[10::2] = unit_quats(n, rng)[10::2]  # any attitude: half of them with w < 0
    q[0] = torch.tensor([0.6, 0.0, 0.8, 0.0])
    q[1] = torch.tensor([-0.6, 0.0, 0.8, -0.0])
    for j, yaw in enumerate((math.pi - 1e-4, -(math.pi - 1e-4), math.pi - 1e-6, -(math.pi - 1e-6), math.pi, -math.pi, 3.0, -3.0)):
        q[2 + j] = torch.tensor([0.0, 0.0, math.sin(yaw / 2), math.cos(yaw / 2)])
    target = (torch.rand(n, 3, generator=rng) - 0.5) * 2.0
    vbody, wbody = torch.randn(n, 3, generator=rng), torch.randn(n, 3, generator=rng)
    actions = (torch.rand(n, 4, generator=rng) - 0.5) * 6.0
    state_in = state.clone()
    fake = types.SimpleNamespace(
        target_position=target, rewards=torch.zeros(n), terminations=torch.zeros(n, dtype=torch.bool), truncations=torch.zeros(n, dtype=torch.bool),
        obs_dict={"robot_position": state[:, 0:3], "robot_orientation": state[:, 3:7], "robot_body_linvel": vbody,
                  "robot_body_angvel": wbody, "robot_actions": actions},
        task_obs={"observations": torch.zeros(n, 17)})
    torch.manual_seed(31)
    cls.process_obs_for_task(fake)
    torch.manual_seed(31)  # the same draws again, in process_obs_for_task's call order (:209-222): euler, position, linvel, angvel
    z = torch.stack([torch.randn_like(target) for _ in range(4)])
    obs_v = fake.task_obs["observations"].clone()
    # the acceleration task's method is the same text: same result on the same inputs and draws
    fake2 = types.SimpleNamespace(**{**vars(fake), "obs_dict": {**fake.obs_dict, "robot_position": state_in[:, 0:3].clone(),
                                                                 "robot_orientation": state_in[:, 3:7].clone()},
                                     "task_obs": {"observations": torch.zeros(n, 17)}})
    torch.manual_seed(31)
    task_class("acceleration").process_obs_for_task(fake2)
    assert torch.equal(fake2.task_obs["observations"], obs_v)
    np.savez(os.path.join(OUT, "sim2real_obs.npz"), state=state_in.numpy(), target=target.numpy(), body_linvel=vbody.numpy(),
             body_angvel=wbody.numpy(), robot_actions=actions.numpy(), z=z.numpy(), obs=obs_v.numpy(),
             orientation_after=state[:, 3:7].numpy().copy())
    print("sim2real_obs: ok  w < 0: %d  rows 0 / 1 after:" % int((state_in[:, 6] < 0).sum()), state[0, 3:7].tolist(), state[1, 3:7].tolist())


N_GLUE, T_GLUE, EPISODE_GLUE = 48, 12, 5


class ScriptedSim:
    """EnvManager stand-in: the tensors the tasks read, advanced from a pre-drawn script."""

    def __init__(self, g):
        N = N_GLUE
        self.num_envs, self.g = N, g
        self.m = ref_shells.ref("utils.math")
        z = torch.zeros
        self.d = {"robot_position": z(N, 3), "robot_orientation": z(N, 4), "robot_vehicle_orientation": z(N, 4),
                  "robot_body_linvel": z(N, 3), "robot_body_angvel": z(N, 3), "robot_actions": z(N, 4),
                  "crashes": z(N, dtype=torch.bool), "truncations": z(N, dtype=torch.bool)}
        self.sim_steps = torch.zeros(N, dtype=torch.int32)
        self.sim_steps[: N // 2] = 2  # two phases of episodes: truncations on different steps
        self.log = []
        self._draw(torch.arange(N))

    def _draw(self, ids):
        g, d, k = self.g, self.d, len(ids)
        far = torch.rand(k, generator=g) < 0.06
        d["robot_position"][ids] = torch.randn(k, 3, generator=g) * torch.where(far, 9.0, 0.8).unsqueeze(1)
        d["robot_orientation"][ids] = unit_quats(k, g)
        d["robot_vehicle_orientation"][ids] = self.m.vehicle_frame_quat_from_quat(d["robot_orientation"][ids])
        d["robot_body_linvel"][ids] = torch.randn(k, 3, generator=g)
        d["robot_body_angvel"][ids] = torch.randn(k, 3, generator=g)

    def get_obs(self):
        return self.d

    def reset(self):
        pass

    def step(self, actions):
        d = self.d
        self.sim_steps += 1
        d["robot_actions"][:] = actions
        self._draw(torch.arange(self.num_envs))
        d["crashes"][:] = torch.rand(self.num_envs, generator=self.g) < 0.04
        self.log.append({k: d[k].clone() for k in ("robot_position", "robot_orientation", "robot_vehicle_orientation", "robot_body_linvel",
                                                   "robot_body_angvel", "crashes")})
        self.log[-1]["sim_steps"] = self.sim_steps.clone()

    def post_reward_calculation_step(self):
        d = self.d
        ids = torch.nonzero(d["crashes"] | d["truncations"]).squeeze(-1)
        if len(ids) > 0:
            self._draw(ids)
            d["robot_actions"][ids] = 0.0
            self.sim_steps[ids] = 0
        mask = torch.zeros(self.num_envs, dtype=torch.uint8)
        mask[ids] = 1
        self.log[-1].update(reset_mask=mask, **{"post_" + k: d[k].clone() for k in ("robot_position", "robot_orientation", "robot_body_linvel",
                                                                                     "robot_body_angvel", "robot_actions")})
        return ids

    def delete_env(self):
        pass


def gen_glue():
    out = {"episode_len_steps": np.int64(EPISODE_GLUE)}
    for kind in KINDS:
        mod = task_module(kind)
        g = torch.Generator().manual_seed(777 if kind == "velocity" else 778)
        sim = ScriptedSim(g)

        class Builder:
            def build_env(self, **kw):
                return sim

        mod.SimBuilder = Builder
        ref_cfg = ref_shells.ref("config.task_config.%s_config" % KINDS[kind][0]).task_config

        class cfg(ref_cfg):
            num_envs = N_GLUE
            device = "cpu"
            headless = True
            episode_len_steps = EPISODE_GLUE

        cfg.reward_parameters = dict(ref_cfg.reward_parameters)
        task = getattr(mod, KINDS[kind][1])(cfg)
        torch.manual_seed(100)
        task.reset()
        rows = {}

        def keep(name, v):
            rows.setdefault(name, []).append(v.clone().numpy())

        buf = torch.zeros(N_GLUE, 4)  # the caller's action buffer: reused and overwritten for the first steps, fresh tensors afterwards
        for t in range(T_GLUE):
            a = (torch.rand(N_GLUE, 4, generator=g) - 0.5) * (6.0 if t % 4 == 3 else 2.0)
            if t < 7:
                buf.copy_(a)
                handed = buf
            else:
                handed = a.clone()
            if t == 6:
                task.target_position[::9, 0] = 11.0  # a moved set-point: distance crashes
            keep("target", task.target_position)
            keep("action_in", handed)
            keep("pre_position", sim.d["robot_position"])
            keep("pre_orientation", sim.d["robot_orientation"])
            torch.manual_seed(1000 + t)
            obs, rewards, terminations, truncations, _ = task.step(handed)
            torch.manual_seed(1000 + t)
            keep("z", torch.stack([torch.randn(N_GLUE, 3) for _ in range(4)]))
            log = sim.log[-1]
            for k, v in log.items():
                keep(k, v)
            for k, v in (("prev_actions", task.prev_actions), ("prev_dist", task.prev_dist), ("action_after", handed),
                         ("rewards", rewards), ("terminations", terminations), ("truncations", truncations),
                         ("observations", obs["observations"]), ("orientation_after", sim.d["robot_orientation"])):
                keep(k, v)
            if kind == "acceleration":
                keep("actions_vehicle_frame", task.actions_vehicle_frame)
                keep("prev_actions_vehicle_frame", task.prev_actions_vehicle_frame)
            assert task.actions is handed
        for k, v in rows.items():
            out[kind + "_" + k] = np.stack(v)
        print("sim2real_glue %-12s resets %d  truncations %d  crashes in / out %d / %d" % (
            kind, int(out[kind + "_reset_mask"].sum()), int(out[kind + "_truncations"].sum()), int(out[kind + "_crashes"].sum()),
            int(out[kind + "_terminations"].sum())))
    np.savez(os.path.join(OUT, "sim2real_glue.npz"), **out)


def gen_config():
    out = {}
    for kind in KINDS:
        c = ref_shells.ref("config.task_config.%s_config" % KINDS[kind][0]).task_config
        out[kind] = np.array(json.dumps({k: getattr(c, k) for k in CONFIG_KEYS}, sort_keys=True))
    np.savez(os.path.join(OUT, "sim2real_config.npz"), **out)
    print("sim2real_config:", {k: str(v) for k, v in out.items()})


def main():
    os.makedirs(OUT, exist_ok=True)
    ref_shells.install()
    ref_shells.install_task_shells()
    rng = torch.Generator().manual_seed(20252)
    gen_reward(rng)
    gen_obs(rng)
    gen_glue()
    gen_config()


if __name__ == "__main__":
    main()
