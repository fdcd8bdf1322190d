"""GPU: k_position_step_fused<AGX_STEP_ANY> with its helper wave (csrc/agx_dyn_position_step.h) against the two
launches it replaces.

In an ANY launch the step wave of a workgroup integrates its 16 envs while the helper wave evaluates the draws and the new state
of the envs that truncate; behind one barrier the helper resets those and the envs that crashed, refreshes every env's derived
tensors and writes the observation.  A task with args={"single_launch_step": False} always issues the two launches; its twin,
same seed and actions, issues ANY launches whenever a witness env truncates.  Every buffer the step touches is compared bit for
bit after every step, and the device's violation word stays 0."""
import pytest
import torch

from aerial_gym_simulator_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ANY = _lib.STEP_MODES.index("any")


@pytest.fixture(autouse=True)
def _restore():
    """the config classes this file changes"""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config.controller_config import lee_controller_config as ctrl
    from aerial_gym_simulator_amd.config.robot_config import BaseQuadCfg
    from aerial_gym_simulator_amd.config.task_config import position_setpoint_task_config as cfg

    mm = BaseQuadCfg.control_allocator_config.motor_model_config
    names = ("motor_time_constant_increasing_min", "motor_time_constant_increasing_max", "motor_time_constant_decreasing_min",
             "motor_time_constant_decreasing_max")
    old = (cfg.device, cfg.controller_name, cfg.episode_len_steps, cfg.args, ctrl.randomize_params, [getattr(mm, k) for k in names])
    yield
    cfg.device, cfg.controller_name, cfg.episode_len_steps, cfg.args, ctrl.randomize_params = old[:5]
    for k, v in zip(names, old[5]):
        setattr(mm, k, v)
    _lib.set_option("single_launch_step", 1)


def _make(n, L, single, randomised=False, seed=5):
    from aerial_gym_simulator_amd.config.controller_config import lee_controller_config as ctrl
    from aerial_gym_simulator_amd.config.robot_config import BaseQuadCfg
    from aerial_gym_simulator_amd.config.task_config import position_setpoint_task_config as cfg
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    cfg.device, cfg.controller_name, cfg.episode_len_steps = DEV, "lee_position_control", L
    cfg.args = {"rng_seed": 1234, "single_launch_step": single}
    if randomised:  # gains re-drawn at every reset, per-env motor time constants drawn from a real interval (kT always is)
        ctrl.randomize_params = True
        mm = BaseQuadCfg.control_allocator_config.motor_model_config
        mm.motor_time_constant_increasing_min, mm.motor_time_constant_increasing_max = 0.01, 0.03
        mm.motor_time_constant_decreasing_min, mm.motor_time_constant_decreasing_max = 0.02, 0.05
    task = task_registry.make_task("position_setpoint_task", seed=seed, num_envs=n, headless=True)
    if randomised:
        B = task.sim_env._buffers
        assert B.gains and B.motor_tau_inc and B.motor_tau_dec and B.motor_kT
    return task


def _tensors(task):
    env = task.sim_env
    g = env.global_tensor_dict
    mm = env.robot_manager.robot.control_allocator.motor_model
    return {"obs": task.task_obs["observations"], "reward": task.rewards, "crashes": g["crashes"], "truncations": g["truncations"],
            "state": g["robot_state_soa"], "derived": g["robot_derived_soa"], "thrust": mm.thrust_soa, "tau_inc": mm.tau_inc_soa,
            "tau_dec": mm.tau_dec_soa, "kT": mm.kT_soa, "gains": g["controller_gains_soa"], "actions": g["robot_actions_soa"],
            "prev_actions": g["robot_prev_actions_soa"], "sim_steps": g["sim_steps"], "episode_count": g["episode_count"],
            "bounds_min": env.bounds_soa[0], "bounds_max": env.bounds_soa[1], "reset_mask": g["reset_mask"],
            "reset_flag": g["reset_flag"]}


def _assert_same(a, b, t):
    ta, tb = _tensors(a), _tensors(b)
    for k in ta:
        assert torch.equal(ta[k], tb[k]), (t, k)


class _Pair:
    """the two-launch task and its single-launch twin, stepped together and compared after every step"""

    def __init__(self, n, L, randomised=False):
        self.n, self.t = n, 0
        self.plain, self.fused = _make(n, L, False, randomised), _make(n, L, True, randomised)
        self.g = torch.Generator(device=DEV).manual_seed(7)
        for task in self.both:
            task.reset()
        self.any_steps = 0      # steps that ran as one AGX_STEP_ANY launch
        self.any_with = {"truncation": 0, "crash": 0, "both_in_one_wave": 0, "more_than_8_in_one_wave": 0}
        _assert_same(self.plain, self.fused, -1)

    @property
    def both(self):
        return (self.plain, self.fused)

    def step(self, scale=1.0):
        a = (torch.rand(self.n, 4, device=DEV, generator=self.g) * 2 - 1) * scale
        for task in self.both:
            task.step(a)
        torch.cuda.synchronize()
        _assert_same(self.plain, self.fused, self.t)
        self.t += 1
        if int(self.fused._plan.last_mode) == ANY:
            self.any_steps += 1
            g = self.fused.sim_env.global_tensor_dict
            tr, cr = g["truncations"].clone(), g["crashes"].clone()
            pad = (-self.n) % 16
            w = lambda x: torch.nn.functional.pad(x, (0, pad)).view(-1, 16)  # noqa: E731  (one row per wave: 16 envs)
            self.any_with["truncation"] += int(tr.any())
            self.any_with["crash"] += int(cr.any())
            self.any_with["both_in_one_wave"] += int((w(tr & ~cr).any(1) & w(cr & ~tr).any(1)).any())
            self.any_with["more_than_8_in_one_wave"] += int(((w(tr | cr)).sum(1) > 8).any())

    def set_sim_steps(self, values):
        for task in self.both:
            task.sim_env.sim_steps.copy_(values)

    def no_violation(self):
        assert self.fused.single_launch_stats()["violations"] == 0
        m = self.plain.single_launch_stats()["modes"]
        assert m["any"] == m["none"] == 0


def _desync(n, L, seed=9):
    return torch.randint(0, L, (n,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed), dtype=torch.int32)


@pytest.mark.parametrize("n", [333, 8192])
def test_one_env_of_a_block_truncates(n):
    """every episode counter far from the end but one env per chosen block: ANY launches in which exactly those envs reset"""
    L = 40
    P = _Pair(n, L)
    steps = torch.zeros(n, dtype=torch.int32, device=DEV)
    chosen = list(range(5, n, 37))  # at most one env of a block; env number k truncates in step 4 + k % 12 from here
    for k, env in enumerate(chosen):
        steps[env] = L - 3 - (k % 12)
    P.set_sim_steps(steps)
    for _ in range(20):
        P.step()
    # (the step that follows the host's write is two launches by design; the first truncation comes three steps later)
    assert P.any_with["truncation"] == min(len(chosen), 12), (P.any_steps, P.any_with)
    P.no_violation()


@pytest.mark.parametrize("n", [333, 8192])
def test_truncation_and_crash_in_the_same_wave(n):
    """desynchronised episodes (a truncation witness in every step: every step behind the first is an ANY launch); some envs
    are teleported beyond 8 m from their target (the step that follows a teleport is two launches by design: the host touched
    the state), others to just inside 8 m flying outward: those cross the crash radius on their own, inside an ANY launch,
    next to envs of the same wave that truncate -- the helper wave evaluates those before the barrier and the crashed ones
    behind it."""
    L = 12
    P = _Pair(n, L)
    P.set_sim_steps(_desync(n, L))
    for _ in range(4):
        P.step()
    far = torch.arange(3, n, 16, device=DEV)   # one env in every wave
    near = torch.arange(9, n, 16, device=DEV)  # another one in every wave
    for rnd in range(6):
        for task in P.both:
            g = task.sim_env.global_tensor_dict
            if rnd % 2 == 0:
                g["robot_position"][near] = task.target_position[near] + torch.tensor([7.9, 0.0, 0.0], device=DEV)
                g["robot_linvel"][near] = torch.tensor([4.0, 0.0, 0.0], device=DEV)
            else:
                g["robot_position"][far] = task.target_position[far] + torch.tensor([0.0, 9.0, 0.0], device=DEV)
        for _ in range(7):
            P.step()
    assert P.any_steps >= 30, (P.any_steps, P.any_with)
    assert P.any_with["crash"] >= 1 and P.any_with["both_in_one_wave"] >= 1, P.any_with
    P.no_violation()


@pytest.mark.parametrize("n", [333, 8192])
def test_more_than_eight_resets_in_a_wave(n):
    """short episodes, and whole waves whose envs truncate together: the per-lane draw path of wave_reset_draws"""
    L = 9
    P = _Pair(n, L)
    steps = _desync(n, L)
    steps[32:48] = L - 2     # a whole wave
    steps[160:171] = L - 4   # 11 envs of one wave
    P.set_sim_steps(steps)
    for _ in range(3 * L):
        P.step()
    assert P.any_with["more_than_8_in_one_wave"] >= 2, (P.any_steps, P.any_with)
    P.no_violation()


@pytest.mark.parametrize("n", [333, 8192])
def test_randomised_gains_and_motor_constants(n):
    """per-env controller gains and motor constants: the reset draws and stores them too, the step wave loads them at its top"""
    L = 14
    P = _Pair(n, L, randomised=True)
    P.set_sim_steps(_desync(n, L))
    for _ in range(3 * L):
        P.step(scale=3.0)
    assert P.any_steps >= 2 * L, (P.any_steps, P.any_with)
    gains = P.fused.sim_env.global_tensor_dict["controller_gains_soa"]
    assert float(gains[0].std()) > 0  # (they were drawn per env)
    P.no_violation()


def test_episode_length_changed_by_the_host_between_steps():
    """the helper wave evaluates the truncation predicate itself, from the same episode length as the step wave"""
    n, L = 333, 20
    P = _Pair(n, L)
    P.set_sim_steps(_desync(n, L))
    now = L
    for t in range(90):
        if t % 15 == 7:  # a shorter episode makes every env beyond it truncate together, a longer one leaves steps without any
            now = L - 6 if (t // 15) % 2 == 0 else L + 3
            for task in P.both:
                task.task_config.episode_len_steps = now
        elif t % 15 == 12:  # spread the episodes again: a witness in every step
            P.set_sim_steps(_desync(n, now, seed=t))
        P.step()
    # the nine steps between a spread and the next change are ANY launches (five such windows in 90 steps), and so are the
    # first six
    assert P.any_steps >= 45, (P.any_steps, P.any_with)
    P.no_violation()
