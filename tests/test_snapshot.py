"""Snapshot / restore / fork, host side (no GPU): the state table of every supported task, the SimSnapshot container, the fingerprint
check, the refusals, and the ABI of the two new entry points.  The device side is tests/test_gpu_snapshot.py."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch
from snapshot_ref import block_rows, make_task, ref_gather, ref_scatter, task_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUPPORTED = ("position_setpoint_task", "navigation_task", "position_setpoint_task_sim2real_end_to_end")
# AgxEnvBuffers members that point at per-env state (the others: scratch outputs, per-step draws, derived collision boxes, the
# exchange of sharded stepping, the device step counter)
PER_ENV_MEMBERS = ("state", "derived", "actions", "prev_actions", "motor_thrust", "motor_kT", "motor_tau_inc", "motor_tau_dec", "gains",
                   "crashes", "truncations", "sim_steps", "reset_mask", "reset_flag", "episode_count", "bounds_min", "bounds_max", "body_force")


def cpu_task(name, n=5, **overrides):
    with task_config(name, "cpu", **overrides):
        return make_task(name, n)


@pytest.mark.parametrize("name", SUPPORTED)
def test_state_table_of_a_supported_task(name):
    from aerial_gym_simulator_amd import _lib

    task = cpu_task(name)
    env = task.sim_env
    T = env.snapshot_table()
    names = [e["name"] for e in T.entries]
    assert len(set(names)) == len(names) and 0 < len(names) <= _lib.SNAPSHOT_MAX_ENTRIES
    assert sum(e["rows"] for e in T.entries) == T.block_rows
    assert [e["block_row"] for e in T.entries] == list(np.cumsum([0] + [e["rows"] for e in T.entries])[:-1])
    for e in T.entries:
        t, n = e["tensor"], env.num_envs
        assert e["elem_size"] == t.element_size() and e["rows"] == (t.numel() if e["layout"] == "global" else t.numel() // n)
    # every per-env pointer the env manager would bind (EnvManager._bind) is in the table, under the member's name
    g, mm = env.global_tensor_dict, env.robot_manager.robot.control_allocator.motor_model
    bound = {"state": g["robot_state_soa"], "derived": g["robot_derived_soa"], "actions": g["robot_actions_soa"],
             "prev_actions": g["robot_prev_actions_soa"], "motor_thrust": mm.thrust_soa, "motor_kT": mm.kT_soa,
             "motor_tau_inc": mm.tau_inc_soa, "motor_tau_dec": mm.tau_dec_soa, "gains": g.get("controller_gains_soa"),
             "crashes": g["crashes"], "truncations": g["truncations"], "sim_steps": g["sim_steps"], "reset_mask": g["reset_mask"],
             "reset_flag": g["reset_flag"], "episode_count": g["episode_count"], "bounds_min": env.bounds_soa[0], "bounds_max": env.bounds_soa[1],
             "body_force": env.robot_manager.imu_sensor.body_force if env.robot_manager.imu_sensor is not None else None}
    assert set(bound) == set(PER_ENV_MEMBERS) <= {f[0] for f in _lib.AgxEnvBuffers._fields_}
    by_name = {e["name"]: e["tensor"] for e in T.entries}
    for member, t in bound.items():
        if t is not None:
            assert by_name[member] is t, member
    # the task's declared tensors and the fingerprint
    assert all(("task." + path) in by_name for path, _ in type(task).SNAPSHOT_TENSORS)
    fp = env.snapshot_fingerprint()
    assert fp["task"] == type(task).__name__ and fp["num_envs"] == 5 and fp["abi_version"] == _lib.ABI_VERSION
    assert fp["layout"] == T.layout() and [row[0] for row in fp["layout"]] == names
    assert env.snapshot_table() is T  # built once


def test_navigation_table_holds_images_and_obstacle_poses():
    task = cpu_task("navigation_task")
    rows = {e["name"]: (e["rows"], e["layout"]) for e in task.sim_env.snapshot_table().entries}
    assert rows["depth_range_pixels"] == (64 * 48, "aos") and rows["env_asset_state_tensor"][1] == "aos"
    assert rows["env_asset_state_tensor"][0] == 13 * task.sim_env.scene.num_assets
    assert rows["task._counters"] == (3, "global") and rows["reset_flag"] == (2, "global")


def hand_filled_snapshot():
    from aerial_gym_simulator_amd.snapshot import SimSnapshot, python_random_state

    layout = [["state", 13, "float32", "soa"], ["crashes", 1, "bool", "soa"], ["reset_flag", 2, "int32", "global"]]
    fp = {"abi_version": 23, "task": "PositionSetpointTask", "robot": "base_quadrotor", "controller": "lee_position_control",
          "env_name": "empty_env", "num_envs": 4, "env_offset": 8, "rng_seed": 2 ** 63 + 5, "layout": layout}
    block = torch.arange(16 * 4, dtype=torch.int32).view(16, 4) - 7
    host = {"env": dict(step_counter=12, flag_parity=1, produced="observation,reward", cpu_rng=torch.get_rng_state(), **python_random_state()),
            "task": {"counter": 12, "flag": True}}
    return SimSnapshot(fp, block, host)


def test_state_dict_round_trip_of_a_hand_filled_snapshot():
    from aerial_gym_simulator_amd.snapshot import SimSnapshot, first_mismatch

    snap = hand_filled_snapshot()
    assert snap.nbytes == 16 * 4 * 4 + sum(v.numel() * v.element_size() for v in snap.host["env"].values() if isinstance(v, torch.Tensor))
    d = snap.state_dict()

    def plain(x):  # CPU tensors, ints, strings (bools and floats among the task's counters), lists and dicts of them
        if isinstance(x, dict):
            return all(isinstance(k, str) and plain(v) for k, v in x.items())
        if isinstance(x, list):
            return all(plain(v) for v in x)
        return (isinstance(x, torch.Tensor) and x.device.type == "cpu") or isinstance(x, (int, str, float))
    assert plain(d)
    buf = io.BytesIO()
    torch.save(d, buf)
    buf.seek(0)
    back = SimSnapshot.from_state_dict(torch.load(buf), "cpu")
    assert first_mismatch(back.fingerprint, snap.fingerprint) is None and back.fingerprint == snap.fingerprint
    assert torch.equal(back.block, snap.block) and back.block.dtype == torch.int32
    assert back.host.keys() == snap.host.keys()
    for part in snap.host:
        assert back.host[part].keys() == snap.host[part].keys()
        for k, v in snap.host[part].items():
            assert torch.equal(back.host[part][k], v) if isinstance(v, torch.Tensor) else back.host[part][k] == v, k
    assert back.nbytes == snap.nbytes
    back.block[0, 0] += 1  # a copy, not an alias
    assert not torch.equal(back.block, snap.block)
    with pytest.raises(ValueError, match="block"):
        SimSnapshot.from_state_dict(dict(d, block=d["block"][:-1]), "cpu")


def test_python_random_state_round_trip():
    import random

    from aerial_gym_simulator_amd.snapshot import python_random_state, set_python_random_state

    random.gauss(0.0, 1.0)  # leaves gauss_next set
    h = python_random_state()
    a = [random.gauss(0.0, 1.0) for _ in range(3)] + [random.random()]
    set_python_random_state(h)
    assert a == [random.gauss(0.0, 1.0) for _ in range(3)] + [random.random()]


FIELDS = {"abi_version": 1, "task": "NavigationTask", "robot": "lmf2", "controller": "lee_velocity_control", "env_name": "env_with_obstacles",
          "num_envs": 6, "env_offset": 3, "rng_seed": 12345}


@pytest.mark.parametrize("field", list(FIELDS) + ["layout_rows", "layout_name", "layout_dtype"])
def test_every_fingerprint_mismatch_raises_and_names_its_field(field):
    from aerial_gym_simulator_amd.snapshot import FINGERPRINT_FIELDS, SimSnapshot

    assert set(FIELDS) | {"layout"} == set(FINGERPRINT_FIELDS)
    task = cpu_task("position_setpoint_task")
    env = task.sim_env
    fp = dict(env.snapshot_fingerprint())
    fp["layout"] = [list(e) for e in fp["layout"]]
    if field.startswith("layout"):
        col = {"layout_name": 0, "layout_rows": 1, "layout_dtype": 2}[field]
        fp["layout"][3][col] = {0: "other", 1: fp["layout"][3][1] + 1, 2: "int32"}[col]
        field = "layout"
    else:
        assert fp[field] != FIELDS[field]
        fp[field] = FIELDS[field]
    snap = SimSnapshot(fp, torch.zeros(sum(e[1] for e in fp["layout"]), fp["num_envs"], dtype=torch.int32), {"env": {}, "task": {}})
    with pytest.raises(ValueError, match=f"'{field}'"):
        task.restore(snap)
    with pytest.raises(ValueError, match=f"'{field}'"):
        env.restore(snap, env_ids=torch.tensor([0]))


def test_first_differing_field_is_the_one_named():
    from aerial_gym_simulator_amd.snapshot import SimSnapshot

    task = cpu_task("position_setpoint_task")
    fp = dict(task.sim_env.snapshot_fingerprint(), robot="x", num_envs=99)
    with pytest.raises(ValueError, match="'robot'"):
        task.restore(SimSnapshot(fp, torch.zeros(1, 99, dtype=torch.int32), {}))


def test_snapshot_on_a_cpu_env_raises_the_hip_device_error():
    from aerial_gym_simulator_amd.snapshot import SimSnapshot

    task = cpu_task("position_setpoint_task")
    env = task.sim_env
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        task.snapshot()
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        env.snapshot()
    T = env.snapshot_table()
    snap = SimSnapshot(env.snapshot_fingerprint(), torch.zeros(T.block_rows, 5, dtype=torch.int32), {"env": {}, "task": {}})
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        task.restore(snap)


def test_refusals_name_their_mode():
    # lean_step
    task = cpu_task("position_setpoint_task", args={"lean_step": True})
    with pytest.raises(RuntimeError, match="lean_step"):
        task.snapshot()
    with pytest.raises(RuntimeError, match="lean_step"):
        task.restore(None)
    # a task stepping by hipGraph replay
    task = cpu_task("navigation_task", args={"step_graph": True})
    with pytest.raises(RuntimeError, match="step_graph"):
        task.snapshot()
    with pytest.raises(RuntimeError, match="step_graph"):
        task.sim_env.snapshot()
    # bound exchange rows / peer push (sharded stepping)
    task = cpu_task("position_setpoint_task")
    task.sim_env._push = dict(rank=0, world=2, slots=4)
    with pytest.raises(RuntimeError, match="exchange rows / peer push"):
        task.snapshot()
    task.sim_env._push = None
    task.sim_env._step_rows = (None, None, None)
    with pytest.raises(RuntimeError, match="exchange rows / peer push"):
        task.restore(None)
    # use_vae = True (the encoder itself needs the device: the switch is enough to refuse)
    task = cpu_task("navigation_task")
    task.vae_model = object()
    with pytest.raises(RuntimeError, match="use_vae"):
        task.snapshot()
    # inside a step
    task = cpu_task("position_setpoint_task_sim2real_end_to_end")
    task.sim_env.post_step_launch = task._launch_post_step
    with pytest.raises(RuntimeError, match="inside a step"):
        task.snapshot()
    task.sim_env.post_step_launch = None
    task.sim_env._in_external_simulate = True
    with pytest.raises(RuntimeError, match="inside a step"):
        task.restore(None)


def test_fork_with_obstacles_is_refused():
    from aerial_gym_simulator_amd.snapshot import SimSnapshot

    task = cpu_task("navigation_task")
    env = task.sim_env
    assert env.scene.num_assets > 0
    snap = SimSnapshot(env.snapshot_fingerprint(), torch.zeros(env.snapshot_table().block_rows, 5, dtype=torch.int32), {"env": {}, "task": {}})
    with pytest.raises(ValueError, match="num_assets == 0"):
        task.restore(snap, from_env_ids=0)
    with pytest.raises(ValueError, match="static per env"):
        task.restore(snap, env_ids=torch.tensor([1, 2]), from_env_ids=torch.tensor([0, 0]))


@pytest.mark.parametrize("ids", [[5], [-1], [0, 7], torch.tensor([2, 2]), torch.tensor([1, 1, 3]), torch.tensor([0.0, 1.0])])
def test_index_env_ids_are_checked_before_they_index(ids):
    """out of [0, N), repeated, or no integers: ValueError on the host, before any tensor is indexed with them"""
    from aerial_gym_simulator_amd.snapshot import SimSnapshot

    task = cpu_task("position_setpoint_task")
    env = task.sim_env
    snap = SimSnapshot(env.snapshot_fingerprint(), torch.zeros(env.snapshot_table().block_rows, 5, dtype=torch.int32), {"env": {}, "task": {}})
    with pytest.raises(ValueError, match="env_ids"):
        task.restore(snap, env_ids=ids)
    with pytest.raises(ValueError, match="env_ids"):
        task.restore(snap, env_ids=ids, from_env_ids=0)
    with pytest.raises(ValueError, match="mask has shape"):
        task.restore(snap, env_ids=torch.ones(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="from_env_ids"):
        task.restore(snap, env_ids=[0, 1], from_env_ids=torch.tensor([0, 1, 2]))


def test_every_registered_task_is_supported_or_refuses_by_name():
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    names = sorted(task_registry.get_task_names())
    assert len(names) >= 8
    seen_supported = set()
    for name in names:
        task = cpu_task(name, n=3)
        cls = type(task).__name__
        if type(task).__dict__.get("SNAPSHOT_TENSORS") is not None:
            seen_supported.add(name)
            task.sim_env.snapshot_table()
            continue
        for call in (task.snapshot, task.sim_env.snapshot, lambda: task.restore(None)):
            with pytest.raises(NotImplementedError, match=cls):
                call()
    assert set(SUPPORTED) <= seen_supported


def test_header_lib_and_exported_symbols_agree_on_the_new_entry_points():
    from aerial_gym_simulator_amd import _lib

    header = open(os.path.join(ROOT, "include", "aerial_gym_hip.h")).read()
    for name in ("agx_state_gather", "agx_state_scatter"):
        assert re.search(r"\bint %s\(const AgxSnapshotTable \*table, int num_envs," % name, header)
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name)
    assert int(re.search(r"#define AGX_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 23
    assert int(re.search(r"#define AGX_SNAPSHOT_MAX_ENTRIES (\d+)", header).group(1)) == _lib.SNAPSHOT_MAX_ENTRIES
    assert re.search(r"enum \{ AGX_SNAP_SOA = 0, AGX_SNAP_AOS = 1, AGX_SNAP_GLOBAL = 2 \}", header)
    assert (_lib.SNAP_SOA, _lib.SNAP_AOS, _lib.SNAP_GLOBAL) == (0, 1, 2)


def test_table_struct_layout_matches_the_header(tmp_path):
    """sizeof and member offsets of the ctypes mirrors == the C compiler's, from the header"""
    import shutil
    import subprocess

    from aerial_gym_simulator_amd import _build, _lib

    gcc = shutil.which("gcc") or shutil.which("cc")
    # (without a system C compiler: the compiler the library itself is built with, on the host side alone; none at all is an error)
    cc = [gcc] if gcc else [_build._hipcc(), "-x", "c++"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "aerial_gym_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
           "sizeof(AgxSnapshotEntry), sizeof(AgxSnapshotTable), offsetof(AgxSnapshotEntry, rows), offsetof(AgxSnapshotEntry, layout), "
           "offsetof(AgxSnapshotTable, block_rows), offsetof(AgxSnapshotTable, error), offsetof(AgxSnapshotTable, entry));return 0;}")
    c, exe = tmp_path / "t.c", str(tmp_path / "t")
    c.write_text(src)
    subprocess.run(cc + ["-I", os.path.join(ROOT, "include"), str(c), "-o", exe], check=True)
    sizes = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    E, T = _lib.AgxSnapshotEntry, _lib.AgxSnapshotTable
    assert sizes == [ctypes.sizeof(E), ctypes.sizeof(T), E.rows.offset, E.layout.offset, T.block_rows.offset, T.error.offset, T.entry.offset]


def test_host_side_argument_checks_need_no_device():
    """AGX_REQUIRE: null table, n <= 0, capacity, null pointers, inconsistent rows -- refused before anything is launched"""
    from aerial_gym_simulator_amd import _lib

    lib = _lib.load()
    T = _lib.AgxSnapshotTable()
    blk = ctypes.c_void_p(4096)

    def both(table, n, expect):
        for rc in (lib.agx_state_gather(table, n, blk, None), lib.agx_state_scatter(table, n, blk, None, None, None)):
            assert rc == -1 and expect in lib.agx_last_error().decode(), lib.agx_last_error()

    both(None, 4, "null table")
    T.count = 0
    both(T, 4, "table entries")
    T.count = _lib.SNAPSHOT_MAX_ENTRIES + 1
    both(T, 4, "table entries")
    T.count, T.block_rows = 1, 3
    both(T, 0, "num_envs must be > 0")
    both(T, 4, "null pointer")
    T.entry[0].ptr, T.entry[0].rows, T.entry[0].elem_size = 4096, 3, 2
    both(T, 4, "element size")
    T.entry[0].elem_size, T.entry[0].layout = 4, 3
    both(T, 4, "layout")
    T.entry[0].layout, T.entry[0].block_row = 0, 1
    both(T, 4, "block row")
    T.entry[0].block_row, T.block_rows = 0, 4
    both(T, 4, "block_rows")
    T.block_rows, T.entry[0].rows = 1 << 30, 1 << 30
    both(T, 4, "2^31")
    T.block_rows, T.entry[0].rows = 3, 3
    assert lib.agx_state_gather(T, 4, None, None) == -1 and lib.agx_state_scatter(T, 4, None, None, None, None) == -1
    src = ctypes.c_void_p(8192)
    assert lib.agx_state_scatter(T, 4, blk, src, None, None) == -1 and "table->error" in lib.agx_last_error().decode()


def test_restatement_round_trips_and_forks():
    """the numpy restatement the GPU tests compare the kernels against, on its own: gather then scatter is the identity, a fork
    copies rows, a mask leaves the other envs and the global words alone"""
    rng = np.random.default_rng(3)
    n = 7
    live = [(rng.integers(0, 2 ** 32, (3, n), dtype=np.uint32), "soa"), (rng.integers(0, 256, (n, 2), dtype=np.uint8), "aos"),
            (rng.integers(0, 2 ** 32, (n, 5), dtype=np.uint32), "aos"), (rng.integers(0, 2 ** 32, (2,), dtype=np.uint32), "global")]
    rows = block_rows(live, n)
    assert rows == 3 + 2 + 5 + 2
    block = ref_gather(live, n, np.full((rows, n), 0xDEADBEEF, np.uint32))
    assert (block[-2:].reshape(-1)[2:] == 0xDEADBEEF).all() and block[3:5].max() < 256
    zero = [(np.zeros_like(a), lay) for a, lay in live]
    back = ref_scatter(zero, n, block)
    assert all(np.array_equal(a, b[0]) for a, b in zip(back, live))
    fork = ref_scatter(zero, n, block, src=np.zeros(n, np.int64))
    assert (fork[0] == live[0][0][:, :1]).all() and (fork[2] == live[2][0][:1]).all() and np.array_equal(fork[3], live[3][0])
    mask = np.arange(n) % 3 == 0
    part = ref_scatter(zero, n, block, mask=mask)
    assert np.array_equal(part[0][:, mask], live[0][0][:, mask]) and not part[0][:, ~mask].any() and not part[3].any()
    assert np.array_equal(part[1][mask], live[1][0][mask]) and not part[1][~mask].any()
