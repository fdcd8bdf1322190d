"""Snapshot / restore / fork on the device.  The two kernels against their numpy restatement (tests/snapshot_ref.py); continuation,
masked restore and fork of running tasks against the UNINTERRUPTED run of the unchanged step path.  Every comparison is on the raw
bits (NaNs included); nothing here has a tolerance."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from snapshot_ref import SENTINEL, assert_same_record, block_rows, make_task, raw_bits, record, ref_gather, ref_scatter, task_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the kernels vs the restatement ----------------------------------------------------------------------------------------------
def kernel_case(n, seed):
    """live tensors (torch, on the device) + their numpy twins: 4-byte SoA entries of 1, 3 and 13 rows, one AoS entry, two 1-byte
    entries (SoA bool, AoS uint8), a 64 x 48 image (3072 rows), a global entry, and a 3-row SoA entry whose pointer is only 4-byte
    aligned (the word-by-word path of the identity copy)"""
    rng = np.random.default_rng(seed)
    words = lambda *shape: rng.integers(0, 2 ** 32, shape, dtype=np.uint32)  # noqa: E731  (every bit pattern: NaNs, denormals)
    spec = [("one", words(n), "soa", torch.float32), ("three", words(3, n), "soa", torch.float32), ("thirteen", words(13, n), "soa", torch.float32),
            ("aos", words(n, 5), "aos", torch.int32), ("flags", rng.integers(0, 2, n).astype(np.uint8), "soa", torch.bool),
            ("bytes", rng.integers(0, 256, (n, 3), dtype=np.uint8), "aos", torch.uint8), ("image", words(n, 1, 48, 64), "aos", torch.float32),
            ("global", words(2), "global", torch.int32), ("unaligned", words(3, n), "soa", torch.float32)]
    tensors, arrays = [], []
    for name, a, layout, dtype in spec:
        if a.dtype == np.uint8:
            t = torch.from_numpy(a.copy()).to(DEV)
            t = t.to(torch.bool) if dtype is torch.bool else t
        else:
            t = torch.from_numpy(a.view(np.int32).copy()).to(DEV)
            if name == "unaligned":
                base = torch.zeros(a.size + 4, dtype=torch.int32, device=DEV)
                t = base[1:1 + a.size].view(a.shape).copy_(t)
                assert t.data_ptr() % 16 == 4 and t.is_contiguous()
            t = t.view(dtype)
        tensors.append((name, t, layout))
        arrays.append((a, layout))
    return tensors, arrays


def c_table(tensors, n):
    from aerial_gym_simulator_amd.snapshot import StateTable

    T = StateTable(n)
    for name, t, layout in tensors:
        T.add(name, t, layout)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    return T, T.c_table(err), err


def live_bits(tensors):
    return [raw_bits(t) for _, t, _ in tensors]


def fill(tensors, arrays):
    for (_, t, _), (a, _) in zip(tensors, arrays):
        src = torch.from_numpy(a.copy() if a.dtype == np.uint8 else a.view(np.int32).copy()).to(DEV)
        (t.view(torch.uint8) if a.dtype == np.uint8 else t.view(torch.int32)).copy_(src.view(t.shape))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_gather_and_scatter_vs_the_restatement(n):
    from aerial_gym_simulator_amd import _lib

    lib, stream = _lib.load(), _lib.current_stream(DEV)
    tensors, arrays = kernel_case(n, seed=n)
    T, table, err = c_table(tensors, n)
    rows = block_rows(arrays, n)
    assert T.block_rows == rows == 1 + 3 + 13 + 5 + 1 + 3 + 3072 + 2 + 3
    # gather: every word of the block, the unused ones (the global entry's tail) included
    block = torch.full((rows, n), SENTINEL - 2 ** 32, dtype=torch.int32, device=DEV)
    _lib.check(lib.agx_state_gather(table, n, _lib.dptr(block), stream), "agx_state_gather")
    want = ref_gather(arrays, n, np.full((rows, n), SENTINEL, np.uint32))
    assert np.array_equal(raw_bits(block), want)
    assert all(np.array_equal(x.reshape(-1), a.reshape(-1)) for x, (a, _) in zip(live_bits(tensors), arrays))  # the live side is read only
    # scatter: another block, live tensors pre-filled with a sentinel; every mask x every source index
    rng = np.random.default_rng(1000 + n)
    blk = rng.integers(0, 2 ** 32, (rows, n), dtype=np.uint32)
    row = 0
    for a, layout in arrays:  # (byte entries hold bytes: what a gather can have put there)
        r = a.size if layout == "global" else a.size // n
        if a.dtype == np.uint8:
            blk[row:row + r] &= 1 if r == 1 else 255  # (the one-row byte entry is the bool one)
        row += r
    block.copy_(torch.from_numpy(blk.view(np.int32)).to(DEV))
    # what the live tensors hold before a scatter; the bool entry can only hold 0 or 1, so every combination runs with both
    sentinels = [[(np.full_like(a, flag_fill) if name == "flags" else np.full_like(a, 0xA5 if a.dtype == np.uint8 else 0xA5A5A5A5), lay)
                  for (name, _, _), (a, lay) in zip(tensors, arrays)] for flag_fill in (0, 1)]
    masks = {"none": None, "all": np.ones(n, np.uint8), "alternating": (np.arange(n) % 2).astype(np.uint8),
             "last": (np.arange(n) == n - 1).astype(np.uint8)}
    sources = {"identity": None, "reversed": np.arange(n - 1, -1, -1, dtype=np.int32), "zero": np.zeros(n, np.int32)}
    for mname, m in masks.items():
        for sname, s in sources.items():
            for flag_fill, sentinel in enumerate(sentinels):
                fill(tensors, sentinel)
                md = torch.from_numpy(m).to(DEV) if m is not None else None
                sd = torch.from_numpy(s).to(DEV) if s is not None else None
                _lib.check(lib.agx_state_scatter(table, n, _lib.dptr(block), _lib.dptr(sd), _lib.dptr(md), stream), "agx_state_scatter")
                want = ref_scatter(sentinel, n, blk, src=s, mask=m)
                for (name, _, _), got, w in zip(tensors, live_bits(tensors), want):
                    assert np.array_equal(got.reshape(-1), w.reshape(-1)), (n, mname, sname, name, flag_fill)
                assert int(err.item()) == 0
    assert np.array_equal(raw_bits(block), blk)  # the block is read only


@pytest.mark.parametrize("bad", ["n", "minus_one", "large"])
def test_out_of_range_source_index_returns_the_error_code_and_writes_nothing(bad):
    from aerial_gym_simulator_amd import _lib

    n = 65
    lib, stream = _lib.load(), _lib.current_stream(DEV)
    tensors, arrays = kernel_case(n, seed=7)
    _T, table, err = c_table(tensors, n)
    rows = block_rows(arrays, n)
    block = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (rows, n)).astype(np.int32)).to(DEV)
    src = np.arange(n, dtype=np.int32)
    src[n - 1 if bad == "n" else 17] = {"n": n, "minus_one": -1, "large": 2 ** 31 - 1}[bad]
    before = live_bits(tensors)
    rc = lib.agx_state_scatter(table, n, _lib.dptr(block), _lib.dptr(torch.from_numpy(src).to(DEV)), None, stream)
    assert rc == -1 and "src_index" in lib.agx_last_error().decode()  # AGX_E_ARG
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(before, live_bits(tensors)))
    assert int(err.item()) == 0  # cleared: the next call starts clean
    ok = torch.zeros(n, dtype=torch.int32, device=DEV)
    _lib.check(lib.agx_state_scatter(table, n, _lib.dptr(block), _lib.dptr(ok), None, stream), "agx_state_scatter")
    with pytest.raises(RuntimeError, match="src_index"):  # ... and through the public interface
        with task_config("position_setpoint_task", DEV, args={"rng_seed": 3}):
            task = make_task("position_setpoint_task", 16)
        task.reset()
        task.restore(task.snapshot(), from_env_ids=torch.tensor([16] + [0] * 15))


# ---- continuation ----------------------------------------------------------------------------------------------------------------
CASES = {
    # name: (task, config overrides, action width)
    "position": ("position_setpoint_task", dict(episode_len_steps=5), 4),
    "position_single_launch": ("position_setpoint_task", dict(episode_len_steps=5, controller_name="lee_position_control"), 4),
    "navigation": ("navigation_task", dict(episode_len_steps=7, env_name="env_with_obstacles"), 4),
    "end_to_end": ("position_setpoint_task_sim2real_end_to_end", dict(episode_len_steps=6), 4),
    # NavigationTask as registered a second time: the octarotor (8 motors, 7-D fully actuated commands, disturbances on) with the
    # 32 x 512 LiDAR; the policy's action is 4 wide, the task's transformation makes the 7-D command of it
    "navigation_fully_actuated_lidar": ("navigation_task_fully_actuated_lidar", dict(episode_len_steps=7, env_name="env_with_obstacles"), 4),
}
RUNS = [(case, 67) for case in CASES] + [("position", 16), ("position", 17), ("position_single_launch", 16), ("position_single_launch", 17)]


def scripted_actions(n, width, steps, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, width, generator=g) * 2.0 - 1.0).to(DEV) for _ in range(steps)]


def run(task, actions):
    return [record(task, task.step(a.clone())) for a in actions]  # (a fresh tensor per step: the position task keeps the caller's)


@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict_rng"])
@pytest.mark.parametrize("case,n", RUNS, ids=[f"{c}-{n}" for c, n in RUNS])
def test_continuation_is_bit_exact_in_place_and_on_a_fresh_object(case, n, strict):
    """12 scripted steps, snapshot, 9 recorded steps, restore, the same 9 actions: every output of every step equal.  Then once more on
    a fresh task object built from the same configs and loaded through state_dict -> torch.save -> torch.load."""
    from aerial_gym_simulator_amd.snapshot import SimSnapshot

    name, overrides, width = CASES[case]
    args = {"strict_rng": strict, "rng_seed": 20240 + n}
    acts = scripted_actions(n, width, 21)
    with task_config(name, DEV, args=args, **overrides):
        task = make_task(name, n)
        env = task.sim_env
        if case.startswith("navigation"):
            px = env.global_tensor_dict["depth_range_pixels"]
            assert env.scene.num_assets > 0 and tuple(px.shape) == ((n, 1, 48, 64) if case == "navigation" else (n, 1, 32, 512))
            assert env.num_robot_actions == (4 if case == "navigation" else 7)
        task.reset()
        before = run(task, acts[:12])
        snap = task.snapshot()
        assert snap.block.is_cuda and snap.nbytes >= snap.block.numel() * 4
        first = run(task, acts[12:])
        resets = [int(r["dict.reset_mask"].sum()) for r in before + first]
        assert any(resets[:12]) and any(resets[12:]), resets  # resets on both sides of the snapshot
        assert not torch.equal(first[-1]["dict.robot_state_soa"], before[-1]["dict.robot_state_soa"])
        task.restore(snap)
        again = run(task, acts[12:])
        for j, (a, b) in enumerate(zip(first, again)):
            assert_same_record(a, b, f"{case}, {n} envs, in place, step {j} after the restore")
        if case == "position_single_launch" and not strict:
            stats = task.single_launch_stats()
            assert stats["violations"] == 0 and stats["modes"]["any"] + stats["modes"]["none"] > 0, stats  # the proof path did run
        # the same on a fresh object, through a file
        buf = io.BytesIO()
        torch.save(snap.state_dict(), buf)
        buf.seek(0)
        loaded = SimSnapshot.from_state_dict(torch.load(buf), DEV)
        assert loaded.nbytes == snap.nbytes
        task.close()
        fresh = make_task(name, n)
        fresh.restore(loaded)
        third = run(fresh, acts[12:])
        for j, (a, b) in enumerate(zip(first, third)):
            assert_same_record(a, b, f"{case}, {n} envs, fresh object, step {j} after the restore")
        fresh.close()


def test_snapshot_is_one_launch_without_host_synchronisation_and_reuses_out():
    from task_test_util import no_host_sync

    with task_config("navigation_task", DEV, args={"rng_seed": 9}, env_name="env_with_obstacles"):
        task = make_task("navigation_task", 16)
    task.reset()
    task.step(torch.zeros(16, 4, device=DEV))
    snap = task.snapshot()
    ptr = snap.block.data_ptr()
    task.step(torch.zeros(16, 4, device=DEV))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    calls, real = [], task.sim_env._lib

    class Counting:  # every library call the snapshot makes, by name
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith("agx_"):
                return fn
            return lambda *a: (calls.append(name), fn(*a))[1]

    task.sim_env._lib = Counting()
    try:
        with no_host_sync():
            again = task.snapshot(out=snap)
    finally:
        task.sim_env._lib = real
    assert calls == ["agx_state_gather"], calls  # the library's one launch: the rest of snapshot() is host bookkeeping on CPU tensors
    assert again is snap and snap.block.data_ptr() == ptr and torch.cuda.memory_allocated() == before
    assert snap.host["env"]["step_counter"] == 2
    # every per-env pointer the env manager bound is in the table (tests/test_snapshot.py checks the names on the CPU)
    from test_snapshot import PER_ENV_MEMBERS

    B, table = task.sim_env._buffers, task.sim_env.snapshot_table().c_table(task.sim_env._snap_error)
    held = {table.entry[j].ptr for j in range(table.count)}
    for member in PER_ENV_MEMBERS:
        assert not getattr(B, member) or getattr(B, member) in held, member
    with task_config("position_setpoint_task", DEV, args={"rng_seed": 9}):
        other = make_task("position_setpoint_task", 16)
    with pytest.raises(ValueError, match="out="):
        other.snapshot(out=snap)
    other.close()
    task.close()


# ---- masked restore --------------------------------------------------------------------------------------------------------------
def quiet_position_task(n, args):
    """the position task with the position controller, disturbance off, an episode longer than the test: no reset, no draw"""
    with task_config("position_setpoint_task", DEV, args=dict(args, rng_seed=77), controller_name="lee_position_control", episode_len_steps=500):
        task = make_task("position_setpoint_task", n)
    assert not task.sim_env.robot_manager.robot.cfg.disturbance.enable_disturbance
    return task


def test_masked_restore_touches_only_its_envs():
    n = 65
    acts = scripted_actions(n, 4, 30, seed=5)
    acts = [0.2 * a for a in acts]
    mask = (torch.arange(n) % 3 == 0).to(DEV)
    keep = (~mask).cpu().numpy()
    took = mask.cpu().numpy()
    whole = quiet_position_task(n, {})
    whole.reset()
    straight = run(whole, acts)  # the uninterrupted run
    assert not any(int(r["dict.reset_mask"].sum()) for r in straight)
    whole.close()
    task = quiet_position_task(n, {})
    task.reset()
    run(task, acts[:12])
    snap = task.snapshot()
    run(task, acts[12:21])
    task.restore(snap, env_ids=mask)
    now = record(task, (task.task_obs, task.rewards, task.terminations, task.truncations, {}))
    assert_same_record(now, straight[20], "unmasked envs at the restore", rows=keep)
    assert_same_record(now, straight[11], "masked envs at the restore: their snapshot rows", rows=took)
    assert task.sim_env.step_counter == 21  # global quantities are not restored by a masked call
    for j in range(9):
        a = torch.where(mask.unsqueeze(1), acts[12 + j], acts[21 + j])
        r = record(task, task.step(a))
        assert_same_record(r, straight[21 + j], f"unmasked envs, step {j} after the masked restore", rows=keep)
        assert_same_record(r, straight[12 + j], f"masked envs, step {j} after the masked restore", rows=took)
    # the index form selects the same envs
    task.restore(snap, env_ids=mask.nonzero().squeeze(1))
    assert_same_record(record(task, (task.task_obs, task.rewards, task.terminations, task.truncations, {})), straight[11], "index form", rows=took)
    task.close()


# ---- fork --------------------------------------------------------------------------------------------------------------------------
def test_fork_copies_env_zero_into_every_env():
    n = 65
    task = quiet_position_task(n, {"per_env_gains": True, "per_env_motor_constants": True})
    env = task.sim_env
    assert env.scene.num_assets == 0 and env._buffers.gains and env._buffers.motor_tau_inc
    task.reset()
    run(task, [0.2 * a for a in scripted_actions(n, 4, 6, seed=8)])
    env.global_tensor_dict["controller_gains_soa"].mul_(torch.linspace(0.9, 1.1, n, device=DEV))  # per-env gains that differ
    snap = task.snapshot()
    table = env.snapshot_table()
    spread = {e["name"]: raw_bits(e["tensor"]) for e in table.entries}
    for name in ("state", "motor_kT", "gains"):  # the envs do differ before the fork
        x = spread[name].reshape(-1, n)
        assert (x != x[:, :1]).any(), name
    task.restore(snap, from_env_ids=0)
    for e in table.entries:
        got, was = raw_bits(e["tensor"]), spread[e["name"]]
        if e["layout"] == "soa":
            assert np.array_equal(got.reshape(-1, n), np.repeat(was.reshape(-1, n)[:, :1], n, axis=1)), e["name"]
        elif e["layout"] == "aos":
            assert np.array_equal(got.reshape(n, -1), np.repeat(was.reshape(n, -1)[:1], n, axis=0)), e["name"]
        else:
            assert np.array_equal(got, was), e["name"]
    same = torch.tensor([0.1, -0.2, 0.15, 0.05], device=DEV).expand(n, 4).contiguous()
    for j in range(5):
        r = record(task, task.step(same.clone()))
        assert int(r["dict.reset_mask"].sum()) == 0
        for name in ("obs", "rewards", "dict.robot_state_soa", "dict.robot_derived_soa", "dict.controller_gains_soa", "dict.sim_steps"):
            x = raw_bits(r[name])
            x = x.reshape(n, -1).T if name == "obs" else x.reshape(-1, n)
            assert (x == x[:, :1]).all(), (j, name)
        mm = env.robot_manager.robot.control_allocator.motor_model
        for t in (mm.thrust_soa, mm.kT_soa, mm.tau_inc_soa, mm.tau_dec_soa):
            x = raw_bits(t)
            assert (x == x[:, :1]).all(), j
    # a partial fork: envs 3 and 4 take rows 1 and 2 of the snapshot, nothing else moves
    held = {e["name"]: raw_bits(e["tensor"]).copy() for e in table.entries}
    task.restore(snap, env_ids=torch.tensor([3, 4]), from_env_ids=torch.tensor([1, 2]))
    got, was, now = raw_bits(env.global_tensor_dict["robot_state_soa"]), spread["state"], held["state"]
    assert np.array_equal(got[:, [3, 4]], was[:, [1, 2]]) and np.array_equal(np.delete(got, [3, 4], axis=1), np.delete(now, [3, 4], axis=1))
    task.close()


def test_the_example_runs_and_prints_equal_checksums():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "snapshot_restore_example.py")], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    sums = dict(line.split(":", 1) for line in out.stdout.splitlines() if line.startswith(("resume", "uninterrupted", "fork")))
    assert sums["resume checksum"].strip() == sums["uninterrupted checksum"].strip(), out.stdout
    assert sums["fork spread"].strip() == "0", out.stdout
