"""Test helper: the table-driven gather / scatter of csrc/agx_snapshot.hip restated in numpy (include/aerial_gym_hip.h, "snapshot /
restore / fork"), and what the snapshot tests share: building a task on a device, recording a step's outputs, comparing records bit
for bit.  Imported like task_test_util.py; nothing here touches the GPU at import."""
import contextlib

import numpy as np
import torch

SENTINEL = 0xDEADBEEF


# ---- the restatement ---------------------------------------------------------------------------------------------------------
# An entry is (live, layout): live a numpy array of uint32 (4-byte elements, raw bits) or uint8 (1-byte elements), shaped
# [rows, n] ("soa"), [n, rows] ("aos") or [rows] ("global").  The block is uint32 [block_rows, n]; an entry of `rows` rows owns the
# rows * n words from word block_row * n on, in the order of its live tensor; a global entry uses the first `rows` of them.
def entry_rows(live, layout, n):
    return live.size if layout == "global" else live.size // n


def block_rows(entries, n):
    return sum(entry_rows(live, layout, n) for live, layout in entries)


def ref_gather(entries, n, block):
    """block (uint32 [rows, n], modified in place and returned) <- live tensors"""
    flat, row = block.reshape(-1), 0
    for live, layout in entries:
        rows = entry_rows(live, layout, n)
        words = rows if layout == "global" else rows * n
        flat[row * n: row * n + words] = live.reshape(-1).astype(np.uint32)  # (a byte is widened to a word)
        row += rows
    return block


def ref_scatter(entries, n, block, src=None, mask=None):
    """live[row][env] <- block[row][src[env]] where mask[env]; returns the new live arrays (the inputs are not modified)"""
    flat, row, out = block.reshape(-1), 0, []
    src_of = np.arange(n) if src is None else np.asarray(src, np.int64)
    take = np.ones(n, bool) if mask is None else np.asarray(mask) != 0
    for live, layout in entries:
        rows = entry_rows(live, layout, n)
        new = live.copy()
        if layout == "global":
            if mask is None:  # global words move only when every env does
                new = flat[row * n: row * n + rows].astype(live.dtype).reshape(live.shape)
        else:
            region = flat[row * n: (row + rows) * n]
            if layout == "soa":
                got = region.reshape(rows, n)[:, src_of]       # [rows, n]
                new2 = new.reshape(rows, n)
                new2[:, take] = got[:, take].astype(live.dtype)  # (a word is narrowed to a byte)
            else:
                got = region.reshape(n, rows)[src_of]          # [n, rows]
                new2 = new.reshape(n, rows)
                new2[take] = got[take].astype(live.dtype)
        out.append(new)
        row += rows
    return out


# ---- tasks -------------------------------------------------------------------------------------------------------------------
CONFIG_KEYS = ("seed", "num_envs", "headless", "device", "use_warp", "args", "episode_len_steps", "env_name", "robot_name",
               "controller_name")


@contextlib.contextmanager
def task_config(name, device, **overrides):
    """the (shared) config class of a registered task with `overrides` written in; everything is put back on exit"""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.registry.task_registry import task_registry
    from task_test_util import config_restored

    cfg = task_registry.get_task_config(name)
    with config_restored(cfg, CONFIG_KEYS):
        cfg.device = device
        for k, v in overrides.items():
            setattr(cfg, k, v)
        yield cfg


def make_task(name, n, seed=5):
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    return task_registry.make_task(name, seed=seed, num_envs=n, headless=True)


def record(task, ret):
    """everything a step leaves behind, cloned: the return tuple, every tensor of the global tensor dict (sensor images, obstacle
    poses, derived scene data included) and the torch generator's offset"""
    obs, rew, term, trunc, _info = ret
    out = {"obs": obs["observations"].clone(), "rewards": rew.clone(), "terminations": term.clone(), "truncations": trunc.clone()}
    g = task.sim_env.global_tensor_dict
    for k in dict.keys(g):
        v = dict.__getitem__(g, k)
        if isinstance(v, torch.Tensor):
            out["dict." + k] = v.clone()
    dev = torch.device(task.sim_env.device)
    if dev.type == "cuda":
        out["generator_offset"] = int(torch.cuda.default_generators[dev.index or 0].get_offset())
    return out


def raw_bits(t):
    a = t.detach().cpu().contiguous()
    if a.dtype == torch.bool:
        a = a.to(torch.uint8)
    return a.numpy().view(np.uint8 if a.element_size() == 1 else (np.uint32 if a.element_size() == 4 else np.uint64))


def assert_same_record(a, b, where, rows=None):
    """bit for bit, NaNs compared as bits (scene_bvh_nodes: every record a traversal can read, see below).  rows: compare only these
    envs of the tensors whose env axis is first or last"""
    assert a.keys() == b.keys(), (where, sorted(a.keys() ^ b.keys()))
    for k in a:
        if not isinstance(a[k], torch.Tensor):
            assert rows is not None or a[k] == b[k], (where, k, a[k], b[k])
            continue
        x, y = raw_bits(a[k]), raw_bits(b[k])
        assert x.shape == y.shape, (where, k)
        if rows is not None:
            n = len(rows)
            if x.ndim and x.shape[0] == n:
                x, y = x[rows], y[rows]
            elif x.ndim and x.shape[-1] == n:
                x, y = x[..., rows], y[..., rows]
            else:
                continue
        if k == "dict.scene_bvh_nodes" and not np.array_equal(x, y):
            # The tree is recomputed by a restore, not stored, and the builders write only the records a traversal can reach: a
            # record no child reference leads to keeps the words of whichever build last used it, in the live buffer as much as
            # after a restore.  Every record that CAN be read must be equal, at the same index; only the others may differ.
            for e in sorted(set(np.argwhere(x != y)[:, 0].tolist())):
                ra, rb = reachable_records(x[e]), reachable_records(y[e])
                assert ra == rb, f"{where}: the trees of env {e} reach different records"
                assert np.array_equal(x[e][ra], y[e][ra]), f"{where}: a reachable BVH record of env {e} differs"
            continue
        if not np.array_equal(x, y):
            bad = np.argwhere(x != y)
            raise AssertionError(f"{where}: '{k}' differs in {len(bad)} of {x.size} words, first at {bad[0].tolist()}")


# ---- the BVH's records --------------------------------------------------------------------------------------------------------
OBJECT_REF = 0x40000000  # AGX_BVH_OBJECT_REF


def reachable_records(nodes_env):
    """indices of the records of one env's tree ([R, 16] words) that a traversal from the root (record 0) can read: internal nodes and
    object nodes.  The builders write only those; a record no child reference leads to (the four spare records of a box object, a
    folded two-leaf node) keeps whatever an earlier build left there, and nothing ever reads it (include/aerial_gym_hip.h)."""
    refs = nodes_env.view(np.int32)
    seen, stack = set(), [0]
    while stack:
        i = stack.pop()
        if i in seen:
            continue
        seen.add(i)
        for word in (3, 7):
            c = int(refs[i, word])
            if c < 0:
                continue  # a leaf: triangle ~c
            if c & OBJECT_REF:
                seen.add(c & ~OBJECT_REF)  # an object node: the tree ends there
            else:
                stack.append(c)
    return sorted(seen)
