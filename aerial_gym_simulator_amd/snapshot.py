"""Snapshot, restore and fork of the simulator state (INTEGRATION.md "Snapshot, restore, fork").

StateTable   the live tensors that make up the state, in a fixed order: what EnvManager and the task declare.  It becomes the
             AgxSnapshotTable that agx_state_gather / agx_state_scatter (csrc/agx_snapshot.hip) walk in ONE launch.
SimSnapshot  one packed [rows, num_envs] block of 32-bit words on the device, the host scalars that belong to it (step counter,
             flag parity, generator states, python's `random`, the task's counters) and a fingerprint of what took it.

Nothing here computes: a missing HIP library or a CPU env is an error, like everywhere else in the package."""
import random

import torch

from . import _lib

LAYOUTS = {"soa": _lib.SNAP_SOA, "aos": _lib.SNAP_AOS, "global": _lib.SNAP_GLOBAL}
# order in which a restore compares the fingerprint: the first field that differs is the one the ValueError names
FINGERPRINT_FIELDS = ("abi_version", "task", "robot", "controller", "env_name", "num_envs", "env_offset", "rng_seed", "layout")
_ELEM_SIZE = {torch.float32: 4, torch.int32: 4, torch.bool: 1, torch.uint8: 1}


class StateTable:
    """entries: dicts of name, tensor, rows, block_row, elem_size, layout ("soa" [rows, N] | "aos" [N, rows] | "global" [rows])"""

    def __init__(self, num_envs):
        self.num_envs = int(num_envs)
        self.entries = []
        self.block_rows = 0
        self.fingerprint = None  # set by the EnvManager that owns the table
        self._c = None

    def add(self, name, tensor, layout):
        N = self.num_envs
        if tensor is None or tensor.numel() == 0:
            return
        if layout not in LAYOUTS:
            raise ValueError(f"snapshot entry '{name}': layout {layout!r} (soa, aos, global)")
        if any(e["name"] == name for e in self.entries):
            raise ValueError(f"snapshot entry '{name}' declared twice")
        if tensor.dtype not in _ELEM_SIZE:
            raise TypeError(f"snapshot entry '{name}': dtype {tensor.dtype} (float32, int32, bool, uint8)")
        if not tensor.is_contiguous():
            raise ValueError(f"snapshot entry '{name}' is not contiguous: declare the storage, not a view of it")
        if layout == "global":
            rows = tensor.numel()
        else:
            env_axis = tensor.shape[-1] if layout == "soa" else tensor.shape[0]
            if env_axis != N or tensor.numel() % N:
                raise ValueError(f"snapshot entry '{name}': shape {tuple(tensor.shape)} has no env axis of {N} {'last' if layout == 'soa' else 'first'}")
            rows = tensor.numel() // N
        if len(self.entries) >= _lib.SNAPSHOT_MAX_ENTRIES:
            raise ValueError(f"more than {_lib.SNAPSHOT_MAX_ENTRIES} snapshot entries (AGX_SNAPSHOT_MAX_ENTRIES)")
        self.entries.append(dict(name=name, tensor=tensor, rows=rows, block_row=self.block_rows, elem_size=_ELEM_SIZE[tensor.dtype], layout=layout))
        self.block_rows += rows
        self._c = None

    def layout(self):
        """the part of the fingerprint that says what a block holds: [name, rows, dtype, layout] per entry"""
        return [[e["name"], e["rows"], str(e["tensor"].dtype).replace("torch.", ""), e["layout"]] for e in self.entries]

    def c_table(self, error_word):
        """the AgxSnapshotTable (built once per table; device pointers: the tensors must live on a HIP device)"""
        if self._c is None:
            T = _lib.AgxSnapshotTable()
            T.count, T.block_rows = len(self.entries), self.block_rows
            T.error = _lib.dptr(error_word)
            for j, e in enumerate(self.entries):
                E = T.entry[j]
                E.ptr, E.rows, E.block_row = _lib.dptr(e["tensor"]), e["rows"], e["block_row"]
                E.elem_size, E.layout = e["elem_size"], LAYOUTS[e["layout"]]
            self._c = T
        return self._c


def python_random_state():
    version, mt, gauss = random.getstate()
    return {"py_random_version": int(version), "py_random_mt": torch.tensor(mt, dtype=torch.int64),
            "py_random_gauss": torch.tensor([] if gauss is None else [gauss], dtype=torch.float64)}


def set_python_random_state(h):
    g = h["py_random_gauss"]
    random.setstate((int(h["py_random_version"]), tuple(int(x) for x in h["py_random_mt"].tolist()), float(g[0]) if g.numel() else None))


class SimSnapshot:
    def __init__(self, fingerprint, block, host):
        self.fingerprint = fingerprint  # dict over FINGERPRINT_FIELDS
        self.block = block              # int32 [rows, num_envs], on the device that took it
        self.host = host                # {"env": {...}, "task": {...}}: ints, strings, CPU tensors

    @property
    def nbytes(self):
        n = self.block.numel() * self.block.element_size()
        for part in self.host.values():
            n += sum(v.numel() * v.element_size() for v in part.values() if isinstance(v, torch.Tensor))
        return int(n)

    def state_dict(self):
        """plain CPU tensors, ints and strings (lists and dicts of them): goes through torch.save.  Copies the block to the host."""
        return {"fingerprint": {k: ([list(e) for e in v] if k == "layout" else v) for k, v in self.fingerprint.items()},
                "block": self.block.detach().cpu().clone(),
                "host": {part: {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in d.items()} for part, d in self.host.items()}}

    @classmethod
    def from_state_dict(cls, d, device):
        missing = [k for k in ("fingerprint", "block", "host") if k not in d]
        if missing:
            raise ValueError(f"not a SimSnapshot state_dict: {missing} missing")
        fp = dict(d["fingerprint"])
        fp["layout"] = [list(e) for e in fp.get("layout", [])]
        block = d["block"]
        rows = sum(int(e[1]) for e in fp["layout"])
        if block.dtype != torch.int32 or tuple(block.shape) != (rows, int(fp.get("num_envs", -1))):
            raise ValueError(f"SimSnapshot state_dict: block {block.dtype} {tuple(block.shape)}, the fingerprint describes int32 "
                             f"({rows}, {fp.get('num_envs')})")
        host = {part: {k: (v.detach().cpu().clone() if isinstance(v, torch.Tensor) else v) for k, v in h.items()} for part, h in d["host"].items()}
        return cls(fp, block.to(device).contiguous(), host)


def first_mismatch(mine, theirs):
    """name of the first FINGERPRINT_FIELDS entry that differs, or None"""
    for k in FINGERPRINT_FIELDS:
        a, b = mine.get(k), theirs.get(k)
        if k == "layout":
            a, b = [list(e) for e in (a or [])], [list(e) for e in (b or [])]
        if a != b:
            return k
    return None
