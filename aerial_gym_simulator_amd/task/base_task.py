"""aerial_gym/task/base_task.py:10-54"""
import os
import random
import time
from abc import ABC, abstractmethod

import numpy as np
import torch


class BaseTask(ABC):
    def __init__(self, task_config):
        self.task_config = task_config
        self.action_space = self.observation_space = None
        self.reward_range = self.metadata = self.spec = None
        seed = task_config.seed
        if seed == -1:
            seed = time.time_ns() % (2**32)
        self.seed(seed)

    def seed(self, seed):
        if seed is None or seed < 0:
            seed = time.time_ns() % (2**32)
        np.random.seed(seed)
        torch.manual_seed(seed)
        if torch.cuda.is_available():
            torch.cuda.manual_seed_all(seed)
        os.environ["PYTHONHASHSEED"] = str(seed)
        random.seed(seed)

    # ---- snapshot / restore / fork (snapshot.py; the env side is EnvManager.snapshot / restore) -------------------------------
    # A task DECLARES its state and this class moves it; no task copies anything by hand:
    #   SNAPSHOT_TENSORS  (attribute path, layout) of the per-env tensors its next step() reads.  Path: dotted attributes, a
    #                     ["key"] for a dict ("task_obs[observations]"); layout "soa" (env axis last), "aos" (env axis first) or
    #                     "global" (a small device tensor that is not per env: restored only with the whole state).
    #   SNAPSHOT_HOST     names of host attributes (ints, bools, floats): restored only with the whole state.
    # None (the default) means the class has not said what its state is: snapshot() and restore() raise NotImplementedError
    # naming it, on the task and on its env manager -- a snapshot that silently misses a tensor is the one thing never handed out.
    SNAPSHOT_TENSORS = None
    SNAPSHOT_HOST = ()

    def _own_env_state(self):
        """called by a task's constructor once sim_env exists: from now on the env manager's snapshot carries this task's state"""
        self.sim_env._state_owner = self

    def _snapshot_refusal(self):
        """raise for a mode of this task a snapshot would capture only in part (subclasses add theirs and call super)"""
        declared = type(self).__dict__.get("SNAPSHOT_TENSORS")
        if declared is None:  # (looked up on the class itself: a subclass with state of its own does not inherit its parent's list)
            raise NotImplementedError(f"{type(self).__name__} does not declare its state (SNAPSHOT_TENSORS): snapshot / restore are not "
                                      f"implemented for {type(self).__name__}")

    def _resolve(self, path):
        obj = self
        for part in path.replace("]", "").replace("[", ".[").split("."):
            obj = obj[part[1:]] if part.startswith("[") else getattr(obj, part)
        return obj

    def _snapshot_entries(self):
        return [(path, self._resolve(path), layout) for path, layout in type(self).__dict__.get("SNAPSHOT_TENSORS") or ()]

    def _snapshot_host(self):
        out = {}
        for name in self.SNAPSHOT_HOST:
            v = getattr(self, name)
            if isinstance(v, torch.Tensor):  # (a counter a strict-mode reduction turned into a 0-d device tensor: reading it
                # synchronises, as that mode's own step does every time)
                v = int(v)
            if not isinstance(v, (bool, int, float)):
                raise TypeError(f"{type(self).__name__}.{name} = {v!r}: SNAPSHOT_HOST takes ints, bools and floats")
            out[name] = v
        return out

    def _restored(self, host, whole):
        """after the env manager put the tensors back.  `whole`: every env was restored, and the global quantities with them"""
        if whole:
            for name in self.SNAPSHOT_HOST:
                setattr(self, name, host[name])

    def snapshot(self, out=None):
        """EnvManager.snapshot of this task's env: the env's state and this task's own, in one SimSnapshot"""
        return self.sim_env.snapshot(out=out)

    def restore(self, snap, env_ids=None, from_env_ids=None):
        """EnvManager.restore: every env (env_ids None: bit-exact continuation), the envs of an index tensor / mask (global
        quantities are NOT restored), or a fork (from_env_ids)"""
        return self.sim_env.restore(snap, env_ids=env_ids, from_env_ids=from_env_ids)

    @abstractmethod
    def render(self, mode="human"):
        raise NotImplementedError

    @abstractmethod
    def reset(self):
        raise NotImplementedError

    @abstractmethod
    def reset_idx(self, env_ids):
        raise NotImplementedError

    @abstractmethod
    def step(self, action):
        raise NotImplementedError

    @abstractmethod
    def close(self):
        raise NotImplementedError
