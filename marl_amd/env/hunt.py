"""Hunt: predator-prey with a lone-catch penalty, batched on the device (csrc/hunt.hip).

N predators (the agents) and M prey on a G x G grid.  A prey is captured, for 10 points, only when two or more predators next to it
catch in the same step; a predator that catches alone costs the team the map's penalty, so under random exploration "catch" looks bad
(relative overgeneralisation) - the task the non-monotonic learners were built for.  The prey walk at random and do not flee.  A map
name is ``<name>[_p<penalty>]``: ``4v2`` has no penalty, ``4v2_p2`` a penalty of 2, ``8v8_p1.5`` one of 1.5 (a multiple of 0.25 in
[0, 16]).  The rules are this project's own; every feature is exact in fp32.  Rules: csrc/hunt_env.h; numpy
restatement: tests/hunt_oracle.py.

The protocol is the one RolloutWorker._generate_batched uses: per lock-step the controller's launches and ONE environment launch -
``fused_step`` (the action choice inside the step's launch), or with ``rollout_mode = "unfused"`` the choice and ``step`` (which
writes slot t + 1, so ``observe`` launches nothing).  There is no whole-rollout kernel.
"""
from __future__ import annotations

import torch

from .. import ops
from ..hostutil import require_cuda
from .synthetic_smac import EpisodeRecord

N_ACTIONS, OBS = 6, 3 * 25 + 2
# map -> (grid side, predators, prey, episode limit)
HUNT_MAPS = {"2v1": (6, 2, 1, 30), "4v2": (8, 4, 2, 50), "8v8": (10, 8, 8, 100)}


def _no_map(name, why=""):
    return ValueError("--env hunt has no map %r%s (maps: %s, each with an optional penalty suffix _p<0 .. 16 in steps of 0.25>)"
                      % (name, why, ", ".join(HUNT_MAPS)))


def hunt_map(name):
    """(G, N, M, T, pen4) of a hunt map, pen4 = 4 x the penalty its suffix states; a ValueError for one the environment does not have.
    A tuple is a shape given directly (the tests' 16 against 16): it is returned as it is, and HuntEnv asks the kernels' range"""
    if isinstance(name, tuple):
        G, n, m, T, pen4 = name
        return int(G), int(n), int(m), int(T), int(pen4)
    base, sep, pen = str(name).partition("_p")
    if base not in HUNT_MAPS:
        raise _no_map(name)
    pen4 = 0
    if sep:
        digits = pen.replace(".", "", 1)
        if not digits.isdigit() or not pen[0].isdigit() or not pen[-1].isdigit():
            raise _no_map(name, ": %r is not a decimal number" % pen)
        q = 4 * float(pen)
        if q != int(q) or not 0 <= q <= 64:
            raise _no_map(name, ": the penalty is a multiple of 0.25 in [0, 16]")
        pen4 = int(q)
    return HUNT_MAPS[base] + (pen4,)


def hunt_shapes(name):
    """(N, O, S, A, T) of a hunt map, the tuple ``main.MAPS`` holds for the synthetic environment"""
    _, n, m, T, _ = hunt_map(name)
    return n, OBS, 2 * n + 3 * m, N_ACTIONS, T


class HuntEnv:
    """``episode_limit``: a time limit below the map's (the kernels take T as a parameter)"""
    batched = True

    def __init__(self, n_envs, map="4v2", seed=1, env0=0, episode_limit=None):
        self.grid, self.n_agents, self.n_prey, self.episode_limit, self.pen4 = hunt_map(map)
        self.map, self.n_envs, self.seed, self.env0 = map, n_envs, seed, env0
        _, self.obs_shape, self.state_shape, self.n_actions, _ = hunt_shapes(map)
        if episode_limit is not None:
            if not 1 <= int(episode_limit) <= self.episode_limit:
                raise ValueError("hunt: episode_limit %r is outside 1 .. %d of map %s" % (episode_limit, self.episode_limit, map))
            self.episode_limit = int(episode_limit)
        if not ops.hunt_supported(self.n_agents, self.n_prey, self.grid, self.n_actions) or not 0 <= self.pen4 <= 64:
            raise ValueError("hunt: %d predators and %d prey on a grid of side %d with pen4 = %d are outside the kernels' range"
                             % (self.n_agents, self.n_prey, self.grid, self.pen4))
        self.episode = -1
        self.device = require_cuda("HuntEnv")
        # x, y, live of every unit, predators first
        self.units = torch.zeros(n_envs, self.n_agents + self.n_prey, 3, dtype=torch.int32, device=self.device)

    def get_env_info(self):
        return {"n_actions": self.n_actions, "n_agents": self.n_agents, "state_shape": self.state_shape,
                "obs_shape": self.obs_shape, "episode_limit": self.episode_limit}

    def new_record(self):
        return EpisodeRecord(self.n_envs, self.episode_limit, self.n_agents, self.obs_shape, self.state_shape,
                             self.n_actions, self.device)

    def begin_episode(self, rec):
        self.episode += 1
        ops.hunt_reset(self.seed, self.env0, self.episode, self.grid, self.n_prey, self.units, rec)

    def observe(self, t, rec):
        pass        # slot 0 came from begin_episode, slot t + 1 from step

    def step(self, t, act, rec, alive_next):
        ops.hunt_step(self.seed, self.env0, self.episode, self.grid, self.pen4, t, act, self.units, rec, alive_next, self.n_prey)

    def fused_step(self, t, q, eps, rseed, rec, sample=False):
        """the action choice + step in one launch (same record as select_actions / policy_sample, then step)"""
        ops.hunt_fused_step(self.seed, rseed, self.env0, self.episode, self.grid, self.pen4, t, eps, q, self.units, rec,
                            self.n_prey, sample=sample)

    def global_step(self, t):
        return self.episode * (self.episode_limit + 1) + t

    def close(self):
        pass

    def save_replay(self):
        pass
