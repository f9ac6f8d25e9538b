"""Battle: a deterministic micro-combat simulator in SMAC's layout, batched on the device (csrc/battle.hip).

N allies against the same N enemy units on a 32 x 32 grid: moves of 2 cells, attacks within range 6 on a cooldown, shields before hp,
a scripted enemy that walks to and fires at its nearest ally.  Observation, state and availability columns are in SMAC's order, so
2s3z and 3s5z have the (N, O, S, A) of ``main.MAPS``; the numbers are this project's own, chosen so that every
feature is exact in fp32 - nothing here claims to be StarCraft.  Rules: csrc/battle_env.h; numpy restatement: tests/battle_oracle.py.

The protocol is SyntheticSMACEnv's (RolloutWorker._generate_batched), without fused_step and whole_rollout: per lock-step the
controller's launches, the action choice and ONE environment launch (``step`` writes slot t + 1, so ``observe`` launches nothing).
``FusedBattleEnv`` (``--battle_fused``) adds the two: the choice inside the step's launch, and the whole rollout - reset, agent
steps, choices and battle steps - in one persistent launch (csrc/battle_rollout.hip); the record is the same, bit for bit.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from ..hostutil import require_cuda
from .synthetic_smac import EpisodeRecord, next_kernel_stats

MARINE, STALKER, ZEALOT = 0, 1, 2
# (hp, shield, damage, cooldown) by type
UNITS = {MARINE: (45, 0, 6, 1), STALKER: (80, 80, 13, 2), ZEALOT: (100, 50, 16, 1)}
# map -> (unit types of either side, episode limit, shield columns, type bits)
BATTLE_MAPS = {"3m": ((MARINE,) * 3, 60, False, 0),
               "2s3z": ((STALKER,) * 2 + (ZEALOT,) * 3, 120, True, 2),
               "3s5z": ((STALKER,) * 3 + (ZEALOT,) * 5, 150, True, 2)}


def battle_map(name):
    """(types, T, shield, type_bits) of a battle map; a ValueError for one the environment does not have"""
    if name == "MMM2":
        raise ValueError("--env battle has no map MMM2: its medivac heals, and heal actions are not part of the battle rules "
                         "(maps: %s)" % ", ".join(BATTLE_MAPS))
    if name not in BATTLE_MAPS:
        raise ValueError("--env battle has no map %r (maps: %s)" % (name, ", ".join(BATTLE_MAPS)))
    return BATTLE_MAPS[name]


def battle_shapes(name):
    """(N, O, S, A, T) of a battle map, the tuple ``main.MAPS`` holds for the synthetic environment"""
    types, T, shield, tb = battle_map(name)
    n = m = len(types)
    a = 6 + m
    nf = 5 + int(shield) + tb
    return n, 4 + (m + n - 1) * nf + 1 + int(shield) + tb, n * (4 + int(shield) + tb) + m * (3 + int(shield) + tb) + n * a, a, T


def reward_scale(types, shield):
    """fp32 20 / (sum of enemy hp and shield + 10 per enemy + 200): a won episode's rewards sum to 20"""
    total = sum(UNITS[t][0] + (UNITS[t][1] if shield else 0) for t in types) + 10 * len(types) + 200
    return float(np.float32(20) / np.float32(total))


class BattleEnv:
    batched = True

    def __init__(self, n_envs, map="3m", seed=1, env0=0):
        self.types, self.episode_limit, self.shield, self.type_bits = battle_map(map)
        self.map, self.n_envs, self.seed, self.env0 = map, n_envs, seed, env0
        self.n_agents, self.obs_shape, self.state_shape, self.n_actions, _ = battle_shapes(map)
        self.n_enemies = self.n_agents
        if not ops.battle_supported(self.n_agents, self.n_enemies, self.n_actions):
            raise ValueError("battle: %d against %d units with %d actions is outside the kernels' range"
                             % (self.n_agents, self.n_enemies, self.n_actions))
        self.type_mask = sum(t << (2 * i) for i, t in enumerate(self.types))
        self.scale = reward_scale(self.types, self.shield)
        self.episode = -1
        self.device = require_cuda("BattleEnv")
        # x, y, hp, shield, cooldown of every unit, allies first
        self.units = torch.zeros(n_envs, self.n_agents + self.n_enemies, 5, dtype=torch.int32, device=self.device)

    def get_env_info(self):
        return {"n_actions": self.n_actions, "n_agents": self.n_agents, "state_shape": self.state_shape,
                "obs_shape": self.obs_shape, "episode_limit": self.episode_limit}

    def new_record(self):
        return EpisodeRecord(self.n_envs, self.episode_limit, self.n_agents, self.obs_shape, self.state_shape,
                             self.n_actions, self.device)

    def begin_episode(self, rec):
        self.episode += 1
        ops.battle_reset(self.seed, self.env0, self.episode, self.type_mask, self.shield, self.type_bits, self.units, rec,
                         self.n_enemies)

    def observe(self, t, rec):
        pass        # slot 0 came from begin_episode, slot t + 1 from step

    def step(self, t, act, rec, alive_next):
        ops.battle_step(self.type_mask, self.shield, self.type_bits, self.scale, t, act, self.units, rec, alive_next,
                        self.n_enemies)

    def global_step(self, t):
        return self.episode * (self.episode_limit + 1) + t

    def close(self):
        pass

    def save_replay(self):
        pass


class FusedBattleEnv(BattleEnv):
    """BattleEnv with the fused step and the whole-rollout kernel: RolloutWorker dispatches on the two attributes.
    ``episode_limit``: a time limit below the map's (the kernels take T as a parameter)."""

    def __init__(self, n_envs, map="3m", seed=1, env0=0, episode_limit=None):
        super().__init__(n_envs, map, seed=seed, env0=env0)
        if episode_limit is not None:
            if not 1 <= int(episode_limit) <= self.episode_limit:
                raise ValueError("battle: episode_limit %r is outside 1 .. %d of map %s" % (episode_limit, self.episode_limit, map))
            self.episode_limit = int(episode_limit)

    def fused_step(self, t, q, eps, rseed, rec, sample=False):
        """the action choice + step in one launch (same record as select_actions / policy_sample, then step)"""
        ops.battle_fused_step(self.type_mask, self.shield, self.type_bits, self.scale, rseed, self.env0, self.episode, t, eps, q,
                              self.units, rec, self.n_enemies, sample=sample)

    def supports_whole_rollout(self):
        return ops.battle_rollout_supported(self.n_agents, self.obs_shape, self.n_actions)

    def whole_rollout(self, weights, eps_dev, rseed, rec, last_action, reuse_network, h_out=None, eps_sched=None, x6=False,
                      sample=False):
        """Reset and all episode_limit lock-steps in ONE persistent launch; same record and unit state as begin_episode and
        fused_step called step by step.  The kernel evaluates the epsilon schedule itself (eps_sched; no device vector) and is the
        fp32 one whatever x6 says.  sample: as fused_step(..., sample=True)."""
        if eps_dev is not None or eps_sched is None:
            raise ValueError("battle: the whole-rollout kernel takes the epsilon schedule (eps_sched), not a device vector")
        self.episode += 1
        ops.battle_rollout(weights, self.seed, rseed, self.env0, self.episode, self.type_mask, self.shield, self.type_bits,
                           self.scale, self.units, rec, h_out, self.n_enemies, last_action, reuse_network,
                           next_kernel_stats(self, rec), eps_sched, sample=sample)
