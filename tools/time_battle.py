#!/usr/bin/env python3
"""Time of a lock-step's ENVIRONMENT launches: the battle environment's one launch (csrc/battle.hip: step + slot t + 1) beside the
synthetic environment's unfused two (csrc/rollout.hip: step, then observe of slot t + 1) at the same (N, O, S, A), in one process.

    python tools/time_battle.py [--envs 64 1024 4096] [--maps 3m 2s3z 3s5z] [--steps 16] [--reps 20]

HIP events around `reps` passes over the first `steps` lock-steps of an episode (every environment is still live there: the
agents stand still and the enemies need the first steps to arrive), seven rounds alternating between the two environments, the
median round of each.  The synthetic figure is a yardstick for reading the number - what the launches cost that this one replaces -
not a bar: the two kernels compute different things.  One JSON line per (map, envs)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from marl_amd.env.battle import BattleEnv, battle_shapes          # noqa: E402
from marl_amd.env.synthetic_smac import SyntheticSMACEnv          # noqa: E402

ROUNDS = 7


def timed(fn, reps):
    """microseconds of `reps` calls of fn between two HIP events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, nargs="+", default=[64, 1024, 4096])
    p.add_argument("--maps", nargs="+", default=["3m", "2s3z", "3s5z"])
    p.add_argument("--steps", type=int, default=16)
    p.add_argument("--reps", type=int, default=20)
    a = p.parse_args()
    dev = torch.device("cuda")
    for name in a.maps:
        N, O, S, A, T = battle_shapes(name)
        for E in a.envs:
            battle = BattleEnv(E, name, seed=1)
            synth = SyntheticSMACEnv(E, N, O, S, A, T, seed=1, fixed_length=True)
            rb, rs = battle.new_record(), synth.new_record()
            act = torch.ones(E, N, dtype=torch.int32, device=dev)             # stop
            alive = torch.empty(E, dtype=torch.int32, device=dev)
            battle.begin_episode(rb)
            synth.begin_episode(rs)
            units0, length0 = battle.units.clone(), rb.length.clone()

            def battle_pass():
                battle.units.copy_(units0)          # back to the episode's start (two small copies per `steps` launches)
                rb.length.copy_(length0)
                for t in range(a.steps):
                    battle.step(t, act, rb, alive)

            def synth_pass():
                for t in range(a.steps):
                    synth.step(t, act, rs, alive)
                    synth.observe(t + 1, rs)
            for fn in (battle_pass, synth_pass):                             # warm-up
                timed(fn, 2)
            rounds = {"battle": [], "synthetic": []}
            for _ in range(ROUNDS):
                rounds["battle"].append(timed(battle_pass, a.reps) / (a.reps * a.steps))
                rounds["synthetic"].append(timed(synth_pass, a.reps) / (a.reps * a.steps))
            assert int((rb.length == T).sum().item()) == E, "an episode ended inside the timed steps"
            print(json.dumps({"map": name, "envs": E, "steps": a.steps, "reps": a.reps, "rounds": ROUNDS,
                              "battle_step_us": round(statistics.median(rounds["battle"]), 2),
                              "synthetic_step_observe_us": round(statistics.median(rounds["synthetic"]), 2),
                              "battle_min_max_us": [round(min(rounds["battle"]), 2), round(max(rounds["battle"]), 2)],
                              "synthetic_min_max_us": [round(min(rounds["synthetic"]), 2), round(max(rounds["synthetic"]), 2)]}),
                  flush=True)


if __name__ == "__main__":
    main()
