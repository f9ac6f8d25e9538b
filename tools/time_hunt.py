#!/usr/bin/env python3
"""Time of a lock-step's ENVIRONMENT launch on the hunt environment (csrc/hunt.hip): the step, and the fused choice + step, beside
the battle environment's step (csrc/battle.hip) of the same tree in the same process.

    python tools/time_hunt.py [--envs 64 1024 4096] [--maps 4v2 8v8] [--battle_maps 3m 3s5z] [--steps 16] [--reps 20]

HIP events around one pass over the first `steps` lock-steps of an episode, the unit state and the lengths put back to the
episode's start before every pass (two small copies per pass, inside the timing, on every row alike); after two passes of warm-up,
the median of `reps` passes, in microseconds per lock-step.  The predators and the allies stand still (no captures, and the battle's
enemies need the first steps to arrive), so every environment is live throughout the step's pass; the fused step chooses from a
fixed random q at epsilon 0.5, so an episode may end inside its pass: live_at_the_end counts those that did not.  The battle figure
is a yardstick for reading the number - a kernel of the same shape at other widths - not a bar.  One JSON line per (map, envs)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from marl_amd.env.battle import BattleEnv                          # noqa: E402
from marl_amd.env.hunt import HuntEnv                              # noqa: E402


def timed(fn):
    """microseconds of one call of fn between two HIP events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def median_us(fn, steps, reps):
    for _ in range(2):
        timed(fn)
    return round(statistics.median(timed(fn) for _ in range(reps)) / steps, 2)


def passes(env, steps, stay, dev):
    """{label: one pass over the first `steps` lock-steps from the episode's start} of an environment whose agents all give `stay`"""
    E, N, A = env.n_envs, env.n_agents, env.n_actions
    rec = env.new_record()
    env.begin_episode(rec)
    units0, length0 = env.units.clone(), rec.length.clone()
    act = torch.full((E, N), stay, dtype=torch.int32, device=dev)
    alive = torch.empty(E, dtype=torch.int32, device=dev)

    def rewind():
        env.units.copy_(units0)
        rec.length.copy_(length0)

    def step_pass():
        rewind()
        for t in range(steps):
            env.step(t, act, rec, alive)
    out = {"step": step_pass}
    if hasattr(env, "fused_step"):
        q = torch.randn(E, 1, N, A, generator=torch.Generator().manual_seed(3)).to(dev)

        def fused_pass():
            rewind()
            for t in range(steps):
                env.fused_step(t, q, 0.5, 7, rec)
        out["fused_step"] = fused_pass
    return out, rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, nargs="+", default=[64, 1024, 4096])
    p.add_argument("--maps", nargs="+", default=["4v2", "8v8"])
    p.add_argument("--battle_maps", nargs="+", default=["3m", "3s5z"])
    p.add_argument("--steps", type=int, default=16)
    p.add_argument("--reps", type=int, default=20)
    a = p.parse_args()
    dev = torch.device("cuda")
    for kind, names in (("hunt", a.maps), ("battle", a.battle_maps)):
        for name in names:
            for E in a.envs:
                env = HuntEnv(E, name, seed=1) if kind == "hunt" else BattleEnv(E, name, seed=1)
                fns, rec = passes(env, a.steps, 0 if kind == "hunt" else 1, dev)
                row = {"env": kind, "map": name, "envs": E, "steps": a.steps, "reps": a.reps}
                for label, fn in fns.items():
                    row[label + "_us"] = median_us(fn, a.steps, a.reps)
                row["live_at_the_end"] = int((rec.length == env.episode_limit).sum().item())
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
