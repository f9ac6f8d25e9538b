#!/usr/bin/env python3
"""Time of a lock-step's ENVIRONMENT launches: the battle environment's one launch (csrc/battle.hip: step + slot t + 1) beside the
synthetic environment's unfused two (csrc/rollout.hip: step, then observe of slot t + 1) at the same (N, O, S, A), in one process.

    python tools/time_battle.py [--envs 64 1024 4096] [--maps 3m 2s3z 3s5z] [--steps 16] [--reps 20] [--rollout_reps 5]

HIP events around `reps` passes over the first `steps` lock-steps of an episode (every environment is still live there: the
agents stand still and the enemies need the first steps to arrive), seven rounds alternating between the two environments, the
median round of each.  The synthetic figure is a yardstick for reading the number - what the launches cost that this one replaces -
not a bar: the two kernels compute different things.  One JSON line per (map, envs).

Then, in the same process and protocol, a second line per (map, envs) with the three ROLLOUT paths over FusedBattleEnv, in
microseconds per lock-step of a whole episode_limit-step rollout of a SharedMAC with seeded random weights at epsilon 0.5 (init_hidden
and the reset included, no host read-back): "unfused" = agent step + select_actions + battle step, three launches a lock-step;
"fused_step" = agent step + fused step, two; "whole" = the persistent kernel (csrc/battle_rollout.hip), one launch per rollout.  The
episodes end where the fight ends (random weights lose within 17 - 48 steps), on all three paths alike: the per-step paths go on
launching to the time limit, the persistent kernel goes on stepping."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from marl_amd import ops                                          # noqa: E402
from marl_amd.env.battle import BattleEnv, FusedBattleEnv, battle_shapes      # noqa: E402
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


def rollout_paths(name, E, dev):
    """{path: one whole rollout, enqueued without a host read-back} over one FusedBattleEnv each"""
    import tempfile
    from marl_amd.controller.share_params import SharedMAC
    from marl_amd.main import build
    N, O, S, A, T = battle_shapes(name)
    tmp = os.path.join(tempfile.gettempdir(), "marl_battle_tool")      # build() only names the directories
    args, _ = build(["--env", "battle", "--map", name, "--alg", "qmix", "--n_envs", str(E), "--battle_fused", "True",
                     "--result_dir", tmp + "/result", "--model_dir", tmp + "/model"])
    torch.manual_seed(3)
    mac = SharedMAC(args)
    mac.cuda()
    H, eps, rseed = args.rnn_hidden_dim, 0.5, 7
    q = torch.empty(E, 1, N, A, device=dev)
    act = torch.empty(E, N, dtype=torch.int32, device=dev)
    alive = torch.empty(E, dtype=torch.int32, device=dev)

    def per_step(fused):
        env = FusedBattleEnv(E, name, seed=1)
        rec = env.new_record()

        def go():
            env.begin_episode(rec)
            mac.init_hidden(E)
            h = mac.hidden_states.view(E * N, H)
            w = mac.rollout_weights()
            alive.fill_(1)
            for t in range(T):
                mac.rollout_step(w, rec, t, h, q, E)
                if fused:
                    env.fused_step(t, q, eps, rseed, rec)
                else:
                    ops.select_actions(q, rec.avail[:, t], (T + 1) * N * A, alive, eps, rseed, env.env0, None, env.global_step(t), act,
                                       N, E, N, A)
                    env.step(t, act, rec, alive)
        return go

    def whole():
        env = FusedBattleEnv(E, name, seed=1)
        rec = env.new_record()

        def go():
            mac.init_hidden(E)
            env.whole_rollout(mac.agent.weights(), None, rseed, rec, args.last_action, args.reuse_network,
                              h_out=mac.hidden_states.view(E * N, H), eps_sched=(eps, 0.0, 0.05))
        return go
    return {"unfused": per_step(False), "fused_step": per_step(True), "whole": whole()}, T


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, nargs="+", default=[64, 1024, 4096])
    p.add_argument("--maps", nargs="+", default=["3m", "2s3z", "3s5z"])
    p.add_argument("--steps", type=int, default=16)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--rollout_reps", type=int, default=5, help="whole rollouts per round of the rollout rows (0: none)")
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
    for name in a.maps if a.rollout_reps > 0 else ():
        for E in a.envs:
            paths, T = rollout_paths(name, E, dev)
            for fn in paths.values():                                        # warm-up
                timed(fn, 1)
            rounds = {k: [] for k in paths}
            for _ in range(ROUNDS):
                for k, fn in paths.items():
                    rounds[k].append(timed(fn, a.rollout_reps) / (a.rollout_reps * T))
            row = {"map": name, "envs": E, "T": T, "reps": a.rollout_reps, "rounds": ROUNDS,
                   "plan": ops.battle_rollout_plan(E, *battle_shapes(name)[:2], battle_shapes(name)[3])}
            for k in paths:
                row[k + "_us_per_step"] = round(statistics.median(rounds[k]), 2)
                row[k + "_min_max_us"] = [round(min(rounds[k]), 2), round(max(rounds[k]), 2)]
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
