#!/usr/bin/env python3
"""Learning curves on the battle environment: trains --alg qmix and --alg iql on map 3m for a stated number of updates and prints the
greedy evaluation win rate every so many updates, beside two fixed policies played on the same environment:

    stop    always stop (wins nothing: the enemies walk up and fire)
    attack  attack the lowest-index attackable enemy, else move east (stop at the edge)

    python tools/train_battle.py [--algs qmix iql] [--updates 400] [--every 50] [--n_envs 64] [--anneal_steps 6000] [--seed 123]
                                  [--battle_fused]

One update = one lock-step rollout of n_envs episodes into the replay ring + one learner update on a sampled batch (the launcher's
loop, marl_amd/runner.py).  --battle_fused: the rollouts take the whole-rollout kernel, one launch each, straight into the replay
ring.  One JSON line per evaluation; the last line of an algorithm carries the wall time per update."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from marl_amd.env.battle import BattleEnv                          # noqa: E402
from marl_amd.main import build, make_runner                        # noqa: E402
from marl_amd.utils.logging import Logger                           # noqa: E402


def stop_policy(avail):
    return torch.where(avail[:, :, 1] > 0, 1, 0).to(torch.int32)


def attack_policy(avail):
    shots = avail[:, :, 6:]
    act = torch.where(shots.sum(2) > 0, 6 + shots.argmax(2), torch.where(avail[:, :, 4] > 0, 4, 1))
    return torch.where(avail[:, :, 0] > 0, 0, torch.where(avail.sum(2) > 0, act, 0)).to(torch.int32)      # (argmax: the first maximum)


def play_fixed(policy, name, n_envs, seed, episodes=4):
    """win rate and mean episode reward of a fixed policy over `episodes` lock-step episodes of n_envs environments"""
    env = BattleEnv(n_envs, name, seed=seed)
    alive = torch.empty(n_envs, dtype=torch.int32, device=env.device)
    won = reward = 0.0
    for _ in range(episodes):
        rec = env.new_record()
        env.begin_episode(rec)
        for t in range(env.episode_limit):
            env.step(t, policy(rec.avail[:, t]), rec, alive)
        won += float(rec.won.float().mean().item())
        reward += float(rec.r.sum(1).mean().item())
    return won / episodes, reward / episodes


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--algs", nargs="+", default=["qmix", "iql"])
    p.add_argument("--map", default="3m")
    p.add_argument("--updates", type=int, default=400)
    p.add_argument("--every", type=int, default=50)
    p.add_argument("--n_envs", type=int, default=64)
    p.add_argument("--anneal_steps", type=int, default=6000, help="lock-steps over which epsilon falls from 1 to 0.05")
    p.add_argument("--seed", type=int, default=123)
    p.add_argument("--battle_fused", action="store_true", help="FusedBattleEnv: one launch per rollout")
    a = p.parse_args()
    for label, policy in (("stop", stop_policy), ("attack", attack_policy)):
        win, reward = play_fixed(policy, a.map, a.n_envs, a.seed)
        print(json.dumps({"policy": label, "map": a.map, "win_rate": round(win, 4), "episode_reward": round(reward, 3)}), flush=True)
    for alg in a.algs:
        with tempfile.TemporaryDirectory() as tmp:
            args, env = build(["--env", "battle", "--map", a.map, "--alg", alg, "--n_envs", str(a.n_envs), "--seed", str(a.seed),
                               "--evaluate_epoch", "1", "--result_dir", tmp + "/result", "--model_dir", tmp + "/model",
                               "--battle_fused", str(a.battle_fused)])
            args.save_cycle = 10 ** 9
            args.anneal_epsilon = (args.epsilon - args.min_epsilon) / a.anneal_steps
            torch.manual_seed(a.seed)
            r = make_runner(args, env, Logger())
            w, wins, loss = r.rolloutWorker, [], float("nan")
            spent = 0.0
            for k in range(a.updates + 1):
                if k % a.every == 0:
                    win, reward = r.evaluate()
                    print(json.dumps({"alg": alg, "map": a.map, "update": k, "eval_win_rate": round(win, 4),
                                      "eval_episode_reward": round(reward, 3), "epsilon": round(w.epsilon, 3),
                                      "train_win_rate": round(sum(wins) / max(len(wins), 1), 4),
                                      "loss": None if loss != loss else round(loss, 5)}), flush=True)
                    wins = []
                if k == a.updates:
                    break
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                episodes, _, tags, steps = w.generate_episodes(a.n_envs)
                wins += tags
                r.time_steps += steps
                r.buffer.store_episode(episodes)
                loss = float(r.learner.train(r.buffer.sample(min(r.buffer.current_size, args.batch_size)), r.train_steps))
                r.train_steps += 1
                torch.cuda.synchronize()
                spent += time.perf_counter() - t0
            print(json.dumps({"alg": alg, "map": a.map, "battle_fused": a.battle_fused, "updates": a.updates,
                              "ms_per_update": round(1e3 * spent / max(a.updates, 1), 3)}), flush=True)


if __name__ == "__main__":
    main()
