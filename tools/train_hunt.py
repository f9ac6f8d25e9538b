#!/usr/bin/env python3
"""Learning curves on the hunt environment: trains vdn, qmix, qplex and cw_qmix on 4v2 (no penalty) and 4v2_p2 (a lone catch costs
2) for a stated number of updates and prints the greedy evaluation win rate and mean episode return every so many updates, beside
two scripted policies of the numpy oracle (tests/hunt_oracle.py) on the same map:

    team     walk onto the lowest-index prey, catch only together (the coordinated policy: every episode won, return 10 per prey)
    uniform  uniform over the available actions (what exploration sees: at a penalty the return is negative)

    python tools/train_hunt.py [--algs vdn qmix qplex cw_qmix] [--maps 4v2 4v2_p2] [--updates 400] [--every 50] [--n_envs 64]
                               [--anneal_steps 6000] [--seed 123]

One update = one lock-step rollout of n_envs episodes into the replay ring + one learner update on a sampled batch (the launcher's
loop, marl_amd/runner.py).  One JSON line per scripted policy and per evaluation; the last line of a run carries the wall time per
update.  What to look for: at penalty 2 the weighted and duplex learners reach captures where QMIX and VDN stay near 0."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import hunt_oracle as ho                                             # noqa: E402
from marl_amd.main import build, make_runner                        # noqa: E402
from marl_amd.utils.logging import Logger                           # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--algs", nargs="+", default=["vdn", "qmix", "qplex", "cw_qmix"])
    p.add_argument("--maps", nargs="+", default=["4v2", "4v2_p2"])
    p.add_argument("--updates", type=int, default=400)
    p.add_argument("--every", type=int, default=50)
    p.add_argument("--n_envs", type=int, default=64)
    p.add_argument("--anneal_steps", type=int, default=6000, help="lock-steps over which epsilon falls from 1 to 0.05")
    p.add_argument("--seed", type=int, default=123)
    a = p.parse_args()
    for name in a.maps:
        for label in ("team", "uniform"):
            rec = ho.play(name, a.n_envs, a.seed, ho.POLICIES[label](a.seed))
            print(json.dumps({"policy": label, "map": name, "win_rate": round(float(rec["won"].mean()), 4),
                              "episode_reward": round(float(rec["r"].sum(axis=1).mean()), 3)}), flush=True)
        for alg in a.algs:
            with tempfile.TemporaryDirectory() as tmp:
                args, env = build(["--env", "hunt", "--map", name, "--alg", alg, "--n_envs", str(a.n_envs), "--seed", str(a.seed),
                                   "--evaluate_epoch", "1", "--result_dir", tmp + "/result", "--model_dir", tmp + "/model"])
                args.save_cycle = 10 ** 9
                args.anneal_epsilon = (args.epsilon - args.min_epsilon) / a.anneal_steps
                torch.manual_seed(a.seed)
                r = make_runner(args, env, Logger())
                w, wins, loss = r.rolloutWorker, [], float("nan")
                spent = 0.0
                for k in range(a.updates + 1):
                    if k % a.every == 0:
                        win, reward = r.evaluate()
                        print(json.dumps({"alg": alg, "map": name, "update": k, "eval_win_rate": round(win, 4),
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
                print(json.dumps({"alg": alg, "map": name, "updates": a.updates,
                                  "ms_per_update": round(1e3 * spent / max(a.updates, 1), 3)}), flush=True)


if __name__ == "__main__":
    main()
