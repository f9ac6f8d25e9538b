#!/usr/bin/env python3
"""Trains --alg {qmix, ow_qmix, cw_qmix, maven (the table of noise index 0)} on the launcher's matrix game ([[8, -12, -12], [-12, 0, 0], [-12, 0, 0]], the payoff of the
Weighted QMIX paper) for --steps environment steps and prints ``get_q_and_q_tot_table()``: the 3 x 3 q_tot table and the two agents'
Q rows, with the argmax of the table.  The paper's outcome is the weighted variants' argmax at (0, 0) where QMIX's is not; what
happens here is recorded in DESIGN section 10, it is not a pass criterion.

    python tools/matrix_table.py --alg ow_qmix [--steps 20000] [--n_envs 32] [--seed 123]"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alg", default="ow_qmix", choices=["qmix", "ow_qmix", "cw_qmix", "maven"])
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--n_envs", type=int, default=32)
    ap.add_argument("--seed", type=int, default=123)
    o = ap.parse_args()
    from marl_amd.main import build, make_runner
    from marl_amd.utils.logging import Logger
    tmp = tempfile.mkdtemp(prefix="matrix_table_")
    args, env = build(["--env", "matrix", "--alg", o.alg, "--n_envs", str(o.n_envs), "--n_steps", str(o.steps), "--seed", str(o.seed),
                       "--evaluate_epoch", "0", "--result_dir", os.path.join(tmp, "res"), "--model_dir", os.path.join(tmp, "model")])
    args.save_cycle = 10 ** 9
    torch.manual_seed(o.seed)
    np.random.seed(o.seed)
    r = make_runner(args, env, Logger())
    loss = r.run(0)
    table, qi, qj = r.learner.get_q_and_q_tot_table()
    np.set_printoptions(precision=3, suppress=True)
    print("%s: %d environment steps, %d updates, final loss %.4f" % (o.alg, r.time_steps, r.train_steps, float(loss)))
    print("q_tot table\n%s" % table)
    print("agent 0 Q %s   agent 1 Q %s" % (qi, qj))
    print("%s argmax of the q_tot table: %s   greedy joint action of the agents: (%d, %d)"
          % (o.alg, tuple(int(x) for x in np.unravel_index(np.argmax(table), table.shape)), int(np.argmax(qi)), int(np.argmax(qj))), flush=True)
    env.close()


if __name__ == "__main__":
    main()
