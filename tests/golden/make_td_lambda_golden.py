#!/usr/bin/env python3
"""TD(lambda) fixtures: run the REAL reference build_td_lambda_targets (utils/rl_utils.py:4-14) on seeded inputs and store what
it computes, in float64.  Run in the build container only:
    python tests/golden/make_td_lambda_golden.py
Inputs: tests/td_lambda_oracle.py:make_case (float32 values, so the kernel reads exactly what the reference read).  Per case
(B, T) of SHAPES and lambda of LAMBDAS, gamma = GAMMA, with q[t] the target value at the next state of step t:
    G          the function called with target_qs[:, t+1] = q[t] (slot 0 is never read), terminated = term * (1 - padded),
               mask = 1 - padded - the definition csrc/td_lambda.hip implements
    G_literal  the same call with the batch's raw terminated flags, which are 1 on every padded step (quirk Q15): the sum
               over them goes past 1 and the padded rows' q reach every step
Writes tests/golden/td_lambda.npz (data only)."""
import os
import sys

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("MARL_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import td_lambda_oracle as tl  # noqa: E402
from utils.rl_utils import build_td_lambda_targets  # noqa: E402  (reference)

th.set_num_threads(1)


def call(q, r, term, padded, lam, mask_term):
    t = lambda a: th.tensor(np.asarray(a, dtype=np.float64))
    q, r, term, padded = t(q), t(r), t(term), t(padded)
    m = 1.0 - padded
    target_qs = th.cat([th.zeros(q.shape[0], 1, dtype=th.float64), q], dim=1)
    out = build_td_lambda_targets(r, term * m if mask_term else term, m, target_qs, None, tl.GAMMA, lam)
    return out.numpy()


def main():
    out = {}
    for i, (B, T) in enumerate(tl.SHAPES):
        k = tl.case_key(B, T)
        inputs = tl.make_case(B, T, seed=500 + i)
        for n, a in zip(("q", "r", "term", "padded"), inputs):
            out["%s/%s" % (k, n)] = a
        for lam in tl.LAMBDAS:
            out["%s/lam%g/G" % (k, lam)] = call(*inputs, lam, True)
            out["%s/lam%g/G_literal" % (k, lam)] = call(*inputs, lam, False)
            print(k, lam, "max|G| %.3g  max|G - G_literal| %.3g" % (
                np.abs(out["%s/lam%g/G" % (k, lam)]).max(),
                np.abs(out["%s/lam%g/G" % (k, lam)] - out["%s/lam%g/G_literal" % (k, lam)]).max()))
    path = os.path.join(HERE, "td_lambda.npz")
    np.savez_compressed(path, **out)
    print("td_lambda.npz written,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
