#!/usr/bin/env python3
"""HIP-event times of IQL's fused select-and-loss launch (csrc/iql.hip) beside the three launches it stands for - marl_q_gather,
marl_q_double_select and marl_td_loss on the same buffers (the loss on r / term / padded expanded to one entry per row) - and of
the TD(lambda) sequence select + returns + loss.  The fused call is the learner's: it writes q_taken and q_next too.  Same process,
alternating, median of --reps.  --A overrides the map's action count, --operands 2 leaves avail_next out and 1 leaves q_sel out as
well (the composition then selects with marl_q_masked_max): the staged form's row pitch and its switches.
    python tools/time_iql.py [--shape 2s3z] [--envs 4096] [--T 0] [--reps 30] [--A 0] [--operands 3]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--shape", default="2s3z")
    ap.add_argument("--T", type=int, default=0)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--A", type=int, default=0)
    ap.add_argument("--operands", type=int, default=3, choices=(1, 2, 3))
    o = ap.parse_args()
    from marl_amd import ops
    from marl_amd.algorithm.common import MASK_BIG
    a = bench.make_args("iql", o.shape, o.T)
    B, T, N, A = o.envs, a.episode_limit, a.n_agents, o.A or a.n_actions
    R, dev = B * T * N, torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    q, q_sel, q_tgt = rnd(R, A), rnd(R, A), rnd(R, A)
    avail = (torch.rand(R, A, device=dev, generator=g) < 0.7).float()
    u = torch.randint(0, A, (R,), device=dev, generator=g, dtype=torch.int32)
    r, term = rnd(B * T), (torch.rand(B * T, device=dev, generator=g) < 0.01).float()
    padded = (torch.rand(B * T, device=dev, generator=g) < 0.2).float()
    rows = lambda x: x.repeat_interleave(N).contiguous()
    r_r, term_r, padded_r = rows(r), rows(term), rows(padded)
    dq, qt, qn, out2 = [torch.zeros(R, device=dev) for _ in range(3)] + [torch.zeros(2, device=dev)]
    qn_bnt, G, per = torch.zeros(B, N, T, device=dev), torch.zeros(B, N, T, device=dev), torch.zeros(3, B, N, T, device=dev)
    for k, x in enumerate((r, term, padded)):
        per[k].copy_(x.view(B, 1, T).expand(B, N, T))

    if o.operands < 3:
        avail = None
    if o.operands < 2:
        q_sel = None
    qt_f, qn_f = torch.zeros(R, device=dev), torch.zeros(R, device=dev)

    def fused():
        ops.iql_loss_bwd(q, u, q_sel, q_tgt, avail, None, r, term, padded, 0.99, MASK_BIG, dq, out2, B, T, N, A, q_taken=qt_f, q_next=qn_f)

    def gather():
        ops.q_gather(q, u, qt, R, A)

    def dsel():
        if q_sel is None:
            ops.q_masked_max(q_tgt, avail, MASK_BIG, qn, None, R, A)
        else:
            ops.q_double_select(q_sel, q_tgt, avail, MASK_BIG, qn, None, R, A)

    def loss():
        ops.td_loss(qt, qn, r_r, term_r, padded_r, 0.99, dq, out2, R)

    def sel():
        ops.iql_select(q, u, q_sel, q_tgt, avail, padded, MASK_BIG, qt, qn_bnt, B, T, N, A)

    def ret():
        ops.td_lambda_returns(qn_bnt, per[0], per[1], per[2], 0.99, 0.8, G, B * N, T)

    def loss_ret():
        ops.iql_loss_bwd(q, u, None, None, None, G, None, None, padded, 0.99, MASK_BIG, dq, out2, B, T, N, A)

    fns = dict(fused=fused, q_gather=gather, q_double_select=dsel, td_loss=loss, iql_select=sel, td_lambda_returns=ret, loss_ret=loss_ret)
    ms = {k: [] for k in fns}
    for rep in range(o.reps + 3):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if rep >= 3:
                ms[k].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print("== iql rows %s envs=%d T=%d: R=%d A=%d operands=%d" % (o.shape, B, T, R, A, o.operands))
    for k in fns:
        print("  %-20s median %.4f  min %.4f ms" % (k, med[k], min(ms[k])))
    print("  fused %.4f ms   vs   gather + double_select + td_loss %.4f ms" % (med["fused"], med["q_gather"] + med["q_double_select"] + med["td_loss"]))
    print("  lambda: select + returns + loss %.4f ms" % (med["iql_select"] + med["td_lambda_returns"] + med["loss_ret"]))


if __name__ == "__main__":
    main()
