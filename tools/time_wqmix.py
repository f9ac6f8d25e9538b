#!/usr/bin/env python3
"""Cost of Weighted QMIX on one MI355X, per shape (2s3z, MMM2; T = 120, 4096 fixed-length episodes, f32 mode,
eager launches, one process):

* the WQMIXLearner update (--alg ow_qmix or cw_qmix) beside the QLearner(qmix, no_loss_fold) update built from the same tree, seven
  alternating rounds, host clock around a device synchronise (the set-up of tools/time_lica.py);
* by HIP events (median of --iters): marl_wqmix_select beside the launches it replaces - marl_q_gather twice (CW: three times),
  marl_q_masked_max with its argmax (CW only) and marl_q_double_select -, and marl_wqmix_loss beside two marl_td_loss calls; each
  beside the bytes it must move at 6.0 TB/s, the streaming rate tools/time_qatten.py uses;
* the footprint of the central mixer's kept activations: four (rows, 256) buffers for the eval forward, four more per further tag.

    python tools/time_wqmix.py --shape 2s3z [--alg cw_qmix] [--envs 4096] [--skip_update]

Run each shape under a time limit of its own."""
import argparse
import gc
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

HBM = 6.0e12


def time_update(o):
    from marl_amd.controller.share_params import SharedMAC
    from marl_amd.algorithm.q_learner import QLearner
    from marl_amd.algorithm.wqmix import WQMIXLearner
    from marl_amd.common.arguments import get_wqmix_args
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv

    def make(alg):
        args = bench.make_args(alg, o.shape, o.T)
        args.gemm_mode, args.hip_graph, args.no_loss_fold = "f32", False, True
        if alg != "qmix":
            get_wqmix_args(args)
        torch.manual_seed(0)
        mac = SharedMAC(args)
        learner = (QLearner if alg == "qmix" else WQMIXLearner)(mac, args)
        env = SyntheticSMACEnv(o.envs, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, args.episode_limit,
                               seed=1, fixed_length=True)
        w = RolloutWorker(env, mac, args)
        w.rollout_mode = "unfused"
        return args, learner, w

    (wa, wl, ww), (qa, ql, qw) = make(o.alg), make("qmix")
    ep_w, ep_q = ww.generate_episodes(o.envs)[0], qw.generate_episodes(o.envs)[0]
    steps = {o.alg: lambda i: wl.train(ep_w, i), "qmix": lambda i: ql.train(ep_q, i)}
    for f in steps.values():
        for i in range(3):
            f(i)
    gc.collect()
    gc.disable()
    rates = {k: [] for k in steps}
    for _ in range(o.rounds):
        for k, f in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(o.updates):
                f(i)
            torch.cuda.synchronize()
            rates[k].append((time.perf_counter() - t0) * 1e3 / o.updates)
    gc.enable()
    med = {k: statistics.median(r) for k, r in rates.items()}
    for k, r in rates.items():
        print("%-10s update  %s  envs %d  T %d  median %.2f ms  (min %.2f - max %.2f)" % (k, o.shape, o.envs, wa.episode_limit, med[k], min(r), max(r)))
    print("update %s / qmix (no_loss_fold) = %.2f" % (o.alg, med[o.alg] / med["qmix"]))
    rows, E = o.envs * wa.episode_limit, wa.central_mixing_embed_dim
    tags = 3 if o.alg == "cw_qmix" else 2
    print("central mixer: %.2f GB per (rows, %d) buffer, %d rows; kept: 4 per forward tag x %d tags (eval%s, target) + 2 gradient buffers = %.2f GB"
          % (rows * E * 4 / 1e9, E, rows, tags, ", greedy" if tags == 3 else "", (4 * tags + 2) * rows * E * 4 / 1e9), flush=True)


def time_kernels(o):
    from marl_amd import ops
    from marl_amd.algorithm.common import MASK_BIG
    dev = torch.device("cuda")
    N, O, S, A, T0 = bench.SHAPES[o.shape]
    B, T = o.envs, o.T or T0
    BT, R = B * T, B * T * N
    cw = o.alg == "cw_qmix"
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *shape: torch.randn(*shape, device=dev, generator=g)
    q, qc, q_en, qc_tgt = rnd(R, A), rnd(R, A), rnd(R, A), rnd(R, A)
    avail, avail_next = ((torch.rand(R, A, device=dev, generator=g) < 0.7).float() for _ in range(2))
    u = torch.randint(0, A, (R,), device=dev, generator=g, dtype=torch.int32)
    padded, term = (rnd(BT) > 1.0).float(), (rnd(BT) > 1.5).float()
    f = lambda: torch.empty(R, device=dev)
    i32 = lambda: torch.empty(R, dtype=torch.int32, device=dev)
    qt, qct, qcg, qcn, ug, un = f(), f(), f(), f(), i32(), i32()
    q_tot, q_cen, q_cen_g, q_next, r = rnd(BT), rnd(BT), rnd(BT), rnd(BT), rnd(BT)
    dq_tot, dqc, w, out4, out2 = torch.empty(BT, device=dev), torch.empty(BT, device=dev), torch.empty(BT, device=dev), torch.zeros(4, device=dev), torch.zeros(2, device=dev)

    def select():
        ops.wqmix_select(q, qc, u, avail if cw else None, q_en, qc_tgt, avail_next, padded, MASK_BIG, qt, qct, un, qcn, B, T, N, A,
                         u_greedy=ug if cw else None, qc_greedy=qcg if cw else None)

    def replaced():
        ops.q_gather(q, u, qt, R, A)
        ops.q_gather(qc, u, qct, R, A)
        if cw:
            ops.q_masked_max(q, avail, MASK_BIG, None, ug, R, A)
            ops.q_gather(qc, ug, qcg, R, A)
        ops.q_double_select(q_en, qc_tgt, avail_next, MASK_BIG, qcn, un, R, A)

    def loss():
        ops.wqmix_loss(q_tot, q_cen, q_cen_g if cw else None, q_next, r, term, padded, 0.99, u if cw else None, ug if cw else None, 0.75,
                       dq_tot, dqc, out4, BT, N, w=w)

    def two_td():
        ops.td_loss(q_tot, q_next, r, term, padded, 0.99, dq_tot, out2, BT)
        ops.td_loss(q_cen, q_next, r, term, padded, 0.99, dqc, out2, BT)

    # bytes per agent row / per step that must move: the staged row operands, the scalars read and the outputs written
    sel_b = 4 * ((6 * A if cw else 3 * A + 2) + 1 + 4 + (2 if cw else 0)) * R + 4 * BT
    rep_b = 4 * ((3 * A + 2 + 2 + 2 + 2) + ((2 * A + 1 + 1 + 2) if cw else 0)) * R
    loss_b = 4 * (6 + (1 + 2 * N if cw else 0) + 3) * BT
    td_b = 2 * 4 * (5 + 1) * BT
    for name, fn, nb in (("wqmix_select", select, sel_b), ("the launches it replaces", replaced, rep_b), ("wqmix_loss", loss, loss_b),
                         ("two td_loss calls", two_td, td_b)):
        for _ in range(o.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(o.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        t = statistics.median(ts)
        print("  %-26s %s %s R=%d A=%d  %9.1f us   %8.1f MB, %8.1f us at 6.0 TB/s (%.2f of it)"
              % (name, o.shape, o.alg, R, A, t, nb / 1e6, nb / HBM * 1e6, t / (nb / HBM * 1e6)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--shape", default="2s3z", choices=["2s3z", "MMM2"])
    ap.add_argument("--alg", default="ow_qmix", choices=["ow_qmix", "cw_qmix"])
    ap.add_argument("--T", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip_update", action="store_true")
    ap.add_argument("--skip_kernels", action="store_true")
    o = ap.parse_args()
    if not o.skip_kernels:
        time_kernels(o)
        gc.collect()
        torch.cuda.empty_cache()
    if not o.skip_update:
        time_update(o)


if __name__ == "__main__":
    main()
