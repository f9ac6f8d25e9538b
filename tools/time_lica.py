#!/usr/bin/env python3
"""Cost of LICA on one MI355X, per shape (2s3z, MMM2; T = 120, 4096 fixed-length episodes, f32 mode, eager
launches):

* the LICALearner update beside the CentralVLearner update built from the same tree, seven alternating rounds, host clock around a
  device synchronise (the set-up of tools/time_coma.py);
* the three entries of csrc/lica.hip and marl_policy_probs_bwd as the update calls them, by HIP events (median of --iters), each
  beside its byte floor: the bytes it must move at 6.0 TB/s, the streaming rate tools/time_qatten.py uses (the contiguous rows of
  profiles/r06_wbw_probe.txt: 5.8 - 6.1 TB/s).  hy alone is 3.5 GB (2s3z) / 11.4 GB (MMM2), far past the 256 MB Infinity Cache, so
  the operands are not rotated.

    python tools/time_lica.py --shape 2s3z [--envs 4096] [--skip_update]

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
    from marl_amd.controller.share_params import PolicyMAC
    from marl_amd.algorithm.central_v import CentralVLearner
    from marl_amd.algorithm.lica import LICALearner
    from marl_amd.common.arguments import get_centralv_args, get_lica_args
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv

    def make(alg):
        args = bench.make_args(alg, o.shape, o.T)
        args.gemm_mode, args.hip_graph = "f32", False
        (get_lica_args if alg == "lica" else get_centralv_args)(args)
        torch.manual_seed(0)
        mac = PolicyMAC(args)
        learner = (LICALearner if alg == "lica" else CentralVLearner)(mac, args)
        env = SyntheticSMACEnv(o.envs, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, args.episode_limit,
                               seed=1, fixed_length=True)
        w = RolloutWorker(env, mac, args)
        w.rollout_mode = "unfused"
        return args, learner, w

    (la, ll, lw), (va, vl, vw) = make("lica"), make("central_v")
    ep_l, ep_v = lw.generate_episodes(o.envs)[0], vw.generate_episodes(o.envs)[0]
    steps = {"lica": lambda i: ll.train(ep_l, i, epsilon=lw.epsilon), "central_v": lambda i: vl.train(ep_v, i, epsilon=vw.epsilon)}
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
        print("%-10s update  %s  envs %d  T %d  median %.2f ms  (min %.2f - max %.2f)" % (k, o.shape, o.envs, la.episode_limit, med[k], min(r), max(r)))
    print("update lica / central_v = %.2f" % (med["lica"] / med["central_v"]), flush=True)


def time_kernels(o):
    from marl_amd import ops
    dev = torch.device("cuda")
    N, O, S, A, T0 = bench.SHAPES[o.shape]
    E, T = 32, o.T or T0
    R, K = o.envs * T, N * A
    KE = K * E
    W = KE + 2 * E + 1
    ld = (W + 3) // 4 * 4
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *shape: torch.randn(*shape, device=dev, generator=g)
    hy = rnd(R, ld)[:, :W]
    dhy = torch.empty(R, ld, device=dev)[:, :W - 1]
    u = torch.randint(0, A, (R * N,), device=dev, generator=g, dtype=torch.int32)
    logits, avail = rnd(R * N, A), (torch.rand(R * N, A, device=dev, generator=g) < 0.7).float()
    avail[:, 0] = 1.0
    pi, dpi, dlogits = (torch.empty(R * N, A, device=dev) for _ in range(3))
    ent = torch.empty(R * N, device=dev)
    ops.policy_probs(logits, avail, 0.3, pi, R * N, A)
    x = pi.view(R, K)
    q, q_tgt, r, dq_tot, dq = rnd(R), rnd(R), rnd(R), torch.empty(R, device=dev), rnd(R)
    term, padded = (rnd(R) > 1.5).float(), (rnd(R) > 1.0).float()
    out2, out3 = torch.zeros(2, device=dev), torch.zeros(3, device=dev)
    a = (R, N, A, E)
    tail = 2 * E + 1
    entries = (
        ("mix_fwd (u)", lambda: ops.lica_mix_fwd(hy, None, u, q, *a), 4 * (N * E + tail + N + 1)),
        ("mix_fwd (pi)", lambda: ops.lica_mix_fwd(hy, x, None, q, *a), 4 * (KE + tail + K + 1)),
        ("mix_bwd (pi, dx alone)", lambda: ops.lica_mix_bwd(hy, x, None, dq, None, dpi.view(R, K), *a), 4 * (KE + tail + K + 1 + K)),
        ("loss_bwd", lambda: ops.lica_loss_bwd(hy, u, q_tgt, r, term, padded, 0.0, q, dhy, dq_tot, out2, *a),
         4 * (N * E + tail + N + 4 + KE + 2 * E + 2)),
        ("policy_probs_bwd", lambda: ops.policy_probs_bwd(logits, avail, dpi, q, padded, 0.3, 0.01, dlogits, ent, out3, R * N, N, A),
         4 * (N * (4 * A + 1) + 2)),
    )
    tr, grid, lds, walks = ops.lica_plan(*a)
    print("%s rows %d: tile %d rows, %d workgroups, %d B LDS, %d tiles per workgroup; hy %.2f GB" % (o.shape, R, tr, grid, lds, walks, R * ld * 4 / 1e9))
    for name, fn, per_row in entries:
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
        t, nb = statistics.median(ts), per_row * R
        print("  %-24s %9.1f us   %6d B/row, %8.1f MB, %8.1f us at 6.0 TB/s (%.2f of it)" % (name, t, per_row, nb / 1e6, nb / HBM * 1e6, t / (nb / HBM * 1e6)),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--shape", default="2s3z", choices=["2s3z", "MMM2"])
    ap.add_argument("--T", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip_update", action="store_true")
    ap.add_argument("--skip_kernels", action="store_true")
    o = ap.parse_args()
    if not o.skip_update:
        time_update(o)
        gc.collect()
        torch.cuda.empty_cache()
    if not o.skip_kernels:
        time_kernels(o)


if __name__ == "__main__":
    main()
