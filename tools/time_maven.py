#!/usr/bin/env python3
"""Cost of MAVEN on one MI355X, per shape (2s3z, MMM2; T = 120, 4096 fixed-length episodes, f32 mode, eager
launches, one process):

* the MAVENLearner update (--alg maven) beside the QLearner(qmix, no_loss_fold) update built from the same tree, seven alternating
  rounds of five updates, host clock around a device synchronise (the set-up of tools/time_wqmix.py);
* by HIP events (median of --iters) the three new entries of csrc/maven.hip - marl_maven_head_fwd, marl_maven_head_bwd and
  marl_maven_mi -, each beside the bytes it must move at 6.0 TB/s, the streaming rate tools/time_qatten.py uses.

    python tools/time_maven.py --shape 2s3z [--envs 4096] [--skip_update]

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
    from marl_amd.controller.share_params import SharedMAC, MAVENMAC
    from marl_amd.algorithm.q_learner import QLearner
    from marl_amd.algorithm.maven import MAVENLearner
    from marl_amd.common.arguments import get_maven_args
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv

    def make(alg):
        args = bench.make_args(alg, o.shape, o.T)
        args.gemm_mode, args.hip_graph, args.no_loss_fold = "f32", False, True
        if alg == "maven":
            get_maven_args(args)
        torch.manual_seed(0)
        mac = (MAVENMAC if alg == "maven" else SharedMAC)(args)
        learner = (MAVENLearner if alg == "maven" else QLearner)(mac, args)
        env = SyntheticSMACEnv(o.envs, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, args.episode_limit,
                               seed=1, fixed_length=True)
        w = RolloutWorker(env, mac, args)
        w.rollout_mode = "unfused"
        return args, learner, w

    (ma, ml, mw), (qa, ql, qw) = make("maven"), make("qmix")
    ep_m, ep_q = mw.generate_episodes(o.envs)[0], qw.generate_episodes(o.envs)[0]
    steps = {"maven": lambda i: ml.train(ep_m, i), "qmix": lambda i: ql.train(ep_q, i)}
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
        print("%-10s update  %s  envs %d  T %d  median %.2f ms  (min %.2f - max %.2f)" % (k, o.shape, o.envs, ma.episode_limit, med[k], min(r), max(r)))
    print("update maven / qmix (no_loss_fold) = %.2f" % (med["maven"] / med["qmix"]), flush=True)


def time_kernels(o):
    from marl_amd import ops
    dev = torch.device("cuda")
    N, O, S, A, T0 = bench.SHAPES[o.shape]
    B, T, K, H, D = o.envs, o.T or T0, 16, 64, 64
    BT, R = B * T, B * T * N
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *shape: torch.randn(*shape, device=dev, generator=g)
    hs, q = rnd(B, T, N, H), rnd(B, T, N, A)
    noise = torch.randint(0, K, (B,), device=dev, generator=g, dtype=torch.int32)
    tab = {"maven.noise_w": rnd(K, A, H) * 0.2, "maven.id_w": rnd(N, A, H) * 0.2, "maven.noise_b": rnd(K, A) * 0.2, "maven.id_b": rnd(N, A) * 0.2}
    w, gw = ops.maven_weights(tab), ops.maven_grads({k: torch.zeros_like(v) for k, v in tab.items()})
    u = torch.randint(0, A, (R,), device=dev, generator=g, dtype=torch.int32)
    dq_val, dq_dense = rnd(R), rnd(B, T, N, A)
    dq_out, dhs = torch.empty(B, T, N, A, device=dev), torch.empty(B, T, N, H, device=dev)
    avail = (torch.rand(B, T + 1, N, A, device=dev, generator=g) < 0.7).float()
    avail[..., 0] = 1.0
    SP = (S + 3) // 4 * 4
    state = rnd(B * (T + 1), SP)[:, :S]
    emap = torch.randperm(B, device=dev, generator=g).to(torch.int32)
    padded = (rnd(BT) > 1.0).float()
    disc = {"l1.weight": rnd(D, N * A + S) * 0.05, "l1.bias": rnd(D) * 0.05, "l2.weight": rnd(K, D) * 0.1, "l2.bias": rnd(K) * 0.1}
    d, gd = ops.maven_disc(disc), ops.maven_disc_grads({k: torch.zeros_like(v) for k, v in disc.items()})
    mi_dq, ce, stats = torch.empty(B, T, N, A, device=dev), torch.empty(BT, device=dev), torch.zeros(2, device=dev)

    def head_fwd():
        ops.maven_head_fwd(w, hs, noise, q, B, T, N, A, K)

    def head_bwd():
        ops.maven_head_bwd(w, gw, hs, noise, u, dq_val, dq_dense, dq_out, dhs, B, T, N, A, K)

    def mi():
        ops.maven_mi(d, gd, q, avail, (T + 1) * N * A, state, SP, T + 1, emap, noise, padded, 0.001, mi_dq, ce, stats, B, T, N, A, S, K)

    # bytes that must move: the planes read and written once (weights and per-episode scalars are noise beside them)
    fwd_b = 4 * R * (H + 2 * A)
    bwd_b = 4 * R * (H + 1 + 1 + A + A + H)
    mi_b = 4 * (R * (A + A + A) + BT * (S + 2))
    for name, fn, nb in (("maven_head_fwd", head_fwd, fwd_b), ("maven_head_bwd", head_bwd, bwd_b), ("maven_mi", mi, mi_b)):
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
        print("  %-16s %s B=%d T=%d N=%d A=%d K=%d  %9.1f us   %8.1f MB, %8.1f us at 6.0 TB/s (%.2f of it)"
              % (name, o.shape, B, T, N, A, K, t, nb / 1e6, nb / HBM * 1e6, t / (nb / HBM * 1e6)), flush=True)
    print("  plan", ops.maven_plan(B, T, N, A, K, S), flush=True)


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
    if not o.skip_kernels:
        time_kernels(o)
        gc.collect()
        torch.cuda.empty_cache()
    if not o.skip_update:
        time_update(o)


if __name__ == "__main__":
    main()
