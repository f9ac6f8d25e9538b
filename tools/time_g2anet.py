#!/usr/bin/env python3
"""Cost of the G2ANet actor on one MI355X, in alternating rounds of one process:
  1. marl_g2anet_head_fwd and marl_g2anet_head_bwd alone (hard on and off) and marl_g2anet_noise, by HIP events, beside the forward's
     floor: 2 x (55.3 K + 24.6 K (N - 1)) FLOP per row at the fp32 MFMA peak (--peak_tflops, the microarchitecture guide's figure);
  2. the reinforce+g2anet update beside the reinforce update built from the same tree (host clock around a device synchronise;
     fixed-length episodes, f32 mode, eager launches - the set-up of tools/time_pg.py and tools/time_commnet.py).
Defaults: 2s3z and MMM2, T = 120, 4096 episodes, seven rounds."""
import argparse
import gc

import torch

from time_commnet import events, make, time_updates      # (puts the repository root on sys.path)


def one_shape(shape, o):
    from marl_amd import ops
    dev = torch.device("cuda")
    (ga, gmac, gl, gw), (pa, pmac, pl, pw) = make("g2anet", shape, o), make(None, shape, o)
    B, T, N, A, H = o.envs, ga.episode_limit, ga.n_agents, ga.n_actions, 64
    G, R = B * T, B * T * N
    # 1. the head alone
    hs, dl = torch.tanh(torch.randn(R, H, device=dev)), torch.randn(R, A, device=dev)
    logits, dhs = torch.empty(R, A, device=dev), torch.empty(R, H, device=dev)
    noise = torch.empty(B, T, N, N - 1, device=dev)
    ag = gmac.agent
    calls = {"noise": lambda: ops.g2anet_noise(1, 0, 0, noise, B, T, N)}
    for hard in (True, False):
        tag = "hard" if hard else "soft only"
        calls["head fwd " + tag] = lambda hard=hard: ops.g2anet_head_fwd(ag.head_weights(), hs, noise, logits, G, N, A, hard, gmac.tau)
        calls["head bwd " + tag] = lambda hard=hard: ops.g2anet_head_bwd(ag.head_weights(), ag.head_grads(), hs, noise, dl, dhs, G, N, A,
                                                                         hard, gmac.tau)
    head = events(calls, o.rounds, o.reps)
    floor_ms = 2.0 * (55.3e3 + 24.6e3 * (N - 1)) * R / (o.peak_tflops * 1e12) * 1e3
    for k, (med, lo, hi) in head.items():
        print("%-5s %-19s G %d x N %d, A %d  median %.2f ms (min %.2f - max %.2f, %d rounds of %d)"
              % (shape, k, G, N, A, med / 1e3, lo / 1e3, hi / 1e3, o.rounds, o.reps))
    print("%-5s head fwd floor at %.0f TFLOP/s fp32 MFMA: %.2f ms  (fwd hard / floor %.1f)"
          % (shape, o.peak_tflops, floor_ms, head["head fwd hard"][0] / 1e3 / floor_ms))
    del hs, dl, logits, dhs, noise
    if o.head_only:
        return
    # 2. the updates
    time_updates(shape, "reinforce+g2anet", o, gl, gw, pl, pw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--shapes", nargs="+", default=["2s3z", "MMM2"])
    ap.add_argument("--T", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--peak_tflops", type=float, default=157.3)
    ap.add_argument("--head_only", action="store_true", help="stop after the head's own timings")
    o = ap.parse_args()
    for shape in o.shapes:
        one_shape(shape, o)
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
