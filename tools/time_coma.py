#!/usr/bin/env python3
"""Cost of COMA on one MI355X: the COMALearner update beside the CentralVLearner update built from the same tree
(alternating rounds, host clock around a device synchronise, the set-up of tools/time_central_v.py: fixed-length episodes, f32 mode,
eager launches), and the critic's factored first layer (csrc/coma.hip: forward + backward, with the two block products and their
weight gradients) beside marl_linear / marl_linear_wgrad over a materialised (R, K) input, by HIP events in alternating rounds, at
``--fc1_envs`` episodes (a size at which the materialised input fits)."""
import argparse
import gc
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def time_fc1(ops, B, T, N, A, S, O, D, rounds, reps):
    dev = torch.device("cuda")
    BT, R, C, K = B * T, B * T * N, 2 * N * A + N, S + O + 2 * N * A + N
    g = torch.Generator(device=dev).manual_seed(0)
    W = (torch.rand(D, K, device=dev, generator=g) - 0.5) / K ** 0.5
    b = torch.zeros(D, device=dev)
    s, o = torch.randn(BT, S, device=dev, generator=g), torch.randn(R, O, device=dev, generator=g)
    u = torch.randint(0, A, (B, T, N), device=dev, generator=g, dtype=torch.int32)
    dh1 = torch.randn(R, D, device=dev, generator=g)
    wt, pre_s, h1, dpre, dsum = (torch.empty(n, D, device=dev) for n in (C, BT, R, R, BT))
    dW, db = torch.zeros(D, K, device=dev), torch.zeros(D, device=dev)
    uf = u.reshape(-1)

    def factored():
        ops.coma_onehot_cols(W, S + O, wt, C, D)
        ops.linear(ops.src(s), W[:, :S], b, pre_s, BT, D, S, ldw=K)
        ops.linear(ops.src(o), W[:, S:S + O], None, h1, R, D, O, ldw=K)
        ops.coma_fc1_fwd(pre_s, wt, uf, h1, B, T, N, A, D)
        ops.coma_fc1_bwd(dh1, h1, uf, dpre, dsum, dW, S + O, B, T, N, A, D)
        ops.linear_wgrad(dsum, ops.src(s), dW[:, :S], db, BT, D, S, lddw=K)
        ops.linear_wgrad(dpre, ops.src(o), dW[:, S:S + O], None, R, D, O, lddw=K)

    # the materialised input (built once, outside the clock: the composition is charged for its products alone)
    ul = u.long()
    acts = torch.nn.functional.one_hot(ul, A).float()                                   # (B, T, N, A)
    x = torch.zeros(B, T, N, K, device=dev)
    x[..., :S] = s.view(B, T, 1, S)
    x[..., S:S + O] = o.view(B, T, N, O)
    for i in range(N):
        blk = acts.clone()
        blk[:, :, i] = 0
        x[:, :, i, S + O:S + O + N * A] = blk.reshape(B, T, N * A)
    x[:, 1:, :, S + O + N * A:S + O + 2 * N * A] = acts[:, :-1].reshape(B, T - 1, 1, N * A)
    x[..., S + O + 2 * N * A:] = torch.eye(N, device=dev)
    x = x.view(R, K)
    del acts
    y = torch.empty(R, D, device=dev)

    def materialised():
        ops.linear(ops.src(x), W, b, y, R, D, K, act=1)
        ops.linear_wgrad(dh1, ops.src(x), dW, db, R, D, K, Yact=y)

    factored(); materialised()
    torch.cuda.synchronize()
    err = float((h1 - y).abs().max())
    calls = {"factored": factored, "materialised": materialised}
    times = {k: [] for k in calls}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for k, f in calls.items():
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / reps)
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print("fc1 %-12s rows %d  K %d  median %.3f ms  (min %.3f - max %.3f)   forward + backward" % (k, R, K, med[k], min(v), max(v)))
    print("fc1 factored / materialised = %.3f   (input of the materialised form: %.2f GB; max |h1 difference| %.2e)"
          % (med["factored"] / med["materialised"], R * K * 4 / 1e9, err))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--fc1_envs", type=int, default=1024)
    ap.add_argument("--shape", default="2s3z")
    ap.add_argument("--T", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--fc1_reps", type=int, default=5)
    o = ap.parse_args()
    from marl_amd import ops
    from marl_amd.controller.share_params import PolicyMAC
    from marl_amd.algorithm.central_v import CentralVLearner
    from marl_amd.algorithm.coma import COMALearner
    from marl_amd.common.arguments import get_centralv_args, get_coma_args
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv

    def make(alg):
        args = bench.make_args(alg, o.shape, o.T)
        args.gemm_mode, args.hip_graph = "f32", False
        (get_coma_args if alg == "coma" else get_centralv_args)(args)
        torch.manual_seed(0)
        mac = PolicyMAC(args)
        learner = (COMALearner if alg == "coma" else CentralVLearner)(mac, args)
        env = SyntheticSMACEnv(o.envs, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, args.episode_limit,
                               seed=1, fixed_length=True)
        w = RolloutWorker(env, mac, args)
        w.rollout_mode = "unfused"
        return args, learner, w

    (ca, cl, cw), (va, vl, vw) = make("coma"), make("central_v")
    ep_c, ep_v = cw.generate_episodes(o.envs)[0], vw.generate_episodes(o.envs)[0]
    steps = {"coma": lambda i: cl.train(ep_c, i, epsilon=cw.epsilon), "central_v": lambda i: vl.train(ep_v, i, epsilon=vw.epsilon)}
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
    med = {k: statistics.median(r) for k, r in rates.items()}
    for k, r in rates.items():
        print("%-10s update  %s  envs %d  T %d  median %.2f ms  (min %.2f - max %.2f)" % (k, o.shape, o.envs, ca.episode_limit, med[k], min(r), max(r)))
    print("update coma / central_v = %.2f" % (med["coma"] / med["central_v"]))
    gc.enable()
    del cl, vl, cw, vw, ep_c, ep_v, steps
    gc.collect()
    torch.cuda.empty_cache()
    time_fc1(ops, o.fc1_envs, ca.episode_limit, ca.n_agents, ca.n_actions, ca.state_shape, ca.obs_shape, ca.critic_dim, o.rounds,
             o.fc1_reps)


if __name__ == "__main__":
    main()
