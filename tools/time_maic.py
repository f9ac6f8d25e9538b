#!/usr/bin/env python3
"""Cost of the MAIC message head (csrc/maic_head.hip) in the per-step rollout: HIP-event ms per lock-step of the fused_step
rollout with a MAICMAC (agent step + head + env step) and with the plain controller (no head), and the head launch alone, with
BatchNorm in eval mode (one launch) and in batch-statistics mode (three launches).  Evaluation rollouts: test-mode latents.
    python tools/time_maic.py [--shape 2s3z|MMM2] [--envs 512 4096 ...]
tools/time_rtw.py with the same arguments is the yardstick next to it.
    python tools/time_maic.py --train [--shape ...] [--envs ...] [--train_T 120]
times training instead: the head's backward alone (csrc/maic_head_bwd.hip, sampled latents, one call over envs * N rows) and one
MAICTDLearner update (qmix, BatchNorm in batch-statistics mode: one head call per transition index) beside a plain QLearner update
of the same shape, HIP events; and beside them the auxiliary pass alone (csrc/maic_aux.hip: the MI and entropy losses with their
gradients, one call over envs * N rows) and the update with both loss weights on (0.001 / 0.01)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import seeded  # noqa: E402
from marl_amd.common.arguments import get_maic_args  # noqa: E402
from marl_amd.controller.share_params import SharedMAC, MAICMAC  # noqa: E402
from marl_amd.rollout import RolloutWorker  # noqa: E402
from marl_amd.env.synthetic_smac import SyntheticSMACEnv  # noqa: E402


def rollout_ms(mac_cls, args, E, train=False):
    torch.manual_seed(0)
    mac = mac_cls(args)
    mac.cuda()
    mac.agent.train(train)
    env = SyntheticSMACEnv(E, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, args.episode_limit, seed=1,
                           fixed_length=True)
    w = RolloutWorker(env, mac, args)
    w.rollout_mode = "fused_step"
    w.generate_episodes(E, evaluate=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(3):
        w.generate_episodes(E, evaluate=True)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 3 / args.episode_limit, mac


def head_ms(mac, args, E, train):
    N, A = args.n_agents, args.n_actions
    dev = torch.device("cuda")
    h = torch.randn(E * N, 64, device=dev)
    q = torch.zeros(E * N, A, device=dev)
    mac.agent.train(train)
    for _ in range(3):
        mac.agent.head(h, q, E, True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(50):
        mac.agent.head(h, q, E, True)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 50


def _timed(fn, reps):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def head_bwd_ms(args, E, train):
    N, A = args.n_agents, args.n_actions
    dev = torch.device("cuda")
    mac = MAICMAC(args)
    mac.cuda()
    mac.agent.train(train)
    for p in mac.agent.parameters():
        p.grad = torch.zeros_like(p)
    h, dh = torch.randn(E * N, 64, device=dev), torch.empty(E * N, 64, device=dev)
    eps = torch.randn(E * N, N * args.latent_dim, device=dev)
    u = torch.randint(0, A, (E * N,), device=dev, dtype=torch.int32)
    v = torch.randn(E * N, device=dev)
    return _timed(lambda: mac.agent.head_backward(h, u, v, E, False, eps, dh), 20)


def aux_ms(args, E, train):
    N, A = args.n_agents, args.n_actions
    dev = torch.device("cuda")
    mac = MAICMAC(args)
    mac.cuda()
    mac.agent.train(train)
    for p in mac.agent.parameters():
        p.grad = torch.zeros_like(p)
    h, dh = torch.randn(E * N, 64, device=dev), torch.empty(E * N, 64, device=dev)
    eps = torch.randn(E * N, N * args.latent_dim, device=dev)
    q = torch.randn(E * N, A, device=dev)
    dpar = torch.empty(E * N, 2 * N * args.latent_dim, device=dev)
    out = torch.zeros(2, device=dev)
    return _timed(lambda: mac.agent.aux_backward(h, q, E, False, eps, dpar, dh, out[0:1], out[1:2]), 20)


def update_ms(args, E, maic):
    from marl_amd.algorithm.q_learner import QLearner
    from marl_amd.algorithm.maic_td_learner import MAICTDLearner
    from marl_amd.hostutil import DeviceBatch
    torch.manual_seed(0)
    mac = (MAICMAC if maic else SharedMAC)(args)
    learner = (MAICTDLearner if maic else QLearner)(mac, args)
    learner.graphs = None
    env = SyntheticSMACEnv(E, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, args.episode_limit, seed=1,
                           fixed_length=True)
    w = RolloutWorker(env, mac, args)
    w.rollout_mode = "fused_step"
    batch = w.generate_episodes(E)[0]
    db = DeviceBatch.from_record(batch.record, args, T=args.episode_limit)
    return _timed(lambda: learner.train(db, 1), 3)


def train_main(o):
    for E in o.envs:
        args = get_maic_args(seeded.make_args(o.shape, "qmix", episode_limit=o.train_T, seed=1))
        args.batch_size, args.buffer_size = E, E
        plain, maic = update_ms(args, E, False), update_ms(args, E, True)
        print("%-5s envs %5d T %d  head backward alone: eval %.3f ms, batch %.3f ms   update: QLearner %.2f ms, MAICTDLearner %.2f ms "
              "(x%.1f)" % (o.shape, E, o.train_T, head_bwd_ms(args, E, False), head_bwd_ms(args, E, True), plain, maic, maic / plain),
              flush=True)
        args.mi_loss_weight, args.entropy_loss_weight = 0.001, 0.01
        both = update_ms(args, E, True)
        print("%-5s envs %5d T %d  auxiliary pass alone: eval %.3f ms, batch %.3f ms   update with both loss weights on %.2f ms "
              "(x%.2f of the TD-only update)" % (o.shape, E, o.train_T, aux_ms(args, E, False), aux_ms(args, E, True), both,
                                                 both / maic), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="2s3z", choices=["2s3z", "MMM2"])
    ap.add_argument("--envs", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--T", type=int, default=20, help="lock-steps per timed rollout")
    ap.add_argument("--train", action="store_true", help="time the head backward and a MAICTDLearner update instead")
    ap.add_argument("--train_T", type=int, default=120, help="episode length of the timed update")
    o = ap.parse_args()
    if o.train:
        return train_main(o)
    for E in o.envs:
        args = get_maic_args(seeded.make_args(o.shape, "qmix", episode_limit=o.T, seed=1))
        base, _ = rollout_ms(SharedMAC, args, E)
        for train in (False, True):
            step, mac = rollout_ms(MAICMAC, args, E, train)
            print("%-5s envs %5d  BatchNorm %-5s per lock-step: no head %.3f ms  with head %.3f ms  (+%.3f)   head launch alone "
                  "%.3f ms" % (o.shape, E, "batch" if train else "eval", base, step, step - base, head_ms(mac, args, E, train)),
                  flush=True)


if __name__ == "__main__":
    main()
