#!/usr/bin/env python3
"""MAIC fixtures: run the REAL reference MAICAgent (network/MAIC.py) in float64 on seeded inputs and store what it computes.
Run in the build container only, with the reference checkout in MARL_REFERENCE:
    python tests/golden/make_maic_golden.py
Weights: tests/maic_oracle.py:maic_state (scale 3).  Per shape (2s3z, MMM2), bs = 37:
    maic_<shape>_inputs.npz              seed, inputs, h0, h, the state-dict key / shape list
    maic_<shape>_<test|samp>_<eval|batch>.npz   return_q, latent, alpha, msg, the running statistics after the call and, in
                                         sampled mode, the very noise the reference drew (torch.distributions.utils.
                                         _standard_normal wrapped while it runs; rounded to float32 so it is stored exactly)
    maic_serial.npz                      greedy serial episodes: SerialSynthEnv stepped by this script's loop
                                         (tests/maic_oracle.py:serial_rollout), the reference forward (bs = 1, test mode, eval)
                                         once per step
The alpha gate and the greedy argmax are discontinuous, so a seed is only accepted if the reference itself is clear of the
edges: no off-diagonal alpha within a relative 1e-4 of 0.25 / N, no two available Q values of a greedy choice within 1e-4 of
max|q|.  Otherwise the next seed is tried.  Nothing is left out of a fixture."""
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

import maic_oracle as mo  # noqa: E402
from oracle import rollout as orl  # noqa: E402
from network.MAIC import MAICAgent  # noqa: E402  (reference)
import torch.distributions.utils as tdu  # noqa: E402
import torch.distributions.normal as tdn  # noqa: E402

th.set_num_threads(1)
BS = 37
GATE_CLEAR, Q_CLEAR = 1e-4, 1e-4


def build(args, seed):
    I = args.obs_shape + args.n_actions + args.n_agents
    agent = MAICAgent(I, args).double()
    agent.load_state_dict(mo.p64(mo.maic_state(args, seed=seed)))
    return agent, I


class CaptureNoise:
    """records (and rounds to float32) what rsample draws"""

    def __enter__(self):
        self.drawn = []
        self.orig = tdu._standard_normal

        def wrapped(shape, dtype, device):
            z = self.orig(shape, dtype=dtype, device=device).float().to(dtype)
            self.drawn.append(z.clone())
            return z
        tdu._standard_normal = wrapped
        tdn._standard_normal = wrapped
        return self

    def __exit__(self, *a):
        tdu._standard_normal = self.orig
        tdn._standard_normal = self.orig


def gate_gap(alpha, N):
    """smallest relative distance of an off-diagonal pre-gate alpha to the threshold"""
    off = alpha[~np.broadcast_to(np.eye(N, dtype=bool), alpha.shape)]
    thr = 0.25 / N
    return float(np.abs(off - thr).min() / thr)


def gen_shape(shape):
    args = mo.maic_args(shape)
    N, A = args.n_agents, args.n_actions
    seed = mo.MAIC_SEED
    while True:
        agent, I = build(args, seed)
        rng = np.random.default_rng(100 + seed)
        x = rng.standard_normal((BS * N, I)).astype(np.float32)
        h0 = (0.5 * rng.standard_normal((BS * N, 64))).astype(np.float32)
        cases, ok = {}, True
        for test_mode in (True, False):
            for bn_train in (False, True):
                agent, _ = build(args, seed)          # fresh running statistics for every case
                agent.train(bn_train)
                th.manual_seed(7)
                with th.no_grad(), CaptureNoise() as cap:
                    rq, h, ret = agent(th.tensor(x, dtype=th.float64), th.tensor(h0, dtype=th.float64), BS, test_mode=test_mode)
                assert ret == {}
                eps = None if test_mode else cap.drawn[0]
                o = mo.forward(mo.p64(mo.maic_state(args, seed=seed)), th.tensor(x, dtype=th.float64),
                               th.tensor(h0, dtype=th.float64), BS, N, test_mode, bn_train, eps)
                assert float((o["return_q"] - rq).abs().max()) < 1e-10      # the restatement IS the reference
                if test_mode:
                    gap = gate_gap(pre_gate_alpha(o, args, seed, h, BS, N), N)
                    ok = ok and gap > GATE_CLEAR
                    print(shape, "seed", seed, "bn_train", bn_train, "gate gap %.2e" % gap, "zeroed %.0f %%" % (
                        100 * float((o["alpha"].numpy()[~np.broadcast_to(np.eye(N, dtype=bool), o["alpha"].shape)] == 0).mean())))
                bn = agent.embed_net[1]
                tag = ("test" if test_mode else "samp") + "_" + ("batch" if bn_train else "eval")
                c = dict(return_q=rq.numpy(), latent=o["latent"].numpy(), alpha=o["alpha"].numpy(), msg=o["msg"].numpy(),
                         running_mean=bn.running_mean.numpy().copy(), running_var=bn.running_var.numpy().copy(),
                         num_batches_tracked=np.array(int(bn.num_batches_tracked)))
                if eps is not None:
                    assert th.equal(eps.float().double(), eps)
                    c["eps"] = eps.numpy().astype(np.float32)
                cases[tag] = c
                h_out = h.numpy()
        if ok:
            break
        seed += 1
    keys = [(k, tuple(v.shape)) for k, v in agent.state_dict().items()]
    np.savez_compressed(os.path.join(HERE, "maic_%s_inputs.npz" % shape), seed=np.array(seed), inputs=x, h0=h0, h=h_out,
                        keys=np.array([k for k, _ in keys]), shapes=np.array([",".join(map(str, s)) for _, s in keys]))
    for tag, c in cases.items():
        np.savez_compressed(os.path.join(HERE, "maic_%s_%s.npz" % (shape, tag)), **c)
    print(shape, "written, seed", seed)


def pre_gate_alpha(o, args, seed, h, bs, N):
    """alpha before the gate, from the latent and hidden state of the case"""
    p = mo.p64(mo.maic_state(args, seed=seed))
    key = th.nn.functional.linear(h, p["w_key.weight"], p["w_key.bias"]).view(bs, N, 1, -1) / np.sqrt(mo.D)
    q = th.nn.functional.linear(o["latent"].reshape(bs, N, N, mo.L), p["w_query.weight"], p["w_query.bias"])
    logits = (key * q).sum(-1)
    logits[:, np.arange(N), np.arange(N)] = -1e9
    return th.softmax(logits, -1).numpy()


def gen_serial():
    args = mo.maic_args("2s3z", episode_limit=8)
    N = args.n_agents
    seed = mo.MAIC_SEED
    while True:
        agent, _ = build(args, seed)
        agent.eval()

        def fwd(inp, h):
            with th.no_grad():
                q, h2, _ = agent(inp, h, 1, test_mode=True)
            return q, h2
        env = orl.SerialSynthEnv(orl.SynthSMAC(5, 80, 120, 11, 8, seed=5))
        ep, rew, wins, steps = mo.serial_rollout(fwd, args, env, 6)
        gap = float(ep["qmax_gap"].min())
        print("serial seed", seed, "smallest greedy gap / max|q| %.2e" % gap)
        if gap > Q_CLEAR:
            break
        seed += 1
    out = {k: v for k, v in ep.items()}
    out.update(seed=np.array(seed), rewards=np.array(rew), wins=np.array(wins), steps=np.array(steps))
    np.savez_compressed(os.path.join(HERE, "maic_serial.npz"), **out)
    print("maic_serial written")


if __name__ == "__main__":
    for s in ("2s3z", "MMM2"):
        gen_shape(s)
    gen_serial()
