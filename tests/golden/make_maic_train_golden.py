#!/usr/bin/env python3
"""MAIC training fixtures: the REAL reference MAICAgent (network/MAIC.py) in float64, BatchNorm in training mode, sampled
latents, and torch autograd through its own forward.  Run in the build container only, with the reference checkout in
MARL_REFERENCE:
    python tests/golden/make_maic_train_golden.py
Per shape (2s3z, MMM2), bs = 6, weights tests/maic_oracle.py:maic_state (seed of maic_<shape>_inputs.npz):
    maic_<shape>_train_grad.npz   inputs, h0, the weights G, the noise the reference drew (torch reseeded as for the samp fixtures),
                                  and the gradients of sum(return_q * G): dh with respect to the GRU output h (the fc2 path
                                  included: return_q = fc2(h) + messages) and grad/<name> for every head parameter."""
import os
import sys

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_maic_golden as mg  # noqa: E402  (puts the repository, tests/ and the reference on sys.path)
import maic_oracle as mo  # noqa: E402
import maic_train_oracle as mt  # noqa: E402

BS = 6


def gen_shape(shape):
    args = mo.maic_args(shape)
    N, A = args.n_agents, args.n_actions
    seed = int(np.load(os.path.join(HERE, "maic_%s_inputs.npz" % shape))["seed"])
    agent, I = mg.build(args, seed)
    agent.train(True)
    rng = np.random.default_rng(300 + seed)
    x = rng.standard_normal((BS * N, I)).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((BS * N, 64))).astype(np.float32)
    G = rng.standard_normal((BS * N, A)).astype(np.float32)
    kept = {}

    def keep_h(mod, inp, out):
        out.retain_grad()
        kept["h"] = out
    hook = agent.rnn.register_forward_hook(keep_h)
    th.manual_seed(7)
    with mg.CaptureNoise() as cap:
        rq, h, ret = agent(th.tensor(x, dtype=th.float64), th.tensor(h0, dtype=th.float64), BS, test_mode=False)
    hook.remove()
    (rq * th.tensor(G, dtype=th.float64)).sum().backward()
    eps = cap.drawn[0]
    assert th.equal(eps.float().double(), eps)
    out = dict(seed=np.array(seed), inputs=x, h0=h0, G=G, eps=eps.numpy().astype(np.float32), h=kept["h"].detach().numpy(),
               return_q=rq.detach().numpy(), dh=kept["h"].grad.numpy())
    for k, p in agent.named_parameters():
        if mt.is_head_param(k):
            out["grad/" + k] = p.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "maic_%s_train_grad.npz" % shape), **out)
    print(shape, "written, seed", seed, {k: v.shape for k, v in out.items() if k.startswith("grad/")})


if __name__ == "__main__":
    for s in ("2s3z", "MMM2"):
        gen_shape(s)
