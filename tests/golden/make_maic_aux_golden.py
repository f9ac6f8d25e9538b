#!/usr/bin/env python3
"""MAIC auxiliary-loss fixtures: the REAL reference MAICAgent (network/MAIC.py) in float64 on the CPU, BatchNorm in training mode,
sampled latents, ``forward(..., train_mode=True)`` with mi_loss_weight = 0.001 and entropy_loss_weight = 0.01, and torch autograd
through its own forward.  Run in the build container only, with the reference checkout in MARL_REFERENCE:
    python tests/golden/make_maic_aux_golden.py
Per shape (2s3z, MMM2), bs = 6, weights tests/maic_oracle.py:maic_state (seed of maic_<shape>_inputs.npz):
    maic_<shape>_aux.npz   inputs, h0, the noise the reference drew, h, return_q, the two returned losses, the gradients of their
                           sum with respect to the GRU output h (dh) and to every parameter that receives one (grad/<name>), and
                           both BatchNorm modules' buffers after the call (buf/<name>)."""
import os
import sys

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_maic_golden as mg  # noqa: E402  (puts the repository, tests/ and the reference on sys.path)
import maic_oracle as mo  # noqa: E402
import maic_aux_oracle as ma  # noqa: E402

BS = 6


def gen_shape(shape):
    args = mo.maic_args(shape)
    args.device = "cpu"
    args.mi_loss_weight, args.entropy_loss_weight = ma.MI_W, ma.ENT_W
    N = args.n_agents
    seed = int(np.load(os.path.join(HERE, "maic_%s_inputs.npz" % shape))["seed"])
    agent, I = mg.build(args, seed)
    agent.train(True)
    rng = np.random.default_rng(400 + seed)
    x = rng.standard_normal((BS * N, I)).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((BS * N, 64))).astype(np.float32)
    kept = {}

    def keep_h(mod, inp, out):
        out.retain_grad()
        kept["h"] = out
    hook = agent.rnn.register_forward_hook(keep_h)
    th.manual_seed(7)
    with mg.CaptureNoise() as cap:
        rq, h, ret = agent(th.tensor(x, dtype=th.float64), th.tensor(h0, dtype=th.float64), BS, test_mode=False, train_mode=True)
    hook.remove()
    (ret["mi_loss"] + ret["entropy_loss"]).backward()
    eps = cap.drawn[0]
    assert th.equal(eps.float().double(), eps)
    out = dict(seed=np.array(seed), inputs=x, h0=h0, eps=eps.numpy().astype(np.float32), h=kept["h"].detach().numpy(),
               return_q=rq.detach().numpy(), mi_loss=np.array(float(ret["mi_loss"])),
               entropy_loss=np.array(float(ret["entropy_loss"])), dh=kept["h"].grad.numpy())
    for k, p in agent.named_parameters():
        if p.grad is not None:
            out["grad/" + k] = p.grad.numpy()
    for k, b in agent.named_buffers():
        out["buf/" + k] = b.detach().numpy()
    np.savez_compressed(os.path.join(HERE, "maic_%s_aux.npz" % shape), **out)
    print(shape, "written, seed", seed, "mi %.6e ent %.6e" % (float(ret["mi_loss"]), float(ret["entropy_loss"])),
          sorted(k for k in out if k.startswith("grad/")))


if __name__ == "__main__":
    for s in ("2s3z", "MMM2"):
        gen_shape(s)
