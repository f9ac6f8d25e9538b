#!/usr/bin/env python3
"""RTW fixtures: run the REAL reference RTWAgent / RTWMAC / RolloutWorker (network/RTW.py, controller/share_params.py:612-804,
rollout.py:73-76) on seeded inputs and store what they compute.  Run in the build container only:
    python tests/golden/make_rtw_golden.py
The reference moves every tensor to the GPU with .cuda(); here Tensor.cuda / Module.cuda are no-ops so it runs on the CPU.
The serial environment's observations are returned as float32 (real SMAC does; the float64 lists of SerialSynthEnv would
make RTWAgent concatenate Double and Float).  Writes tests/golden/rtw_*.npz and copies the shipped QMIX model
model/qmix/2s3z/{rnn,mixer}_net_params.pkl (data) to tests/golden/ref_ckpt/qmix_rtw/."""
import os
import shutil
import sys
import types

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("MARL_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)
sys.argv = ["x"]
np.float = float
np.long = int
sys.modules.setdefault("gym", types.SimpleNamespace(Env=object))
th.Tensor.cuda = lambda self, *a, **k: self
th.nn.Module.cuda = lambda self, *a, **k: self

from oracle import seeded, rollout as orl  # noqa: E402
import rtw_oracle  # noqa: E402
from controller.share_params import RTWMAC  # noqa: E402  (reference)
from rollout import RolloutWorker  # noqa: E402  (reference)

th.set_num_threads(1)
CKPT = os.path.join(REF, "model", "qmix", "2s3z")


def rtw_args(shape, T, not_self=True, **over):
    a = seeded.make_args(shape, "qmix", episode_limit=T, **over)
    a.RTW = True
    a.world_loss_weight, a.teammate_loss_weight, a.hidden_dim, a.attn_dim = 1, 1, 64, 64
    a.not_self_model = not_self
    return a


class Float32Obs:
    def __init__(self, env):
        self.env = env

    def __getattr__(self, k):
        return getattr(self.env, k)

    def get_obs(self):
        return [np.asarray(o, dtype=np.float32) for o in self.env.get_obs()]


def act_case(mac, args, G, seed):
    """per row (env g, agent i): RTWAgent.forward(test_mode=True, agent_num=i) on seeded inputs; teammate logits and o_hat
    captured with forward hooks on teammate_net / world_net."""
    rng = np.random.default_rng(seed)
    N, A, O = args.n_agents, args.n_actions, args.obs_shape
    I = mac._get_input_shape()
    inp = rng.standard_normal((G, N, I)).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((G, N, 64))).astype(np.float32)
    obs = rng.standard_normal((G, N, O)).astype(np.float32)
    avail = (rng.random((G, N, A)) < 0.7).astype(np.float32)
    avail[..., 0] = 1.0
    cap = {}
    hk = [mac.agent.teammate_net.register_forward_hook(lambda m, i, o: cap.__setitem__("t", o.detach().clone())),
          mac.agent.world_net.register_forward_hook(lambda m, i, o: cap.__setitem__("w", o.detach().clone()))]
    q, h, ohat, act, gap = [], [], [], [], []
    with th.no_grad():
        for g in range(G):
            for i in range(N):
                qq, hh = mac.agent(th.tensor(inp[g, i:i + 1]), th.tensor(h0[g, i:i + 1]), th.tensor(obs[g, i:i + 1]), None, None,
                                   th.tensor(avail[g:g + 1]), test_mode=True, agent_num=i)
                t = cap["t"].view(N, A).clone()
                t[th.tensor(avail[g]) == 0.0] = -1e9
                top = t.topk(2, -1).values
                q.append(qq[0].numpy()); h.append(hh[0].numpy()); ohat.append(cap["w"][0].numpy())
                act.append(t.argmax(-1).numpy()); gap.append((top[:, 0] - top[:, 1]).numpy())
    for x in hk:
        x.remove()
    return dict(inp=inp, h0=h0, obs=obs, avail=avail, q=np.array(q), h=np.array(h), ohat=np.array(ohat),
                act=np.array(act, dtype=np.int32), gap=np.array(gap))


def pick_act(mac, args, G, seed0):
    for seed in range(seed0, seed0 + 200):
        c = act_case(mac, args, G, seed)
        if c["gap"].min() > 1e-4:
            c["seed"] = np.array(seed)
            return c
    raise RuntimeError("no seed with all teammate gaps > 1e-4")


def given_case(mac, args, B, T, seed, lengths):
    batch = seeded.make_batch(args, B, seed=seed, lengths=lengths)
    tb = {k: th.tensor(v, dtype=th.long if k == "u" else th.float32) for k, v in batch.items()}
    with th.no_grad():
        mac.init_hidden(B)
        q, h, l1, l2 = mac.get_current_q_values(tb, T)
    return dict(checksum=np.array(seeded.checksum(batch)), q=q.numpy(), h=h.numpy(), loss_t=np.array(float(l1)),
                loss_w=np.array(float(l2)))


def put(out, prefix, d):
    for k, v in d.items():
        out[prefix + "/" + k] = v


def main():
    dst = os.path.join(HERE, "ref_ckpt", "qmix_rtw")
    os.makedirs(dst, exist_ok=True)
    for kind in ("rnn_net", "mixer_net"):
        shutil.copyfile(os.path.join(CKPT, "%s_params.pkl" % kind), os.path.join(dst, "%s_params.pkl" % kind))
        os.chmod(os.path.join(dst, "%s_params.pkl" % kind), 0o644)

    # ---- shipped model, 2s3z: act mode, given mode, not_self_model on and off
    out = {}
    T = 5
    for tag, ns in (("self0", True), ("self1", False)):
        args = rtw_args("2s3z", T, not_self=ns)
        mac = RTWMAC(args)
        mac.load_models(os.path.join(CKPT, "rnn_net_params.pkl"))     # the reference's own loading call (:800-804)
        put(out, tag + "/act", pick_act(mac, args, 8, 100))
        put(out, tag + "/given", given_case(mac, args, 3, T, 700, [5, 3, -1]))
    np.savez_compressed(os.path.join(HERE, "rtw_2s3z_ckpt.npz"), **out)

    # ---- serial RolloutWorker with RTW on the synthetic env (shipped model)
    out = {}
    args = rtw_args("2s3z", 8)
    for tag, eps, evaluate in (("greedy", 0.0, True), ("eps05", 0.5, False)):
        args.epsilon = eps
        mac = RTWMAC(args)
        mac.load_models(os.path.join(CKPT, "rnn_net_params.pkl"))
        sy = orl.SynthSMAC(5, 80, 120, 11, 8, seed=5)
        w = RolloutWorker(Float32Obs(orl.SerialSynthEnv(sy)), mac, args)
        np.random.seed(9)
        ep, rew, wins, steps = w.generate_episodes(4, evaluate=evaluate)
        for k in ("o", "u", "r", "avail_u", "avail_u_next", "padded", "terminated"):
            out["%s/%s" % (tag, k)] = np.asarray(ep[k], dtype=np.float64)
        out[tag + "/rewards"] = np.array(rew)
        out[tag + "/wins"] = np.array(wins)
        out[tag + "/steps"] = np.array(steps)
        out[tag + "/eps_after"] = np.array(w.epsilon)
    np.savez_compressed(os.path.join(HERE, "rtw_serial.npz"), **out)

    # ---- MMM2 with seeded initial weights (state dict stored)
    out = {}
    args = rtw_args("MMM2", 4)
    mac = RTWMAC(args)
    sd = rtw_oracle.random_rtw_params(args, 11)
    mac.agent.load_state_dict({k: th.tensor(v) for k, v in sd.items()})
    put(out, "sd", sd)
    put(out, "act", pick_act(mac, args, 3, 200))
    put(out, "given", given_case(mac, args, 2, 4, 701, [4, 2]))
    np.savez_compressed(os.path.join(HERE, "rtw_MMM2.npz"), **out)
    print("wrote rtw_2s3z_ckpt.npz rtw_serial.npz rtw_MMM2.npz")


if __name__ == "__main__":
    main()
