#!/usr/bin/env python3
"""World-model fixtures: run the REAL reference SharedMACWithState / QLearnerWithState (controller/share_params.py:185-387,
algorithm/q_learner_state.py) on seeded inputs and store what they compute.  Run in the build container only:
    python tests/golden/make_world_golden.py
Tensor.cuda / Module.cuda are no-ops so the reference runs on the CPU (as make_rtw_golden.py).  Weights: oracle.seeded for
the agent and the mixer, tests/world_oracle.py:world_param_shapes with seed WORLD_SEED for world.*.  Pins as make_golden.py:
norms and strided samples of the gradients and parameters after steps 0 and 1, the losses of TRAIN_STEPS, loss_pred through a
spy, the target agent after every step, the forward q, r, o_hat, tau of both passes, get_q_and_q_tot_table and one serial
rollout.  Writes tests/golden/world_*.npz."""
import os
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

from oracle import seeded  # noqa: E402
import world_oracle as wo  # noqa: E402
from controller.share_params import SharedMACWithState  # noqa: E402  (reference)
from algorithm.q_learner_state import QLearnerWithState  # noqa: E402  (reference)

th.set_num_threads(1)


def load(module, state):
    module.load_state_dict({k: th.tensor(v) for k, v in state.items()})


def pin(prefix, named, out):
    for name, t in named:
        if t is None:
            out["%s/%s/none" % (prefix, name)] = np.array(1)
            continue
        a = t.detach().cpu().numpy().astype(np.float64).ravel()
        out["%s/%s/norm" % (prefix, name)] = np.array(np.sqrt((a * a).sum()))
        out["%s/%s/samp" % (prefix, name)] = a[seeded.sample_indices(a.size)].astype(np.float32)


def named_params(learner):
    out = [("agent." + k, p) for k, p in learner.eval_net.agent.named_parameters()]
    return out + [("mixer." + k, p) for k, p in learner.mixer.named_parameters()]


def gen_case(case):
    name, shape, alg, B, T, lengths, over = case
    args, agent, mixer = wo.case_states(case)
    mac = SharedMACWithState(args)
    load(mac.agent, agent)
    learner = QLearnerWithState(mac, args)
    if mixer:
        load(learner.mixer, mixer)
        load(learner.target_mixer, mixer)
    out = {"meta/B": np.array(B), "meta/T": np.array(T), "meta/lengths": np.array(lengths)}
    batch = seeded.make_batch(args, B, seed=100, lengths=lengths)
    out["meta/batch_checksum"] = np.array(seeded.checksum(batch))
    tb = {k: th.tensor(v, dtype=th.long if k == "u" else th.float32) for k, v in batch.items()}
    with th.no_grad():
        mac.init_hidden(B)
        q, ret = mac.get_current_q_values(tb, T)
        out["fwd/q_cur"], out["fwd/h_cur"] = q.numpy(), ret["ep_hidden_states"].numpy()
        for k in ("r", "o_next", "terminated"):
            out["fwd/cur_" + k] = ret[k].numpy()
        mac.init_hidden(B)
        q, ret = mac.get_next_q_values(tb, T)
        out["fwd/q_next"], out["fwd/r_next"] = q.numpy(), ret["r"].numpy()

    captured = {}
    orig_clip, orig_mean = th.nn.utils.clip_grad_norm_, th.Tensor.mean

    def spy(params, max_norm, *a, **k):
        params = list(params)
        captured["grads"] = [None if p.grad is None else p.grad.detach().clone() for p in params]
        captured["norm"] = orig_clip(params, max_norm, *a, **k)
        return captured["norm"]

    def mean_spy(self, *a, **k):        # the one .mean() of train() is loss_pred (q_learner_state.py:181)
        v = orig_mean(self, *a, **k)
        captured["pred"] = float(v.detach())
        return v

    th.nn.utils.clip_grad_norm_ = spy
    th.Tensor.mean = mean_spy
    try:
        losses, preds = [], []
        for i, ts in enumerate(wo.TRAIN_STEPS):
            b = seeded.make_batch(args, B, seed=100 + i, lengths=lengths)
            losses.append(learner.train(b, ts))
            preds.append(captured["pred"])
            names = [n for n, _ in named_params(learner)]
            assert len(names) == len(captured["grads"])
            if i <= 1:
                pin("step%d/grad" % i, list(zip(names, captured["grads"])), out)
                pin("step%d/param" % i, named_params(learner), out)
            out["step%d/grad_norm" % i] = np.array(float(captured["norm"]))
            pin("step%d/target_agent" % i, [("agent." + k, p) for k, p in learner.target_net.agent.named_parameters()], out)
        out["losses"] = np.array(losses, dtype=np.float64)
        out["loss_pred"] = np.array(preds, dtype=np.float64)
        out["meta/T_used"] = np.array(learner.max_episode_len)
    finally:
        th.nn.utils.clip_grad_norm_ = orig_clip
        th.Tensor.mean = orig_mean
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(name, "losses", losses, "pred", preds)


def gen_matrix_table():
    """get_q_and_q_tot_table (q_learner_state.py:211-262) for vdn / qmix / qplex on the matrix game"""
    out = {}
    for alg in ("vdn", "qmix", "qplex"):
        case = ("x", "matrix", alg, 1, 1, [1], {})
        args, agent, mixer = wo.case_states(case)
        mac = SharedMACWithState(args)
        load(mac.agent, agent)
        learner = QLearnerWithState(mac, args)
        if mixer:
            load(learner.mixer, mixer)
        qt, qi, qj = learner.get_q_and_q_tot_table()
        out[alg + "/q_tot"], out[alg + "/q_i"], out[alg + "/q_j"] = np.asarray(qt), np.asarray(qi), np.asarray(qj)
    np.savez_compressed(os.path.join(HERE, "world_matrix_table.npz"), **out)
    print("world_matrix_table written")


def gen_serial():
    """the reference RolloutWorker's serial loop (rollout.py:30-173) with SharedMACWithState.choose_action (:214-260) on the
    synthetic env, greedy and epsilon = 0.5 (the numpy draw order): 4 episodes of 2s3z, T = 8"""
    from oracle import rollout as orl
    from rollout import RolloutWorker  # (reference)
    out = {}
    args = seeded.make_args("2s3z", "qmix", episode_limit=8)
    for tag, eps, evaluate in (("greedy", 0.0, True), ("eps05", 0.5, False)):
        args.epsilon = eps
        mac = SharedMACWithState(args)
        load(mac.agent, wo.serial_agent_state(args))
        w = RolloutWorker(orl.SerialSynthEnv(orl.SynthSMAC(5, 80, 120, 11, 8, seed=5)), mac, args)
        np.random.seed(9)
        ep, rew, wins, steps = w.generate_episodes(4, evaluate=evaluate)
        for k in ("o", "u", "r", "avail_u", "avail_u_next", "padded", "terminated"):
            out["%s/%s" % (tag, k)] = np.asarray(ep[k], dtype=np.float64)
        out[tag + "/rewards"] = np.array(rew)
        out[tag + "/wins"] = np.array(wins)
        out[tag + "/steps"] = np.array(steps)
        out[tag + "/eps_after"] = np.array(w.epsilon)
    np.savez_compressed(os.path.join(HERE, "world_serial.npz"), **out)
    print("world_serial written")


if __name__ == "__main__":
    for c in wo.CASES:
        gen_case(c)
    gen_matrix_table()
    gen_serial()
