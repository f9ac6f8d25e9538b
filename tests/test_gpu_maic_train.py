"""MAIC training on the MI355X: the message head's backward (csrc/maic_head_bwd.hip) and MAICTDLearner against the float64
oracle (tests/maic_train_oracle.py) in both gemm modes, bitwise repeatability, target copies with the BatchNorm buffers, resume
and model files, the Runner with --MAIC_train and the refusals.

Bounds: tests/parity.close at 1e-4 * max|ref| for every tensor; only the two gradients that are zero analytically (w_query.bias:
the softmax's d logits sum to zero; embed_net.0.bias under batch statistics), whose max|ref| is rounding, are bounded by 4 x the
float32 oracle's own error on that tensor (maic_train_oracle.bound_scale, figures in DESIGN section 10)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import learners
import parity
import maic_oracle as mo
import maic_train_oracle as mt

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _t(d):
    return {k: torch.tensor(np.asarray(v)) for k, v in d.items()}


def _close(case, name, got, ref64, ref32, bn_batch=False):
    """name: "<what> <parameter>" or a scalar's name; the parameter decides whether the zero-gradient bound applies"""
    kind, _, param = name.rpartition(" ")
    scale = mt.bound_scale(param, bn_batch, ref64, ref32) if kind == "grad" else None
    parity.close(case, name, got, ref64, scale=scale)


# ---------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("case", mt.HEAD_CASES, ids=[mt.head_case_id(c) for c in mt.HEAD_CASES])
def test_head_backward_matches_oracle(case):
    """dh and every weight gradient; += over two calls; the running statistics stay where they are"""
    from marl_amd import ops
    shape, bs, test_mode, bn = case
    args, state, h, q, eps, u_act, dq_val = mt.head_case_inputs(case)
    N, A = args.n_agents, args.n_actions
    r64 = mt.head_grads(state, h, q, eps, u_act, dq_val, bs, N, test_mode, bn)
    r32 = mt.head_grads(state, h, q, eps, u_act, dq_val, bs, N, test_mode, bn, dtype=torch.float32)
    dev = {k: v.to(DEV).contiguous() for k, v in _t(state).items()}
    before = {k: dev[mo.BN + k].clone() for k in mt.BUFFERS}
    g = {k: torch.zeros_like(v) for k, v in dev.items() if mt.is_head_param(k)}
    hd, epsd = torch.tensor(h, device=DEV), torch.tensor(eps, device=DEV)
    ud, vd = torch.tensor(u_act, device=DEV), torch.tensor(dq_val, device=DEV)
    dh = torch.full((bs * N, 64), 7.0, device=DEV)
    kw = dict(test_mode=test_mode, bn_batch=bn, eps=None if test_mode else epsd)
    ops.maic_head_bwd(ops.maic_weights(dev), ops.maic_grads(g), hd, ud, vd, dh, bs, N, A, **kw)
    c = "maic_head_bwd_" + mt.head_case_id(case)
    _close(c, "dh", dh.cpu().numpy(), r64["dh"], r32["dh"])
    for k in g:
        _close(c, "grad " + k, g[k].cpu().numpy(), r64["grads"][k], r32["grads"][k], bn)
    for k in mt.BUFFERS:
        assert torch.equal(dev[mo.BN + k], before[k]), k
    # a second call accumulates: twice the first, bit for bit (x + x is exact), and writes the same dh
    first = {k: v.clone() for k, v in g.items()}
    dh2 = torch.zeros_like(dh)
    ops.maic_head_bwd(ops.maic_weights(dev), ops.maic_grads(g), hd, ud, vd, dh2, bs, N, A, **kw)
    assert torch.equal(dh, dh2)
    for k in g:
        assert torch.equal(g[k], 2 * first[k]), k
    for k in mt.BUFFERS:
        assert torch.equal(dev[mo.BN + k], before[k]), k


def test_unsupported_shapes_raise_before_any_launch():
    from marl_amd import ops
    h, dh = torch.zeros(17, 64, device=DEV), torch.zeros(17, 64, device=DEV)
    u, v = torch.zeros(17, dtype=torch.int32, device=DEV), torch.zeros(17, device=DEV)
    with pytest.raises(ValueError):
        ops.maic_head_bwd(None, None, h, u, v, dh, 1, 17, 11, test_mode=True)
    with pytest.raises(ValueError):
        ops.maic_head_bwd(None, None, h, u, v, dh, 1, 5, 33, test_mode=True)
    with pytest.raises(ValueError):
        ops.maic_head_bwd(None, None, h, u, v, dh, 1, 5, 11, test_mode=False)            # sampled latents without eps
    with pytest.raises(ValueError):
        ops.maic_head_bwd(None, None, h[:1], u[:1], v[:1], dh[:1], 1, 1, 11, test_mode=True, bn_batch=True)


# ---------------------------------------------------------------------------------------------------- the learner
def build_product(case, gemm_mode=None):
    from marl_amd.controller.share_params import MAICMAC
    from marl_amd.algorithm.maic_td_learner import MAICTDLearner
    args, agent, mixer = mt.update_case_states(case)
    args.cuda = True
    if gemm_mode is not None:
        args.gemm_mode = gemm_mode
    mac = MAICMAC(args)
    mac.agent.load_state_dict(_t(agent), strict=True)
    mac.agent.train(case[6])
    learner = MAICTDLearner(mac, args)
    if mixer:
        learner.mixer.load_state_dict(_t(mixer))
        learner.target_mixer.load_state_dict(_t(mixer))
    return args, mac, learner


def named_product_params(learner):
    out = [("agent." + k, p) for k, p in learner.eval_net.agent.named_parameters()]
    return out + [("mixer." + k, p) for k, p in learner.mixer.named_parameters()]


_ORACLE = {}


def oracle_update(case):
    """the float64 and the float32 oracle's first update of a case, computed once"""
    if case[0] not in _ORACLE:
        _ORACLE[case[0]] = mt.reference_update(case)
    return _ORACLE[case[0]]


@pytest.mark.parametrize("case", mt.UPDATE_CASES, ids=[c[0] for c in mt.UPDATE_CASES])
def test_one_update_matches_oracle(case, gemm_mode):
    """loss, every gradient, the grad norm, the parameters after step 0 and the BatchNorm buffers; inference_net untouched"""
    name, shape, alg, B, T, lengths, bn_train = case[:7]
    o64, o32 = oracle_update(case)
    args, mac, learner = build_product(case, gemm_mode)
    batch, eps = mt.update_case_data(case)
    inf0 = {k: v.detach().clone() for k, v in learner.eval_net.agent.inference_net.named_parameters()}
    loss = learner.train(learners.clone_batch(batch), 0, eps=eps)
    c = "maic_update:%s[%s]" % (name, gemm_mode)
    assert learner.max_episode_len == o64["T"]
    _close(c, "loss", loss, o64["loss"], o32["loss"])
    den = float(learner.last_stats.cpu().numpy()[1])
    named = named_product_params(learner)
    for n, p in named:
        g = p.grad.detach().cpu().numpy() / den
        if n.startswith("agent.inference_net."):
            assert not g.any(), n
            assert torch.equal(p.detach(), inf0[n[len("agent.inference_net."):]]), n
            continue
        _close(c, "grad " + n, g, o64["grads"][n], o32["grads"][n], bn_train)
    gn = float(torch.sqrt(learner.optimizer.sumsq[0]).item()) / den
    _close(c, "grad_norm", gn, o64["grad_norm"], o32["grad_norm"])
    for n, p in named:
        if n.startswith("agent.inference_net."):
            continue
        keep = mt.step_is_decided(n, o64["grads"])
        _close(c, "param " + n, p.detach().cpu().numpy()[keep], o64["params"][n][keep], o32["params"][n][keep])
    for tag, net in (("eval", learner.eval_net), ("target", learner.target_net)):
        bufs = dict(net.agent.named_buffers())
        for k in mt.BUFFERS[:2]:
            _close(c, "%s %s" % (tag, k), bufs[mo.BN + k].cpu().numpy(), o64["bn_" + tag][mo.BN + k], o32["bn_" + tag][mo.BN + k])
        assert int(bufs[mo.BN + "num_batches_tracked"]) == int(o64["bn_" + tag][mo.BN + "num_batches_tracked"])
        # inference_net's BatchNorm is never evaluated
        assert int(bufs["inference_net.1.num_batches_tracked"]) == 3


def _update_bits(case, steps=(0,), hook=None):
    args, mac, learner = build_product(case)
    batch, eps = mt.update_case_data(case)
    out = []
    for ts in steps:
        loss = learner.train(learners.clone_batch(batch), ts, eps=eps)
        out.append((loss, learner._flat.flat.detach().cpu().numpy().copy(), learner._flat.gradx.detach().cpu().numpy().copy(),
                    {k: b.detach().cpu().numpy().copy() for k, b in learner.eval_net.agent.named_buffers()}))
    return learner, out


@pytest.mark.parametrize("case", [mt.UPDATE_CASES[0], mt.UPDATE_CASES[4]], ids=["batch", "eval"])
def test_two_identical_updates_give_the_same_bits(case):
    (_, a), (_, b) = _update_bits(case), _update_bits(case)
    assert a[0][0] == b[0][0]
    np.testing.assert_array_equal(a[0][1], b[0][1])
    np.testing.assert_array_equal(a[0][2], b[0][2])
    for k in a[0][3]:
        np.testing.assert_array_equal(a[0][3][k], b[0][3][k])


def test_own_noise_is_seeded_from_args():
    """without eps the draws come from the learner's generator: the same seed gives the same update, another seed another one"""
    case = mt.UPDATE_CASES[0]
    res = []
    for seed in (5, 5, 6):
        args, mac, learner = build_product(case)
        learner._gen.manual_seed(seed)
        batch, _ = mt.update_case_data(case)
        res.append(learner.train(learners.clone_batch(batch), 0))
    assert res[0] == res[1] and res[0] != res[2] and np.isfinite(res[2])


def test_target_sync_copies_the_buffers_and_resume_reproduces_the_next_update(tmp_path):
    case = mt.UPDATE_CASES[0]
    args, mac, learner = build_product(case)
    args.target_update_cycle = learner.args.target_update_cycle = 2
    batch, eps = mt.update_case_data(case)
    for ts in (0, 1):
        learner.train(learners.clone_batch(batch), ts, eps=eps)
    e, t = dict(learner.eval_net.agent.named_buffers()), dict(learner.target_net.agent.named_buffers())
    assert not torch.equal(e[mo.BN + "running_mean"], t[mo.BN + "running_mean"])
    learner.train(learners.clone_batch(batch), 2, eps=eps)              # train_step = target_update_cycle
    assert torch.equal(learner.target_net.agent._flat.flat, learner.eval_net.agent._flat.flat)
    assert torch.equal(learner.target_mixer._flat.flat, learner.mixer._flat.flat)
    for k, b in learner.target_net.agent.named_buffers():
        assert torch.equal(b, e[k]), k
    # full resume into a fresh learner: the next update is the same, bit for bit
    path = str(tmp_path / "resume.pt")
    learner.save_resume(path)
    args2, mac2, learner2 = build_product(case)
    learner2.args.target_update_cycle = 2
    learner2.load_resume(path)
    b2, eps2 = mt.update_case_data(case, batch_seed=101)
    la = learner.train(learners.clone_batch(b2), 3, eps=eps2)
    lb = learner2.train(learners.clone_batch(b2), 3, eps=eps2)
    assert la == lb
    assert torch.equal(learner._flat.flat, learner2._flat.flat)
    for (k, x), (_, y) in zip(learner.eval_net.agent.named_buffers(), learner2.eval_net.agent.named_buffers()):
        assert torch.equal(x, y), k


def test_model_files_roundtrip(tmp_path):
    """save_models / load_models carry the parameters and the BatchNorm buffers: the loaded controller evaluates the same"""
    case = mt.UPDATE_CASES[0]
    args, mac, learner = build_product(case)
    learner.model_dir = str(tmp_path)
    batch, eps = mt.update_case_data(case)
    learner.train(learners.clone_batch(batch), 0, eps=eps)
    learner.save_models(0)
    for kind in ("rnn_net", "mixer_net"):
        os.replace(learner.model_dir + "/0_%s_params.pkl" % kind, learner.model_dir + "/%s_params.pkl" % kind)
    args2, mac2, learner2 = build_product(case)
    learner2.model_dir = learner.model_dir
    learner2.load_models()
    T, B = case[4], case[3]
    for m in (mac, mac2):
        m.agent.eval()
        m.init_hidden(B)
    assert torch.equal(mac.get_current_q_values(batch, T, test_mode=True)[0], mac2.get_current_q_values(batch, T, test_mode=True)[0])


def test_refuses_a_multi_rank_reducer_and_a_plain_controller(monkeypatch):
    from marl_amd.algorithm import common
    from marl_amd.algorithm.maic_td_learner import MAICTDLearner
    from marl_amd.controller.share_params import SharedMAC, MAICMAC
    args, agent, mixer = mt.update_case_states(mt.UPDATE_CASES[0])
    args.cuda = True
    with pytest.raises(TypeError):
        MAICTDLearner(SharedMAC(args), args)

    class Ranked(common.GradReducer):
        def __init__(self, group=None):
            super().__init__(group)
            self.enabled = True

        def broadcast_(self, *tensors, src=0):
            pass
    monkeypatch.setattr(common, "GradReducer", Ranked)
    with pytest.raises(NotImplementedError):
        MAICTDLearner(MAICMAC(args), args)
    learner = MAICTDLearner.__new__(MAICTDLearner)
    with pytest.raises(NotImplementedError):
        learner.get_q_and_q_tot_table()


def test_runner_trains_and_the_saved_model_evaluates(tmp_path):
    from marl_amd.main import build
    from marl_amd.runner import Runner
    from marl_amd.utils.logging import Logger
    from marl_amd.controller.share_params import MAICMAC
    from marl_amd.algorithm.maic_td_learner import MAICTDLearner
    common = ["--alg", "qmix", "--map", "2s3z", "--n_envs", "16", "--MAIC", "True", "--evaluate_epoch", "1",
              "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "m")]
    args, env = build(common + ["--MAIC_train", "True", "--n_steps", "1500", "--evaluate_cycle", "100000"])
    args.train_steps = 3
    runner = Runner(env, Logger(), args)
    assert isinstance(runner.mac, MAICMAC) and isinstance(runner.learner, MAICTDLearner)
    before = runner.learner._flat.flat.clone()
    loss = runner.run(0)
    assert runner.train_steps >= 3 and np.isfinite(float(loss))
    assert not torch.equal(runner.learner._flat.flat, before)
    runner.learner.save_models(0)
    mdir = tmp_path / "m" / "qmix" / "2s3z"
    os.rename(mdir / "0_rnn_net_params.pkl", mdir / "rnn_net_params.pkl")
    os.rename(mdir / "0_mixer_net_params.pkl", mdir / "mixer_net_params.pkl")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "marl_amd.main"] + common + ["--load_model", "True", "--evaluate", "True"],
                       cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "The win rate of qmix is" in r.stdout
