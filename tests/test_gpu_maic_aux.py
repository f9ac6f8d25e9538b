"""The MAIC agent's MI and entropy losses on the MI355X: csrc/maic_aux.hip, the extended head backward and MAICTDLearner with the
two weights against the float64 oracle (tests/maic_aux_oracle.py); bitwise repeatability, resume, target copies, the untouched
zero-weight path and the Runner with the two new flags.

Bounds: tests/parity.close at 1e-4 * max|ref| for every tensor; the gradients that are zero analytically
(maic_aux_oracle.is_zero_gradient: w_query.bias, and under batch statistics embed_net.0.bias and inference_net.0.bias), whose
max|ref| is rounding, are bounded by 4 x the float32 oracle's own error on that tensor (figures in DESIGN section 10)."""
import numpy as np
import pytest
import torch

from oracle import learners
import parity
import maic_oracle as mo
import maic_train_oracle as mt
import maic_aux_oracle as ma

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _t(d):
    return {k: torch.tensor(np.asarray(v)) for k, v in d.items()}


def _close(case, name, got, ref64, ref32, bn_batch=False):
    """name: "<what> <parameter>" or a tensor's name; the parameter decides whether the zero-gradient bound applies"""
    kind, _, param = name.rpartition(" ")
    scale = ma.bound_scale(param, bn_batch, ref64, ref32) if kind == "grad" else None
    parity.close(case, name, got, ref64, scale=scale)


# ---------------------------------------------------------------------------------------------------- the kernel
def _run_aux(dev, g, hd, qd, epsd, bs, N, A, bn):
    from marl_amd import ops
    out = dict(mi=torch.zeros(1, device=DEV), ent=torch.zeros(1, device=DEV), dh=torch.full((bs * N, 64), 7.0, device=DEV),
               dpar=torch.full((bs * N, 2 * N * mo.L), 7.0, device=DEV))
    ops.maic_aux(ops.maic_weights(dev), ops.maic_infer_weights(dev), ops.maic_grads(g), ops.maic_infer_grads(g), hd, qd, bs, N, A,
                 ma.KMI_W, ma.KENT_W, out["mi"], out["ent"], out["dpar"], out["dh"], test_mode=False, bn_batch=bn, eps=epsd)
    return out


@pytest.mark.parametrize("case", ma.KERNEL_CASES, ids=[ma.kernel_case_id(c) for c in ma.KERNEL_CASES])
def test_aux_kernel_matches_oracle(case):
    """both losses, dh through inference_net's input, the (mean, var) plane, every gradient, inference_net.1's buffers; embed_net.1's
    buffers and every other gradient untouched; a second call gives the same bits and twice the gradients"""
    name, shape, bs, clamped, bn = case
    args, state, h, q, eps = ma.kernel_case_inputs(case)
    N, A = args.n_agents, args.n_actions
    a = (state, h, q, eps, bs, N, False, bn)
    r64, r32 = ma.kernel_reference(*a), ma.kernel_reference(*a, dtype=torch.float32)
    dev = {k: v.to(DEV).contiguous() for k, v in _t(state).items()}
    before = {k: dev[k].clone() for k in dev if mt.is_buffer(k)}
    g = {k: torch.zeros_like(v) for k, v in dev.items() if not mt.is_buffer(k)}
    hd, qd, epsd = torch.tensor(h, device=DEV), torch.tensor(q, device=DEV), torch.tensor(eps, device=DEV)
    out = _run_aux(dev, g, hd, qd, epsd, bs, N, A, bn)
    c = "maic_aux_" + ma.kernel_case_id(case)
    for k in ("mi", "ent"):
        _close(c, k, out[k].cpu().numpy()[0], r64[k], r32[k])
    _close(c, "dh", out["dh"].cpu().numpy(), r64["dh"], r32["dh"])
    _close(c, "dpar", out["dpar"].cpu().numpy(), r64["dpar"], r32["dpar"])
    for k in g:
        if k in r64["grads"]:
            _close(c, "grad " + k, g[k].cpu().numpy(), r64["grads"][k], r32["grads"][k], bn)
        else:
            assert not g[k].any(), k
    for k in (ma.IBN + "running_mean", ma.IBN + "running_var"):
        _close(c, k, dev[k].cpu().numpy(), r64["buffers"][k], r32["buffers"][k])
        if not bn:
            assert torch.equal(dev[k], before[k]), k
    assert int(dev[ma.IBN + "num_batches_tracked"]) == r64["buffers"][ma.IBN + "num_batches_tracked"] == 3 + int(bn)
    for k in mt.BUFFERS:
        assert torch.equal(dev[mo.BN + k], before[mo.BN + k]), k
    first = {k: v.clone() for k, v in g.items()}
    out2 = _run_aux(dev, g, hd, qd, epsd, bs, N, A, bn)
    for k in out:
        assert torch.equal(out[k], out2[k]), k
    for k in g:
        assert torch.equal(g[k], 2 * first[k]), k
    for k in mt.BUFFERS:
        assert torch.equal(dev[mo.BN + k], before[mo.BN + k]), k


def test_gradient_prescale_and_loss_accumulation():
    """the gradients follow den[0] * dscale exactly when that is a power of two; the losses do not, and are added into their slots"""
    case = ma.KERNEL_CASES[1]
    from marl_amd import ops
    args, state, h, q, eps = ma.kernel_case_inputs(case)
    N, A, bs = args.n_agents, args.n_actions, case[2]
    res = []
    for den, dscale, start in ((None, 1.0, 0.0), (torch.tensor([8.0], device=DEV), 0.5, 3.0)):
        dev = {k: v.to(DEV).contiguous() for k, v in _t(state).items()}
        g = {k: torch.zeros_like(v) for k, v in dev.items() if not mt.is_buffer(k)}
        o = dict(mi=torch.full((1,), start, device=DEV), ent=torch.full((1,), start, device=DEV),
                 dh=torch.zeros(bs * N, 64, device=DEV), dpar=torch.zeros(bs * N, 2 * N * mo.L, device=DEV))
        ops.maic_aux(ops.maic_weights(dev), ops.maic_infer_weights(dev), ops.maic_grads(g), ops.maic_infer_grads(g),
                     torch.tensor(h, device=DEV), torch.tensor(q, device=DEV), bs, N, A, ma.KMI_W, ma.KENT_W, o["mi"], o["ent"], o["dpar"],
                     o["dh"], test_mode=False, bn_batch=True, eps=torch.tensor(eps, device=DEV), den=den, dscale=dscale)
        res.append((o, g))
    (o1, g1), (o2, g2) = res
    assert torch.equal(o2["dh"], 4 * o1["dh"]) and torch.equal(o2["dpar"], 4 * o1["dpar"])
    for k in g1:
        assert torch.equal(g2[k], 4 * g1[k]), k
    for k in ("mi", "ent"):
        assert float(o2[k]) == pytest.approx(3.0 + float(o1[k]), rel=1e-6)


@pytest.mark.parametrize("ccase", ma.COMBINED_CASES, ids=[ma.kernel_case_id(c[0]) for c in ma.COMBINED_CASES])
def test_one_embed_backward_carries_both_terms(ccase):
    """ops.maic_head_bwd with the MI plane: dh and the embed_net / msg_net gradients of TD pairs + auxiliary losses; rows without a
    TD pair still receive the MI gradient"""
    from marl_amd import ops
    case, _ = ccase
    bs, bn = case[2], case[4]
    args, state, h, q, eps = ma.kernel_case_inputs(case, seed=ccase[1])
    N, A = args.n_agents, args.n_actions
    u_act, dq_val = ma.combined_inputs(ccase)
    r64, r32 = ma.combined_reference(ccase), ma.combined_reference(ccase, dtype=torch.float32)
    dev = {k: v.to(DEV).contiguous() for k, v in _t(state).items()}
    g = {k: torch.zeros_like(v) for k, v in dev.items() if mt.is_head_param(k)}
    plane = torch.tensor(r64["dpar"], dtype=torch.float32, device=DEV)
    dh = torch.full((bs * N, 64), 7.0, device=DEV)
    ops.maic_head_bwd(ops.maic_weights(dev), ops.maic_grads(g), torch.tensor(h, device=DEV), torch.tensor(u_act, device=DEV),
                      torch.tensor(dq_val, device=DEV), dh, bs, N, A, test_mode=False, bn_batch=bn, eps=torch.tensor(eps, device=DEV),
                      dpar_extra=plane)
    c = "maic_head_bwd_ex_" + ma.kernel_case_id(case)
    _close(c, "dh", dh.cpu().numpy(), r64["dh"], r32["dh"])
    for k in r64["grads"]:
        _close(c, "grad " + k, g[k].cpu().numpy(), r64["grads"][k], r32["grads"][k], bn)
    assert ((u_act < 0) | (dq_val == 0)).sum() >= 10


# ---------------------------------------------------------------------------------------------------- the learner
def build_product(case, weights=(ma.MI_W, ma.ENT_W)):
    from marl_amd.controller.share_params import MAICMAC
    from marl_amd.algorithm.maic_td_learner import MAICTDLearner
    args, agent, mixer = ma.update_case_states(case)
    args.cuda = True
    args.mi_loss_weight, args.entropy_loss_weight = weights
    mac = MAICMAC(args)
    mac.agent.load_state_dict(_t(agent), strict=True)
    mac.agent.train(case[2])
    learner = MAICTDLearner(mac, args)
    if mixer:
        learner.mixer.load_state_dict(_t(mixer))
        learner.target_mixer.load_state_dict(_t(mixer))
    return args, mac, learner


def named_product_params(learner):
    out = [("agent." + k, p) for k, p in learner.eval_net.agent.named_parameters()]
    if learner.mixer is not None:
        out += [("mixer." + k, p) for k, p in learner.mixer.named_parameters()]
    return out


_ORACLE = {}


def oracle_updates(case):
    if case[0] not in _ORACLE:
        _ORACLE[case[0]] = ma.reference_updates(case)
    return _ORACLE[case[0]]


@pytest.mark.parametrize("case", ma.UPDATE_CASES, ids=[c[0] for c in ma.UPDATE_CASES])
def test_two_updates_match_oracle(case):
    """two MAICTDLearner.train calls: the loss, the two statistics sums, every gradient, every parameter after each step, both
    networks' buffers.  The eval-mode case takes one auxiliary call over B*T environments: the same loss definition"""
    name, alg, bn_train = case
    o64, o32 = oracle_updates(case)
    args, mac, learner = build_product(case)
    batch, eps = ma.update_case_data(case)
    inf0 = {k: v.detach().clone() for k, v in learner.eval_net.agent.inference_net.named_parameters()}
    keep = None
    for ts, (s64, s32) in enumerate(zip(o64, o32)):
        loss = learner.train(learners.clone_batch(batch), ts, eps=eps)
        c = "maic_aux_update:%s[step %d]" % (name, ts)
        assert learner.max_episode_len == s64["T"]
        _close(c, "loss", loss, s64["loss"], s32["loss"])
        stats = learner.last_stats.cpu().numpy()
        den = float(stats[1])
        _close(c, "mi_sum", stats[2], s64["mi_sum"], s32["mi_sum"])
        _close(c, "ent_sum", stats[3], s64["ent_sum"], s32["ent_sum"])
        named = named_product_params(learner)
        for n, p in named:
            _close(c, "grad " + n, p.grad.detach().cpu().numpy() / den, s64["grads"][n], s32["grads"][n], bn_train)
        step = {n: mt.step_is_decided(n, s64["grads"]) for n in s64["grads"]}
        keep = step if keep is None else {n: keep[n] & step[n] for n in keep}
        for n, p in named:
            _close(c, "param " + n, p.detach().cpu().numpy()[keep[n]], s64["params"][n][keep[n]], s32["params"][n][keep[n]])
        for tag, net in (("eval", learner.eval_net), ("target", learner.target_net)):
            bufs = dict(net.agent.named_buffers())
            for pre in (mo.BN, ma.IBN):
                for k in mt.BUFFERS[:2]:
                    ref64, ref32 = s64["bn_" + tag][pre + k], s32["bn_" + tag][pre + k]
                    parity.close(c, "%s %s" % (tag, pre + k), bufs[pre + k].cpu().numpy(), ref64,
                                 scale=ma.buffer_scale(pre + k, bn_train, ts, ref64, ref32))
                assert int(bufs[pre + "num_batches_tracked"]) == int(s64["bn_" + tag][pre + "num_batches_tracked"]), pre
    for k, p in learner.eval_net.agent.inference_net.named_parameters():
        assert not torch.equal(p.detach(), inf0[k]), k


def _fresh_update(case, weights=(ma.MI_W, ma.ENT_W), steps=(0,)):
    args, mac, learner = build_product(case, weights)
    batch, eps = ma.update_case_data(case)
    losses = [learner.train(learners.clone_batch(batch), ts, eps=eps) for ts in steps]
    return learner, losses


@pytest.mark.parametrize("case", [ma.UPDATE_CASES[0], ma.UPDATE_CASES[2]], ids=["batch", "eval"])
def test_two_learners_give_the_same_bits(case):
    (a, la), (b, lb) = _fresh_update(case), _fresh_update(case)
    assert la == lb
    assert torch.equal(a._flat.flat, b._flat.flat) and torch.equal(a._flat.gradx, b._flat.gradx)
    for (k, x), (_, y) in zip(a.eval_net.agent.named_buffers(), b.eval_net.agent.named_buffers()):
        assert torch.equal(x, y), k


def test_target_sync_and_resume_carry_the_inference_buffers(tmp_path):
    case = ma.UPDATE_CASES[0]
    args, mac, learner = build_product(case)
    learner.args.target_update_cycle = 2
    batch, eps = ma.update_case_data(case)
    for ts in (0, 1):
        learner.train(learners.clone_batch(batch), ts, eps=eps)
    e, t = dict(learner.eval_net.agent.named_buffers()), dict(learner.target_net.agent.named_buffers())
    assert not torch.equal(e[ma.IBN + "running_mean"], t[ma.IBN + "running_mean"])
    assert int(t[ma.IBN + "num_batches_tracked"]) == 3 and int(e[ma.IBN + "num_batches_tracked"]) == 3 + 2 * ma.UT
    learner.train(learners.clone_batch(batch), 2, eps=eps)              # train_step = target_update_cycle
    e = dict(learner.eval_net.agent.named_buffers())
    for k, b in learner.target_net.agent.named_buffers():
        assert torch.equal(b, e[k]), k
    assert int(e[ma.IBN + "num_batches_tracked"]) == 3 + 3 * ma.UT
    path = str(tmp_path / "resume.pt")
    learner.save_resume(path)
    args2, mac2, learner2 = build_product(case)
    learner2.args.target_update_cycle = 2
    learner2.load_resume(path)
    for (k, x), (_, y) in zip(learner.eval_net.agent.named_buffers(), learner2.eval_net.agent.named_buffers()):
        assert torch.equal(x, y), k
    b2, eps2 = ma.update_case_data(case, batch_seed=101)
    la = learner.train(learners.clone_batch(b2), 3, eps=eps2)
    lb = learner2.train(learners.clone_batch(b2), 3, eps=eps2)
    assert la == lb
    assert torch.equal(learner._flat.flat, learner2._flat.flat)
    for net in ("eval_net", "target_net"):
        for (k, x), (_, y) in zip(getattr(learner, net).agent.named_buffers(), getattr(learner2, net).agent.named_buffers()):
            assert torch.equal(x, y), (net, k)


def test_zero_weights_never_reach_the_auxiliary_kernel(monkeypatch):
    """default weights: ops.maic_aux is not called, inference_net stays where it was, and the update is today's, bit for bit"""
    from marl_amd import ops
    case = ma.UPDATE_CASES[0]
    ref, lref = _fresh_update(case, weights=(0.0, 0.0))

    def refuse(*a, **k):
        raise AssertionError("maic_aux called with both weights zero")
    monkeypatch.setattr(ops, "maic_aux", refuse)
    got, lgot = _fresh_update(case, weights=(0.0, 0.0))
    assert lgot == lref and np.isfinite(lgot[0])
    assert torch.equal(got._flat.flat, ref._flat.flat) and torch.equal(got._flat.gradx, ref._flat.gradx)
    bufs = dict(got.eval_net.agent.named_buffers())
    assert int(bufs[ma.IBN + "num_batches_tracked"]) == 3
    assert got.n_stats == 2 and float(got.last_stats[2]) == 0.0 and float(got.last_stats[3]) == 0.0
    with pytest.raises(AssertionError):
        _fresh_update(case)


def test_runner_trains_with_the_two_flags(tmp_path):
    from marl_amd.main import build
    from marl_amd.runner import Runner
    from marl_amd.utils.logging import Logger
    from marl_amd.algorithm.maic_td_learner import MAICTDLearner
    args, env = build(["--alg", "qmix", "--map", "2s3z", "--n_envs", "8", "--MAIC", "True", "--MAIC_train", "True",
                       "--mi_loss_weight", "0.001", "--entropy_loss_weight", "0.01", "--evaluate_epoch", "1", "--n_steps", "1500",
                       "--evaluate_cycle", "100000", "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "m")])
    args.train_steps = 3
    runner = Runner(env, Logger(), args)
    assert isinstance(runner.learner, MAICTDLearner) and runner.learner.aux
    inf0 = {k: v.detach().clone() for k, v in runner.learner.eval_net.agent.inference_net.named_parameters()}
    loss = runner.run(0)
    assert runner.train_steps >= 3 and np.isfinite(float(loss))
    stats = runner.learner.last_stats.cpu().numpy()
    assert stats[2] > 0 and stats[3] > 0
    for k, p in runner.learner.eval_net.agent.inference_net.named_parameters():
        assert not torch.equal(p.detach(), inf0[k]), k
