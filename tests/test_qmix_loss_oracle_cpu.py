"""The float64 statement of the loss-folded QMIX backward (tests/qmix_loss_oracle.py) checked on the CPU, before the kernels are
held to it (tests/test_gpu_qmix_loss.py): against the project's fp32 learner oracle, against finite differences, on the padded /
terminated row rules, and the kink count of every seeded kernel case."""
import numpy as np
import pytest
import torch

from oracle import learners, seeded

import qmix_loss_oracle as qo

MIXER_KEYS = {"w1": "hyper_w1", "b1": "hyper_b1", "w2": "hyper_w2", "h": "hyper_b2.0"}


def _named(mixer):
    """oracle/seeded.py state_dict names -> the ten names of ops.qmix_weights"""
    P = {}
    for k, name in MIXER_KEYS.items():
        P[k], P[k + "_b"] = mixer[name + ".weight"], mixer[name + ".bias"]
    P["b2_w"], P["b2_b"] = mixer["hyper_b2.2.weight"], mixer["hyper_b2.2.bias"]
    return P


def _learner_case(shape, **over):
    """one seeded learner batch through oracle/learners.q_forward (fp32): the mixer's inputs as the learner forms them, and the
    un-normalised loss numerator's gradients by autograd"""
    T = 6
    args = seeded.make_args(shape, "qmix", episode_limit=T, **over)
    agent = seeded.seeded_state(seeded.agent_param_shapes(args), seed=10)
    mixer = seeded.seeded_state(seeded.mixer_param_shapes(args), seed=12, scale=3.0)
    st = learners.LearnerState(args, agent, mixer)
    st.target_mixer = {k: v * 0.9 for k, v in st.target_mixer.items()}                # a target that differs from the eval mixer
    batch = seeded.make_batch(args, 5, seed=11, lengths=[T, 3, -1, 1, 4])
    _, inter = learners.q_forward(st, batch)
    bt = learners.to_tensors(batch, inter["T"])
    names = list(st.mixer)
    gs = torch.autograd.grad(inter["num"], [inter["q_evals"]] + [st.mixer[k] for k in names])
    rows = lambda t: t.detach().reshape(-1)
    N = args.n_agents
    return dict(args=args, P=_named({k: v.detach() for k, v in st.mixer.items()}),
                s=bt["s"].reshape(-1, args.state_shape), q=torch.gather(inter["q_evals"], 3, bt["u"]).detach().reshape(-1, N),
                q_tot_tgt=rows(inter["q_tot_target"]), r=rows(bt["r"]), term=rows(bt["terminated"]), padded=rows(bt["padded"]),
                q_tot=rows(inter["q_tot"]), num=float(inter["num"].detach()), den=float(inter["den"]),
                dq=torch.gather(gs[0], 3, bt["u"]).reshape(-1, N), grads=_named(dict(zip(names, gs[1:]))))


def _near(got, want, rel, msg):
    """|got - want| <= rel * max|want| elementwise"""
    want = want.double()
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=rel * float(want.abs().max()), err_msg=msg)


# fp32 rounding of the fp32 oracle: sums of up to 322 products per hypernet output and 30 rows per gradient entry, every
# operation rounded to 2^-24 relative - 1e-5 of a tensor's scale is 170 roundings, all in one direction
FP32 = 1e-5


@pytest.mark.parametrize("shape", ["2s3z", "MMM2"])
def test_oracle_equals_the_learner_oracle(shape):
    """(a) oracle.nets.qmix + the TD rule of oracle/learners.py (fp32) on a seeded batch with ragged episodes"""
    c = _learner_case(shape)
    assert c["padded"].sum() > 0 and (c["term"] * (1 - c["padded"])).sum() > 0
    o = qo.loss_backward(c["P"], c["s"], c["q"], c["q_tot_tgt"], c["r"], c["term"], c["padded"], c["args"].gamma)
    _near(o.q_tot, c["q_tot"], FP32, "q_tot")
    assert abs(float(o.loss2[0]) - c["num"]) <= FP32 * c["num"] and float(o.loss2[1]) == c["den"]
    _near(o.dq, c["dq"], FP32, "dq")
    for k in qo.NAMES:
        _near(o.grads[k], c["grads"][k], FP32, k)


def test_bf16_mode_equals_the_learner_oracle_with_a_bf16_mixer():
    """the bf16 option against oracle.nets.qmix with mixer_dtype = "bf16" (same operand rounding).  That oracle also rounds
    d(out) to bf16 in the weight gradient (2^-9 relative per term), this one does not: weight matrices within 1e-2 of scale"""
    c = _learner_case("MMM2", mixer_dtype="bf16")
    o = qo.loss_backward(c["P"], c["s"], c["q"], c["q_tot_tgt"], c["r"], c["term"], c["padded"], c["args"].gamma, bf16=True)
    plain = qo.loss_backward(c["P"], c["s"], c["q"], c["q_tot_tgt"], c["r"], c["term"], c["padded"], c["args"].gamma)
    assert float((o.q_tot - plain.q_tot).abs().max()) > 1e-4 * float(plain.q_tot.abs().max())      # the rounding is visible
    _near(o.q_tot, c["q_tot"], FP32, "q_tot")
    _near(o.dq, c["dq"], FP32, "dq")
    for k in qo.NAMES:
        _near(o.grads[k], c["grads"][k], 1e-2 if k in qo.SEGMENTS else FP32, k)
    # flags = 1: same values, and the weight gradient on the unrounded states - equal where the states are bf16 numbers already
    f = qo.loss_backward(c["P"], c["s"], c["q"], c["q_tot_tgt"], c["r"], c["term"], c["padded"], c["args"].gamma, bf16=True,
                         wgrad_fp32=True)
    assert torch.equal(f.q_tot, o.q_tot) and torch.equal(f.dq, o.dq) and torch.equal(f.loss2, o.loss2)
    for k in qo.NAMES:
        assert torch.equal(f.grads[k], o.grads[k]) == (k not in qo.SEGMENTS), k
    sb = c["s"].bfloat16().float()
    f2 = qo.loss_backward(c["P"], sb, c["q"], c["q_tot_tgt"], c["r"], c["term"], c["padded"], c["args"].gamma, bf16=True, wgrad_fp32=True)
    o2 = qo.loss_backward(c["P"], sb, c["q"], c["q_tot_tgt"], c["r"], c["term"], c["padded"], c["args"].gamma, bf16=True)
    for k in qo.NAMES:
        _near(f2.grads[k], o2.grads[k], 1e-12, k)


def test_gradients_agree_with_central_differences():
    """(b) float64 central differences of sum td^2 for every entry of q and five entries of each of the ten tensors, at a small
    shape whose hypernet outputs stay 1e-3 away from the kinks of |.| and relu"""
    R, N, S = 9, 3, 6
    c = qo.make_case(R, N, S, seed=12, episode=3)
    assert c.padded.sum() > 0 and (c.term * (1 - c.padded)).sum() > 0
    P = {k: v.double() * (3.0 if k in qo.SEGMENTS else 1.0) for k, v in c.P.items()}
    q = c.q.double()
    run = lambda P_, q_: qo.loss_backward(P_, c.s, q_, c.q_tot_tgt, c.r, c.term, c.padded, 0.99)
    o = run(P, q)
    assert min(float(v.abs().min()) for v in o.hyper.values()) > 1e-3
    h = 1e-6
    g = torch.Generator().manual_seed(1)

    def fd(name, idx):
        out = []
        for sign in (1.0, -1.0):
            P_ = {k: v.clone() for k, v in P.items()}
            q_ = q.clone()
            (q_ if name == "q" else P_[name]).view(-1)[idx] += sign * h
            out.append(float(run(P_, q_).loss2[0]))
        return (out[0] - out[1]) / (2 * h)

    # central differences: truncation h^2 f''' / 6 ~ 1e-12 f''', rounding 2^-53 f / h ~ 1e-9 at f ~ 10
    for idx in range(R * N):
        want = float(o.dq.view(-1)[idx])
        assert abs(fd("q", idx) - want) <= 1e-6 * max(1.0, abs(want)), ("q", idx)
    for k in qo.NAMES:
        n = P[k].numel()
        for idx in torch.randperm(n, generator=g)[:5].tolist():
            want = float(o.grads[k].view(-1)[idx])
            assert abs(fd(k, idx) - want) <= 1e-6 * max(1.0, abs(want)), (k, idx)


def test_padded_and_terminated_rows():
    """(c) padded rows get exactly zero dq and add nothing; terminated rows have a target without q_tot_tgt"""
    c = qo.make_case(60, 3, 8, seed=7)
    pad, real_term = c.padded.bool(), (c.term * (1 - c.padded)).bool()
    assert pad.any() and real_term.any() and (~c.term.bool()).any()
    run = lambda **kw: qo.loss_backward(c.P, c.s, c.q, kw.get("tgt", c.q_tot_tgt), kw.get("r", c.r), c.term, c.padded, 0.99)
    o = run()
    assert (o.dq[pad] == 0).all() and (o.dq[~pad].abs().sum(1) > 0).all()
    assert float(o.loss2[1]) == float((~pad).sum())
    assert torch.equal(o.td[real_term], (c.r.double() - o.q_tot)[real_term])
    big = torch.where(pad, torch.full_like(c.r, 1e6), c.r)
    o2 = run(r=big, tgt=torch.where(pad, torch.full_like(c.r, -1e6), c.q_tot_tgt))
    o3 = run(tgt=torch.where(c.term.bool(), c.q_tot_tgt + 5.0, c.q_tot_tgt))
    for other in (o2, o3):
        assert torch.equal(other.loss2, o.loss2) and torch.equal(other.dq, o.dq)
        for k in qo.NAMES:
            assert torch.equal(other.grads[k], o.grads[k]), k
    o4 = run(tgt=c.q_tot_tgt + 5.0)                                                    # ... and rows that go on do use it
    assert not torch.equal(o4.dq, o.dq)


def _all_cases():
    out = [("fused", c[:3], c[3], False) for c in qo.FUSED_CASES]
    for R, N, S, seed, seed_bf in qo.WIDE_CASES:
        out.append(("wide", (R, N, S), seed, False))
        if seed_bf is not None:
            out.append(("wide", (R, N, S), seed_bf, True))
    for fam, (R, N, S, seed) in qo.REMAP_CASES.items():
        out += [(fam, (R, N, S), seed, False)] + ([(fam, (R, N, S), seed, True)] if fam == "wide" else [])
    return out


@pytest.mark.parametrize("family,shape,seed,bf16", _all_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_seeded_kernel_cases_stay_within_the_kink_cap(family, shape, seed, bf16):
    """the seed of every kernel case is chosen so that the float64 hypernet outputs alone have at most 2 columns within 2e-6 of
    a kink (4 for the 32775-row case with bf16-rounded operands: under 1 % of its 416 columns), and every case has the rows
    the loss rules are about: padded ones and terminated real ones (but for the single-row case)"""
    c = qo.make_case(*shape, seed)
    cap = qo.KINK_CAP_32775_BF16 if (bf16 and shape[0] == 32775) else qo.KINK_CAP
    assert qo.count_kinks(c, bf16=bf16) <= cap
    if shape[0] > 1:
        assert c.padded.sum() > 0 and (c.term * (1 - c.padded)).sum() > 0 and (1 - c.term).sum() > 0
    assert ((c.padded == 0) | (c.term == 1)).all()
