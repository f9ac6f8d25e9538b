"""The RTW and world-model head kernels (csrc/rtw_head.hip, csrc/world_head.hip) on the MI355X against their float64 oracles
at every edge of their support: the cases of tests/head_cases.py (partly filled tiles, one and two column tiles, the (T+1)-slot
storage with everything unread at NaN, tiles straddling episodes, the 256-partial seam of the loss reduction, every addressing
mode and every optional argument).  Bound: 1e-4 of max|ref| through parity.close.  Every output buffer carries a 16-row
sentinel tail that must stay untouched."""
import numpy as np
import pytest
import torch

import head_cases as hc
import parity

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PAD, SENT, SENT_A = 16, 12345.0, -7
ROUND = 2.0 ** -24          # rounding of a stored float32 sum, relative


def dev(x):
    return torch.tensor(np.asarray(x), device=DEV)


def padded(rows, fill=SENT):
    """a device buffer PAD rows longer than `rows` (numpy, 2-D), the tail at the sentinel"""
    rows = np.asarray(rows)
    out = torch.full((rows.shape[0] + PAD,) + rows.shape[1:], fill, dtype=torch.tensor(rows[:0]).dtype, device=DEV)
    out[:rows.shape[0]] = dev(rows)
    return out


def blank(n, width, fill=SENT, dtype=torch.float32):
    return torch.full((n + PAD, width), fill, dtype=dtype, device=DEV)


def body_and_tail(buf, n, fill=SENT):
    """the first n rows as numpy after checking that the tail still holds the sentinel and no row holds a NaN"""
    a = buf.cpu().numpy()
    assert (a[n:] == fill).all(), "rows past the batch were written"
    assert not np.isnan(a[:n]).any()
    return a[:n]


def added_term(case, name, q_out, q0, ref, tol=1e-4):
    """(q_out - q0) against the added term alone: 1e-4 max|ref| plus the rounding of the stored sum, 2^-24 max|q_out|"""
    q_out, q0 = np.asarray(q_out, np.float64), np.asarray(q0, np.float64)
    scale = float(np.abs(ref).max()) + ROUND * float(np.abs(q_out).max()) / tol
    parity.close(case, name, q_out - q0, ref, tol=tol, scale=scale)


# ------------------------------------------------------------------------------------------------------------ RTW head
def rtw_weights(N, O, A, seed):
    from marl_amd import ops
    return ops.rtw_weights({k: dev(v) for k, v in hc.rtw_params(N, O, A, seed).items() if not k.startswith(("fc", "rnn"))})


def run_act(w, c, not_self, optional=True):
    from marl_amd import ops
    n = c.G * c.N
    q = padded(c.q0)
    a_out, ohat = (blank(n, c.N, SENT_A, torch.int32), blank(n, c.O)) if optional else (None, None)
    ops.rtw_head_act(w, dev(c.h), dev(c.obs), hc.RTW_SLOTS * c.N, hc.RTW_T0, dev(c.avail), hc.RTW_SLOTS * c.N, hc.RTW_T0, q,
                     c.G, c.N, c.O, c.A, not_self, a_out=a_out, ohat_out=ohat)
    return q, a_out, ohat


def run_given(w, c, not_self):
    from marl_amd import ops
    q = padded(c.q0.reshape(-1, c.A))
    obs = dev(c.obs)
    ops.rtw_head_given(w, dev(c.hs), obs, (c.T + 1) * c.N, 0, obs, (c.T + 1) * c.N, 1, dev(c.plane), (c.T + 2) * c.N, 1, q,
                       c.B, c.T, c.N, c.O, c.A, not_self)
    return q


@pytest.mark.parametrize("not_self", [True, False], ids=["ns", "self"])
@pytest.mark.parametrize("case", hc.RTW_CASES, ids=[hc.shape_id(*c[:3]) for c in hc.RTW_CASES])
def test_rtw_act_head_at_every_row_count(case, not_self):
    """G in {1, EPT - 1, EPT, EPT + 1, 3 EPT + 1}: a_out exactly (every margin is >= 1e-4: no row is left out), o_hat, the
    added term against q_r; sentinel tails; q the same bits without the optional outputs and on a second call"""
    N, O, A, seed = case
    w = rtw_weights(N, O, A, seed)
    for G in hc.rtw_row_counts(N):
        c, o = hc.rtw_act_oracle(N, O, A, G, seed, not_self)
        name = "rtw_edge:%s_%s" % (hc.shape_id(N, O, A), "ns" if not_self else "self")
        n = G * N
        q, a_out, ohat = run_act(w, c, not_self)
        np.testing.assert_array_equal(body_and_tail(a_out, n, SENT_A), o.a, err_msg="G=%d" % G)
        got_o = body_and_tail(ohat, n)
        assert not (got_o == SENT).any()
        parity.close(name, "act/o_hat G=%d" % G, got_o, o.ohat)
        got_q = body_and_tail(q, n)
        assert (got_q != c.q0).any(1).all(), "a row of q was not written"
        added_term(name, "act/q - q0 G=%d" % G, got_q, c.q0, o.qr)
        q1, _, _ = run_act(w, c, not_self, optional=False)
        assert torch.equal(q1, q), "q depends on the optional outputs"
        q2, a2, o2 = run_act(w, c, not_self)
        assert torch.equal(q2, q) and torch.equal(a2, a_out) and torch.equal(o2, ohat)


@pytest.mark.parametrize("not_self", [True, False], ids=["ns", "self"])
@pytest.mark.parametrize("case", hc.RTW_CASES, ids=[hc.shape_id(*c[:3]) for c in hc.RTW_CASES])
def test_rtw_given_head_across_episode_boundaries(case, not_self):
    """B >= 3 episodes of T steps, T no multiple of EPT: tiles straddle episodes; o and o_next from one (T+1)-slot storage,
    u from slot 1 of a (T+2)-slot plane with padded (-1) entries"""
    N, O, A, seed = case
    w = rtw_weights(N, O, A, seed)
    for B, T in hc.rtw_given_bt(N):
        c, qr = hc.rtw_given_oracle(N, O, A, B, T, seed, not_self)
        name = "rtw_edge:%s_%s" % (hc.shape_id(N, O, A), "ns" if not_self else "self")
        n = B * T * N
        q = run_given(w, c, not_self)
        got = body_and_tail(q, n)
        q0 = c.q0.reshape(n, A)
        assert (got != q0).any(1).all(), "a row of q was not written"
        added_term(name, "given/q - q0 B=%d T=%d" % (B, T), got, q0, qr.reshape(n, A))
        assert torch.equal(run_given(w, c, not_self), q)


def test_rtw_unsupported_shapes_are_refused_before_any_launch():
    from marl_amd import ops, _lib
    N, O, A, seed = hc.RTW_CASES[4]
    w = rtw_weights(N, O, A, seed)
    big = lambda *s: torch.full(s, SENT, device=DEV)
    for n, o, a in ((17, O, A), (N, O, 33), (N, 257, A), (N, O, 0), (N, 0, A)):
        assert not ops.rtw_supported(n, o, a)
        q, ohat = big(64, 64), big(64, 512)
        a_out = torch.full((64, 32), SENT_A, dtype=torch.int32, device=DEV)
        with pytest.raises(_lib.MarlHipError):
            ops.rtw_head_act(w, big(64, 64), big(64, 4, 512), 4 * n, 0, big(64, 4, 64), 4 * n, 0, q, 2, n, o, a, True,
                             a_out=a_out, ohat_out=ohat)
        with pytest.raises(_lib.MarlHipError):
            ops.rtw_head_given(w, big(64, 64), big(64, 4, 512), 4 * n, 0, big(64, 4, 512), 4 * n, 1,
                               torch.zeros(4096, dtype=torch.int32, device=DEV), 3 * n, 0, q, 1, 2, n, o, a, True)
        torch.cuda.synchronize()
        assert (q == SENT).all() and (ohat == SENT).all() and (a_out == SENT_A).all()


# ---------------------------------------------------------------------------------------------------------- world head
def world_weights(c):
    from marl_amd import ops
    return ops.world_weights({k: dev(v) for k, v in c.p.items()})


def world_fwd(w, c, q=True, outputs=True, train=None):
    """one forward: (q, r_out, ohat_out, tau_out, loss); train = (storage, mode) adds the loss into slot 0 of a (2,) buffer at 1.5"""
    from marl_amd import ops
    qb = padded(c.q0.reshape(c.R, c.A)) if q else None
    r, oh, tau = (blank(c.R, c.A), blank(c.R, c.O), blank(c.R, 2)) if outputs else (None, None, None)
    kw, loss = {}, None
    if train is not None:
        loss = torch.full((2,), 1.5, device=DEV)
        kw = dict(loss=loss[0:1], **addressing(c, *train))
    ops.world_head_fwd(w, dev(c.h), qb, c.B, c.T, c.N, c.O, c.A, r_out=r, ohat_out=oh, tau_out=tau, **kw)
    return qb, r, oh, tau, loss


def addressing(c, st, mode):
    kw = dict(obs=dev(st), obs_bs=(c.T + 1) * c.N, obs_t0=1)
    if mode in ("map", "len"):
        kw["ep_len"] = dev(c.ep_len)
    if mode == "map":
        kw["ep_map"] = dev(c.emap)
    return kw


def world_bwd(w, c, st, mode, g, dq=True, den=True):
    """one backward accumulating into the gradient dict g; returns dhs with its sentinel tail"""
    from marl_amd import ops
    dhs = blank(c.R, 64)
    kw = addressing(c, st, mode)
    ops.world_head_bwd(w, ops.world_grads(g), dev(c.h), dev(c.dq_idx) if dq else None, dev(c.dq_val) if dq else None,
                       kw["obs"], kw["obs_bs"], kw["obs_t0"], torch.tensor([c.den], device=DEV) if den else None, c.dscale, dhs,
                       c.B, c.T, c.N, c.O, c.A, ep_len=kw.get("ep_len"), ep_map=kw.get("ep_map"))
    return dhs


def fresh_grads(c):
    g = {k: dev(v) for k, v in c.base.items()}
    g.update({"world.terminate_out.weight": torch.zeros(2, 64, device=DEV), "world.terminate_out.bias": torch.zeros(2, device=DEV)})
    return g


def check_grads(name, tag, c, g, ref, times=1.0):
    for k in hc.WORLD_GRADS:
        parity.close(name, "%s grad %s" % (tag, k), g[k].cpu().numpy().astype(np.float64) - c.base[k], times * ref.grads[k])
    assert float(g["world.terminate_out.weight"].abs().max()) == 0.0 and float(g["world.terminate_out.bias"].abs().max()) == 0.0


@pytest.mark.parametrize("case", hc.WORLD_CASES, ids=[hc.world_id(c) for c in hc.WORLD_CASES])
def test_world_head_at_every_row_count_and_addressing_mode(case):
    """forward (r, o_hat, tau, the added term; the same bits with q = None), then per addressing mode the train-mode loss added
    into a non-zero slot and the backward from a random gradient base: fresh-buffer repeat bitwise, second call accumulates"""
    c = hc.world_case(case)
    name = "world_edge:" + hc.world_id(case)
    w = world_weights(c)
    r_ref, o_ref, t_ref = (x.reshape(c.R, -1) for x in hc.world_forward_oracle(case))
    q0 = c.q0.reshape(c.R, c.A)
    q, r, oh, tau, _ = world_fwd(w, c)
    for nm, buf, ref in (("r", r, r_ref), ("o_hat", oh, o_ref), ("tau", tau, t_ref)):
        got = body_and_tail(buf, c.R)
        assert not (got == SENT).any(), nm
        parity.close(name, nm, got, ref)
    added_term(name, "q - q0", body_and_tail(q, c.R), q0, r_ref)
    _, r1, oh1, tau1, _ = world_fwd(w, c, q=False)
    assert torch.equal(r1, r) and torch.equal(oh1, oh) and torch.equal(tau1, tau), "the outputs depend on q"
    for mode in hc.WORLD_MODES:
        st, _ = hc.world_storage(c, mode)
        ref = hc.world_backward_oracle(case, mode)
        q1, _, _, _, loss = world_fwd(w, c, outputs=False, train=(st, mode))
        added_term(name, mode + "/train q - q0", body_and_tail(q1, c.R), q0, r_ref)
        assert float(loss[1].item()) == 1.5, "the neighbouring loss slot was written"
        parity.close(name, mode + "/loss", float(loss[0].item()) - 1.5, ref.loss)
        g = fresh_grads(c)
        dhs = world_bwd(w, c, st, mode, g)
        parity.close(name, mode + "/dhs", body_and_tail(dhs, c.R), ref.dhs.reshape(c.R, 64))
        check_grads(name, mode, c, g, ref)
        g2 = fresh_grads(c)
        dhs2 = world_bwd(w, c, st, mode, g2)
        assert torch.equal(dhs2, dhs) and all(torch.equal(g[k], g2[k]) for k in g), "a second backward gave other bits"
        dhs3 = world_bwd(w, c, st, mode, g)
        assert torch.equal(dhs3, dhs), "dhs is written, not accumulated"
        check_grads(name, mode + " twice", c, g, ref, times=2.0)


SMALL_WORLD = hc.WORLD_OPTIONAL_CASES


@pytest.mark.parametrize("case", SMALL_WORLD, ids=[hc.world_id(c) for c in SMALL_WORLD])
def test_world_backward_without_dq_and_without_den(case):
    """dq_idx = NULL is the oracle with dr = 0 (r_out gets no gradient at all); den = NULL is den = 1"""
    c = hc.world_case(case)
    name = "world_edge:" + hc.world_id(case)
    w = world_weights(c)
    st, _ = hc.world_storage(c, "map")
    for tag, kw in (("no dq", dict(dq=False)), ("no den", dict(den=False))):
        ref = hc.world_backward_oracle(case, "map", **kw)
        g = fresh_grads(c)
        dhs = world_bwd(w, c, st, "map", g, **kw)
        parity.close(name, tag + "/dhs", body_and_tail(dhs, c.R), ref.dhs.reshape(c.R, 64))
        check_grads(name, tag, c, g, ref)
        if tag == "no dq":
            assert np.abs(ref.grads["world.r_out.weight"]).max() == 0.0
            assert torch.equal(g["world.r_out.weight"], dev(c.base["world.r_out.weight"]))


def test_world_unsupported_shapes_are_refused_before_any_launch():
    from marl_amd import ops, _lib
    case = SMALL_WORLD[-1]
    c = hc.world_case(case)
    w = world_weights(c)
    big = lambda *s: torch.full(s, SENT, device=DEV)
    for n, o, a in ((17, c.O, c.A), (c.N, c.O, 33), (c.N, 257, c.A), (c.N, c.O, 0), (c.N, 0, c.A)):
        assert not ops.world_supported(n, o, a)
        q, r, oh, tau, dhs = big(64, 64), big(64, 64), big(64, 512), big(64, 2), big(64, 64)
        loss = big(2)
        with pytest.raises(_lib.MarlHipError):
            ops.world_head_fwd(w, big(64, 64), q, 1, 2, n, o, a, r_out=r, ohat_out=oh, tau_out=tau, obs=big(8, 3, 64, 512),
                               obs_bs=3 * n, obs_t0=1, loss=loss[0:1])
        g = fresh_grads(c)
        with pytest.raises(_lib.MarlHipError):
            ops.world_head_bwd(w, ops.world_grads(g), big(64, 64), torch.zeros(64, dtype=torch.int32, device=DEV), big(64),
                               big(8, 3, 64, 512), 3 * n, 1, big(1), 1.0, dhs, 1, 2, n, o, a)
        torch.cuda.synchronize()
        assert all((t == SENT).all() for t in (q, r, oh, tau, dhs, loss))
        assert all(torch.equal(g[k], dev(c.base[k])) for k in c.base)
