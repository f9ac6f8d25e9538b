"""tests/qtran_oracle.py on the CPU: its operations are held to torch float64 autograd of the project's own QtranQBase / QtranV
submodules, its exact cases to the 2^24 limit, its case table to the library's own plan query (marl_qtran_plan: the host functions
the launches of csrc/qtran_fused.hip themselves decide with - no GPU) and to what the table must reach, and its real cases to the
2 % cap on rows left out of the gradient comparison for sitting on a relu kink."""
import os
import types

import numpy as np
import pytest
import torch

import qtran_oracle as qo

NS = types.SimpleNamespace


@pytest.fixture(scope="module")
def ops():
    from marl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    from marl_amd import ops
    return ops


def head_got(p):
    return (p.FT, p.hot, p.dual, p.grid, p.rounds, p.slabs)


def plan_of(ops, c, what):
    return ops.qtran_plan(what, c.BT, N=c.N, A=c.A, AE=c.AE)


def module_weights(mod, head):
    """NS of qtran_oracle.WNAMES from a QtranQBase / QtranV (float64 numpy)"""
    from marl_amd.network.mixer import _linears
    enc = mod.hidden_action_encoding if head == "q" else mod.hidden_encoding
    ls = _linears(enc) + _linears(mod.q if head == "q" else mod.v)
    w = NS()
    for name, lin in zip(("enc0", "enc2", "q0", "q2", "q4"), ls):
        setattr(w, name + "_w", lin.weight.detach().cpu().double().numpy())
        setattr(w, name + "_b", lin.bias.detach().cpu().double().numpy())
    return w, ls


# ------------------------------------------------------------------------------------------------ 1. the oracle is the operation
@pytest.mark.parametrize("head,BT,N,A,S", [("q", 7, 3, 5, 9), ("q", 4, 1, 16, 3), ("q", 5, 2, 1, 1), ("v", 6, 4, 0, 11), ("v", 3, 1, 0, 2)])
def test_oracle_is_the_modules_autograd(head, BT, N, A, S):
    """per-agent encoder, THEN the agent sum, then the head (reference network/mixer.py:378-388, :411-418) in torch float64 autograd of
    the project's own submodules == the oracle's closed-form forward and backward, 1e-12 relative; actions outside [0, A) included"""
    from marl_amd.network.mixer import QtranQBase, QtranV
    args = NS(n_agents=N, n_actions=max(A, 1), state_shape=S, rnn_hidden_dim=64, qtran_hidden_dim=64)
    torch.manual_seed(BT + 10 * N + A)
    mod = (QtranQBase if head == "q" else QtranV)(args).double()
    w, ls = module_weights(mod, head)
    rng = np.random.default_rng(S)
    R = BT * N
    h = rng.standard_normal((R, 64))
    s = rng.standard_normal((BT, S))
    d = rng.standard_normal(BT)
    u = qo.draw_u(rng, R, A) if A else None
    ht = torch.from_numpy(h).requires_grad_()
    x = torch.cat([ht, torch.from_numpy(qo.onehot(u, A))], 1) if A else ht
    enc = mod.hidden_action_encoding if head == "q" else mod.hidden_encoding
    esum = enc(x).view(BT, N, -1).sum(1)
    out = (mod.q if head == "q" else mod.v)(torch.cat([torch.from_numpy(s), esum], 1)).squeeze(1)
    (out * torch.from_numpy(d)).sum().backward()
    sp = qo.state_part(w.q0_w, w.q0_b, s, S)
    f = qo.forward(w, h, u, sp, BT, N, A)
    g = qo.backward(w, f, s, d, BT, N, A)

    def close(got, want, what):
        want = want.detach().numpy() if torch.is_tensor(want) else want
        assert got.shape == want.shape, what
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), what
    close(f.out, out, "out")
    close(g.dhidden, ht.grad, "dhidden")
    for name, lin in zip(("enc0", "enc2", "q0", "q2", "q4"), ls):
        close(getattr(g, name + "_w"), lin.weight.grad, name + "_w")
        close(getattr(g, name + "_b"), lin.bias.grad, name + "_b")
    # the row-gradient statement on the same tensors gives the same gradients
    AEP = (f.AE + 15) // 16 * 16
    pad = lambda t: np.concatenate([t, np.full((BT, AEP - f.AE), 3.0)], 1)
    rg = qo.row_grads(s, pad(f.s1), pad(f.e2), f.y1, f.y2, d, g.dy1, g.dy2, pad(g.de2), f.AE)
    for k in qo.ROW_GRADS:
        close(getattr(rg, k).reshape(-1), getattr(g, k).reshape(-1), "row_grads " + k)


def test_relu_gradient_at_zero_is_zero():
    w = qo.weights(np.random.default_rng(0), "exact", 3, 4)
    for k in qo.WNAMES:
        getattr(w, k)[...] = 0
    w.q4_w[...] = 1
    f = qo.forward(w, np.zeros((2, 64), qo.F32), np.array([0, 7], np.int32), np.zeros((2, 64), qo.F32), 2, 1, 3)
    assert (f.y2p == 0).all() and (f.e1 == 0).all()
    g = qo.backward(w, f, np.zeros((2, 4)), np.ones(2), 2, 1, 3)
    assert (g.dy2 == 0).all() and (g.dhidden == 0).all() and g.q4_b[0] == 2


# ------------------------------------------------------------------------------------------------ 2. exact cases stay below 2^24
def _below(ns, what):
    for k, v in vars(ns).items():
        if isinstance(v, np.ndarray) and v.dtype == np.float64:
            assert np.abs(v).max(initial=0.0) < qo.LIMIT, "%s %s reaches %g" % (what, k, np.abs(v).max())


def _head_checks(c, kind):
    i = qo.head_inputs(c.name, kind)
    what = "%s[%s]" % (c.name, kind)
    if kind != "real":
        _below(qo.forward_mags(i.w, i.f, i.sp, c.N), what)
        _below(i.g.mag, what + " gradient")
        if c.A:
            _below(qo.forward_mags(i.w, i.f2, i.sp, c.N), what + " second set")
        for v in (i.f.out, i.g.dhidden, i.g.enc0_w, i.g.q0_w):
            assert (v == np.round(v)).all(), what
        zero = (i.f.e1 == 0).mean()
        assert zero > 0.02, "%s: pre-activations of exactly 0 are meant to be frequent (%.4f)" % (what, zero)
        assert np.abs(i.g.dhidden).max() > 0 and np.abs(i.g.enc0_w).max() > 0, what
        if kind == "probe":
            off = np.ones(c.BT, bool); off[i.rows] = False
            assert not i.h.reshape(c.BT, -1)[off].any() and not i.d_out[off].any()
        return None
    # 5. the kink cap
    cut = i.kink.mean()
    cut2 = i.kink2.mean() if c.A else 0.0
    assert cut <= qo.KINK_CAP and cut2 <= qo.KINK_CAP, "%s: %.4f / %.4f of the rows sit on a kink" % (what, cut, cut2)
    assert not i.d_out[i.kink].any() and (c.BT < 64 or np.abs(i.g.dhidden).max() > 0)
    return cut


HEAD_DATA = [(c, k) for c in qo.HEAD_CASES + qo.SEAM_CASES for k in qo.head_kinds(c)]


@pytest.mark.parametrize("c,kind", HEAD_DATA, ids=["%s-%s" % (c.name, k) for c, k in HEAD_DATA])
def test_head_case_data(c, kind):
    """exact / probe: every intermediate and every gradient sum of |terms| below 2^24, integers throughout, exact zeros frequent;
    real: at most 2 % of the rows are left out of the gradient comparison"""
    _head_checks(c, kind)


def test_row_case_data():
    for S in qo.WG_S:
        for AE in qo.WG_AE:
            for BT in qo.WG_BT:
                i = qo.wg_inputs(S, AE, BT, "exact")
                _below(i.g.mag, "wg S%d AE%d BT%d" % (S, AE, BT))
                assert max(np.abs(getattr(i.base, k)).max() + getattr(i.g.mag, k).max() for k in qo.ROW_GRADS) < qo.LIMIT
    for S in qo.SP_S:
        i = qo.sp_inputs(S, 65, "exact", 2)
        assert max(m.max() for m in i.mag) < qo.LIMIT
    # a probe case keeps a gradient row in the last row of a block, in the last slab and in the last, partial block
    BT = qo.WG_BT[-1]
    i = qo.wg_inputs(4, 64, BT, "probe")
    nz = np.flatnonzero(np.abs(i.dy1).sum(1))
    assert {31, 8191, 8160, 8192, BT - 1, BT - 7}.issubset(set(nz.tolist())) and nz.size < 40
    assert (i.g.nnz.q0_b <= nz.size).all()


# ------------------------------------------------------------------------------------------------ 3. every case gets its plan
def test_cases_get_their_plans(ops):
    for c in qo.HEAD_CASES + qo.SEAM_CASES:
        for what in ("fwd", "bwd") + (("fwd2",) if c.A else ()):
            p = plan_of(ops, c, what)
            assert p is not None and head_got(p) == qo.head_plan(c, what), (c.name, what, p)
    for S in qo.SP_S:
        for BT in qo.SP_BT:
            for n in (1, 2):
                p = ops.qtran_plan("state_parts", BT, S=S, nsets=n)
                assert (p.KCT, p.nsets, p.grid, p.rounds) == qo.sp_plan(BT, S, n), (S, BT, n, p)
            p = ops.qtran_plan("qmix_tail", BT, S=S)
            assert (p.KCT, p.nsets, p.grid, p.rounds) == qo.sp_plan(BT, S, 1), (S, BT, p)
    for S in qo.WG_S:
        for AE in qo.WG_AE:
            for BT in qo.WG_BT:
                p = ops.qtran_plan("wgrad_rows", BT, S=S, AE=AE)
                assert (p.FT, p.SMAX, p.grid, p.rounds, p.slabs) == qo.wg_plan(BT, S, AE), (S, AE, BT, p)


# ------------------------------------------------------------------------------------------------ 4. what the table reaches
def test_table_reaches_every_dispatch(ops):
    heads, rounds, grids = set(), {"head": set(), "sp": set(), "wg": set()}, {"head": set(), "sp": set(), "wg": set()}
    for c in qo.HEAD_CASES:
        for what in ("fwd", "bwd") + (("fwd2",) if c.A else ()):
            p = plan_of(ops, c, what)
            heads.add((what, p.FT, p.hot, p.dual))
            rounds["head"].add(p.rounds)
            grids["head"].add(p.grid)
    assert heads == set(qo.HEAD_INSTANCES)          # <5,true>, <4,false>, <5,true,true>; bwd_rows<5>/<4> with bwd_agents<5,true>/<4,false>
    assert {1, 2, 3} <= rounds["head"]
    assert {1, 2, 256} <= grids["head"]          # one workgroup up to 128 rows, the step to two at 129 ...
    # ... and both sides of the cap: 256 workgroups in one round at 32 768 rows, in two from 32 769 on
    assert plan_of(ops, qo.head_case("q", 3, 1, 32768), "fwd")[3:6:2] == (256, 1) and plan_of(ops, qo.head_case("q", 3, 1, 32769), "fwd")[3:6:2] == (256, 2)
    sp = set()
    for S in qo.SP_S:
        for BT in qo.SP_BT:
            for n in (1, 2):
                p = ops.qtran_plan("state_parts", BT, S=S, nsets=n)
                sp.add((p.KCT, p.nsets))
                rounds["sp"].add(p.rounds)
                grids["sp"].add(p.grid)
    assert sp == {(k, n) for k in qo.SP_BUCKETS for n in (1, 2)}
    assert rounds["sp"] == {1, 2} and {1, 2, 256, 129, 130} <= grids["sp"]
    # each bucket from both of its edges
    for lo, hi, k in ((1, 64, 4), (65, 128, 8), (129, 192, 12), (193, 224, 14), (225, 256, 16), (257, 320, 20), (321, 384, 24)):
        assert lo in qo.SP_S and hi in qo.SP_S and qo.sp_plan(1, lo, 1)[0] == qo.sp_plan(1, hi, 1)[0] == k
    wg = set()
    for S in qo.WG_S:
        for AE in qo.WG_AE:
            for BT in qo.WG_BT:
                p = ops.qtran_plan("wgrad_rows", BT, S=S, AE=AE)
                wg.add((p.FT, p.SMAX))
                rounds["wg"].add(p.rounds)
                grids["wg"].add(p.grid)
                if BT > 8192:          # ... with the slab workspace the library asks for holding all of them
                    assert p.slabs == 256
    assert wg == set(qo.WG_INSTANCES) and rounds["wg"] == {1, 2} and {1, 2, 256} <= grids["wg"]
    for a, b in ((224, 228),):
        assert qo.wg_plan(1, a, 64)[1] == 224 and qo.wg_plan(1, b, 64)[1] == 384
    # N = 1 and an odd N, every action count, every kind of action value
    assert {c.N for c in qo.HEAD_CASES} == {1, 2, 3, 4} and {c.A for c in qo.HEAD_CASES} == {0, 1, 3, 16}
    for A in (1, 3, 16):
        u = qo.draw_u(np.random.default_rng(A), 4000, A)
        want = {-1, 16, 1000} | set(range(A)) | set(range(A, 16))
        assert set(u.tolist()) == want, A
