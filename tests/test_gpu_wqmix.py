"""csrc/wqmix.hip on the MI355X.  Needs a real MI355X: ``pytest -m gpu``.

marl_wqmix_select against the composition it replaces - marl_q_gather, marl_q_masked_max and marl_q_double_select - bit for bit, at
the shapes of wqmix_oracle.SELECT_SHAPES (staged and global-scan forms, tile and workgroup edges; padded rows hold NaN and u = -1,
one live row has nothing available, one a u outside [0, A)).  marl_wqmix_loss in both modes against the float64 contract at
parity.close's 1e-4 * max|ref|, w and the two counts exactly, at alpha = 1 bit for bit against marl_td_loss, twice to the same bits,
NaN on padded rows.  Every refused argument set returns the error and leaves the outputs' sentinel."""
import ctypes as C

import numpy as np
import pytest
import torch

import wqmix_oracle as wo
import parity

pytestmark = pytest.mark.gpu

DEV = "cuda"
MASK = wo.MASK_BIG
SENT = 777.0
INVALID = 1        # hipErrorInvalidValue
up = lambda x: None if x is None else torch.tensor(x, device=DEV)


def _select_outputs(R, greedy=True):
    f = lambda: torch.full((R,), SENT, device=DEV)
    i = lambda: torch.full((R,), 777, dtype=torch.int32, device=DEV)
    return dict(q_taken=f(), qc_taken=f(), u_next=i(), qc_next=f(), u_greedy=i() if greedy else None, qc_greedy=f() if greedy else None)


def _run_select(c, d, avail=True, avail_next=True, greedy=True):
    from marl_amd import ops
    o = _select_outputs(c.R, greedy)
    ops.wqmix_select(d["q"], d["qc"], d["u"], d["avail"] if avail else None, d["q_en"], d["qc_tgt"], d["avail_next"] if avail_next else None,
                     d["padded"], MASK, o["q_taken"], o["qc_taken"], o["u_next"], o["qc_next"], c.B, c.T, c.N, c.A,
                     u_greedy=o["u_greedy"], qc_greedy=o["qc_greedy"])
    torch.cuda.synchronize()
    return o


def _composition(c, avail=True, avail_next=True):
    """the launches marl_wqmix_select replaces, on inputs whose padded rows are cleaned (the old kernels know no padding) and whose
    out-of-range u is the -1 marl_q_gather reads as 0"""
    from marl_amd import ops
    R, A = c.R, c.A
    clean = lambda x: up(np.where(c.dead[:, None], np.float32(0), x))
    q, qc, q_en, qc_tgt, av, avn = (clean(x) for x in (c.q, c.qc, c.q_en, c.qc_tgt, c.avail, c.avail_next))
    av, avn = (av if avail else None), (avn if avail_next else None)
    u = up(np.where((c.u < 0) | (c.u >= A), -1, c.u).astype(np.int32))
    f = lambda: torch.empty(R, device=DEV)
    i = lambda: torch.empty(R, dtype=torch.int32, device=DEV)
    ref = dict(q_taken=f(), qc_taken=f(), u_next=i(), qc_next=f(), u_greedy=i(), qc_greedy=f())
    ops.q_gather(q, u, ref["q_taken"], R, A)
    ops.q_gather(qc, u, ref["qc_taken"], R, A)
    ops.q_masked_max(q, av, MASK, None, ref["u_greedy"], R, A)
    ops.q_gather(qc, ref["u_greedy"], ref["qc_greedy"], R, A)
    ops.q_double_select(q_en, qc_tgt, avn, MASK, ref["qc_next"], ref["u_next"], R, A)
    torch.cuda.synchronize()
    return ref


@pytest.mark.parametrize("shape", wo.SELECT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_select_equals_the_four_launches_bit_for_bit(shape):
    c = wo.select_case(*shape)
    d = {k: up(getattr(c, k)) for k in ("q", "qc", "q_en", "qc_tgt", "avail", "avail_next", "u", "padded")}
    live, dead = up(~c.dead), up(c.dead)
    for avail, avail_next in ((True, True), (False, True), (True, False), (False, False)):
        got, ref = _run_select(c, d, avail, avail_next), _composition(c, avail, avail_next)
        for k, x in got.items():
            assert torch.equal(x[live], ref[k][live]), (shape, avail, avail_next, k)
            assert bool((x[dead] == (-1 if x.dtype == torch.int32 else 0)).all()), (shape, k)        # exact zeros, -1 for the indices
        if c.bare is not None and avail and avail_next:
            assert got["u_next"][c.bare] == 0 and got["u_greedy"][c.bare] == 0 and got["qc_next"][c.bare] == MASK
            assert got["qc_greedy"][c.bare] == d["qc"][c.bare, 0]
            assert got["q_taken"][c.stray] == 0 and got["qc_taken"][c.stray] == 0
        # the OW form: no greedy outputs, the other four to the same bits; and again: the same bits
        ow, again = _run_select(c, d, avail, avail_next, greedy=False), _run_select(c, d, avail, avail_next)
        for k in ("q_taken", "qc_taken", "u_next", "qc_next"):
            assert torch.equal(ow[k], got[k]), k
        assert all(torch.equal(again[k], got[k]) for k in got)


def _loss_inputs(c, finite=False):
    """device inputs; finite: the padded rows hold 1.0 where the case has NaN (marl_td_loss multiplies them by the zero mask)"""
    fix = (lambda x: None if x is None else np.where(c.dead, np.float32(1), x)) if finite else (lambda x: x)
    return dict(q_tot=up(fix(c.q_tot)), qc=up(fix(c.qc)), qc_g=up(fix(c.qc_g)), qn=up(fix(c.qn)), r=up(fix(c.r)), term=up(c.term),
                padded=up(c.padded), u=up(c.u), ug=up(c.ug))


def _run_loss(c, d, alpha, gamma=wo.GAMMA):
    from marl_amd import ops
    f = lambda: torch.full((c.rows,), SENT, device=DEV)
    o = dict(dq_tot=f(), dqc=f(), w=f(), out4=torch.full((4,), SENT, device=DEV))
    ops.wqmix_loss(d["q_tot"], d["qc"], d["qc_g"], d["qn"], d["r"], d["term"], d["padded"], gamma, d["u"] if c.cw else None,
                   d["ug"] if c.cw else None, alpha, o["dq_tot"], o["dqc"], o["out4"], c.rows, c.N, w=o["w"])
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("cw", [False, True], ids=["ow", "cw"])
@pytest.mark.parametrize("rows", wo.LOSS_ROWS)
def test_loss_against_the_float64_contract(rows, cw):
    c = wo.loss_case(rows, 5 if rows < 1000 else 3, cw)
    alpha = 0.75 if cw else 0.5
    d = _loss_inputs(c)                                      # NaN on the padded rows
    got, ref = _run_loss(c, d, alpha), wo.loss_oracle(c, alpha)
    case = "wqmix_loss:%s[%d]" % ("cw" if cw else "ow", rows)
    assert np.array_equal(got["w"].cpu().numpy().astype(np.float64), ref.w)
    parity.close(case, "dq_tot", got["dq_tot"].cpu().numpy(), ref.dq_tot)
    parity.close(case, "dqc", got["dqc"].cpu().numpy(), ref.dqc)
    out4 = got["out4"].cpu().numpy().astype(np.float64)
    print(case, "out4", out4, "ref", ref.out4)
    parity.close(case, "sum w (m td)^2", out4[0], ref.out4[0])
    parity.close(case, "sum (m tdc)^2", out4[2], ref.out4[2])
    assert out4[1] == ref.out4[1] and out4[3] == ref.out4[3] <= out4[1]
    dead = up(c.dead)
    for k in ("dq_tot", "dqc", "w"):                         # exact zeros where the inputs hold NaN
        assert bool((got[k][dead] == 0).all()), k
    again = _run_loss(c, d, alpha)
    assert all(torch.equal(again[k], got[k]) for k in got)   # no float atomics: the same bits


@pytest.mark.parametrize("cw", [False, True], ids=["ow", "cw"])
@pytest.mark.parametrize("rows", wo.LOSS_ROWS)
def test_loss_at_alpha_one_equals_td_loss_bit_for_bit(rows, cw):
    from marl_amd import ops
    c = wo.loss_case(rows, 5 if rows < 1000 else 3, cw)
    d = _loss_inputs(c, finite=True)
    got = _run_loss(c, d, 1.0)
    for q, dq_key, slot in ((d["q_tot"], "dq_tot", 0), (d["qc"], "dqc", 2)):
        dq, out2 = torch.empty(rows, device=DEV), torch.empty(2, device=DEV)
        ops.td_loss(q, d["qn"], d["r"], d["term"], d["padded"], wo.GAMMA, dq, out2, rows)
        torch.cuda.synchronize()
        assert torch.equal(got[dq_key], dq), dq_key
        assert got["out4"][slot] == out2[0] and got["out4"][1] == out2[1], (dq_key, got["out4"], out2)
    assert got["out4"][3] == got["out4"][1] and bool((got["w"][up(~c.dead)] == 1).all())
    # the padded rows' finite values add nothing: the NaN inputs give the same bits
    nan = _run_loss(c, _loss_inputs(c), 1.0)
    assert all(torch.equal(nan[k], got[k]) for k in got)


# ------------------------------------------------------------------------------------------------ refusals
def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _select_args(c, d, o, **over):
    a = dict(q=d["q"], qc=d["qc"], u=d["u"], avail=d["avail"], q_en=d["q_en"], qc_tgt=d["qc_tgt"], avail_next=d["avail_next"],
             padded=d["padded"], q_taken=o["q_taken"], qc_taken=o["qc_taken"], u_greedy=o["u_greedy"], qc_greedy=o["qc_greedy"],
             u_next=o["u_next"], qc_next=o["qc_next"], B=c.B, T=c.T, N=c.N, A=c.A)
    a.update(over)
    return a


def _call_select(a):
    from marl_amd import _lib
    p = lambda k: _ptr(a[k])
    return _lib.load().marl_wqmix_select(p("q"), p("qc"), p("u"), p("avail"), p("q_en"), p("qc_tgt"), p("avail_next"), p("padded"),
                                         C.c_float(MASK), p("q_taken"), p("qc_taken"), p("u_greedy"), p("qc_greedy"), p("u_next"),
                                         p("qc_next"), a["B"], a["T"], a["N"], a["A"], None)


def test_select_refusals_launch_nothing():
    c = wo.select_case(3, 5, 5, 11)
    d = {k: up(getattr(c, k)) for k in ("q", "qc", "q_en", "qc_tgt", "avail", "avail_next", "u", "padded")}
    o = _select_outputs(c.R)
    bad = [dict(N=17), dict(N=0), dict(A=33), dict(A=0), dict(B=1 << 15, T=1 << 15, N=2)]
    bad += [{k: None} for k in ("q", "qc", "u", "q_en", "qc_tgt", "padded", "q_taken", "qc_taken", "u_next", "qc_next")]
    bad += [dict(q_taken=d["q"]), dict(qc_next=d["qc_tgt"]), dict(u_next=d["u"]), dict(qc_taken=o["q_taken"]),
            dict(qc_greedy=d["avail"]), dict(u_greedy=o["u_next"]), dict(q_taken=d["padded"])]
    for over in bad:
        assert _call_select(_select_args(c, d, o, **over)) == INVALID, over
    for over in (dict(B=0), dict(T=0), dict(B=-1)):
        assert _call_select(_select_args(c, d, o, **over)) == 0, over
    torch.cuda.synchronize()
    for k, x in o.items():
        assert bool((x == 777).all()), k
    assert _call_select(_select_args(c, d, o)) == 0                     # and the same arguments, unchanged, run
    torch.cuda.synchronize()
    assert not bool((o["q_taken"] == 777).any())


def _call_loss(a):
    from marl_amd import _lib
    p = lambda k: _ptr(a[k])
    return _lib.load().marl_wqmix_loss(p("q_tot"), p("qc"), p("qc_g"), p("qn"), p("r"), p("term"), p("padded"), C.c_float(wo.GAMMA),
                                       p("u"), p("ug"), C.c_float(a["alpha"]), p("dq_tot"), p("dqc"), p("w"), p("out4"), p("ws"),
                                       C.c_long(a["rows"]), a["N"], None)


def test_loss_refusals_launch_nothing():
    from marl_amd import _lib
    c = wo.loss_case(65, 5, True)
    d = _loss_inputs(c, finite=True)
    f = lambda n=65: torch.full((n,), SENT, device=DEV)
    o = dict(dq_tot=f(), dqc=f(), w=f(), out4=f(4), ws=f(_lib.load().marl_loss_workspace(65) // 4))
    base = dict(d, **o, alpha=0.75, rows=65, N=5)
    bad = [dict(N=0), dict(N=17), dict(alpha=-0.1), dict(alpha=1.1), dict(alpha=float("nan")), dict(rows=1 << 31)]
    bad += [{k: None} for k in ("q_tot", "qc", "qn", "r", "term", "padded", "dq_tot", "dqc", "out4", "ws", "u", "ug")]
    bad += [dict(dq_tot=d["q_tot"]), dict(dqc=o["dq_tot"]), dict(w=d["padded"]), dict(out4=o["ws"]), dict(dqc=d["qc_g"]),
            dict(w=o["dq_tot"]), dict(out4=d["r"])]
    for over in bad:
        assert _call_loss(dict(base, **over)) == INVALID, over
    for over in (dict(rows=0), dict(rows=-5)):
        assert _call_loss(dict(base, **over)) == 0, over
    torch.cuda.synchronize()
    for k, x in o.items():
        assert bool((x == SENT).all()), k
    assert _call_loss(dict(base, qc_g=None, u=None, ug=None)) == 0      # OW needs neither u nor u_greedy
    torch.cuda.synchronize()
    assert not bool((o["dq_tot"] == SENT).any()) and float(o["out4"][3]) <= float(o["out4"][1])
