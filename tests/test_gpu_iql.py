"""csrc/iql.hip on the MI355X against tests/iql_oracle.py (float64): marl_iql_loss_bwd in its one-step and its ret mode and
marl_iql_select, at every action count around the three staging switches (21 | 22 with three row operands, 31 | 33 with two,
63 | 64 with one), one, three and ten agents, one row up to 385 rows (two workgroups, a partly filled last wave).  Needs a real MI355X: ``pytest -m gpu``.

Per-row reads and comparisons (q_taken, q_next) equal marl_q_gather / marl_q_double_select / marl_q_masked_max bit for bit on live
rows; the tie rows of the case hold different q_tgt values at the tied columns, so q_next shows the tie order.  dq_val is held to 8 * 2^-24 * (|r| + gamma |q_next| + |q_taken|) of float64: fewer than four fp32 roundings lie on the path
(gamma q_next, its product with 1 - term, + r, - q_taken; m is 0 or 1 and the factor 2 is exact), the bound leaves a factor 2.  The
numerator of the loss gets the bound tests/test_gpu_rowwise.py gives marl_td_loss's: rowwise_oracle.K_TD_NUM u times the sum of the
squared magnitudes; the denominator is exact.  Every output is a view of a longer sentinel-filled buffer whose tail must be intact."""
import numpy as np
import pytest
import torch

import iql_oracle as io
import rowwise_oracle as ro

pytestmark = pytest.mark.gpu

SENT, PAD = -77.25, 16
INVALID = 1          # hipErrorInvalidValue


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from marl_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def cu(x, dev, off=0):
    """x on the device; off: that many elements off the 16-byte grid"""
    x = np.ascontiguousarray(x)
    whole = torch.zeros(x.size + off + 4, dtype=torch.from_numpy(x).dtype, device=dev)
    v = whole[off:off + x.size].view(*x.shape)
    v.copy_(torch.from_numpy(x))
    return v


def out_buf(dev, n):
    whole = torch.full((n + PAD,), SENT, device=dev)
    return whole, whole[:n]


def tail_ok(whole, n):
    return bool((whole[n:] == SENT).all())


def host(t):
    return t.detach().cpu().numpy()


class Dev:
    """a kernel case's inputs on the device"""

    def __init__(self, c, dev, off_sel=0):
        self.c, self.dev = c, dev
        self.q, self.u, self.q_tgt, self.avail = cu(c.q, dev), cu(c.u, dev), cu(c.q_tgt, dev), cu(c.avail, dev)
        self.q_sel = cu(c.q_sel, dev, off_sel)
        self.r, self.term, self.padded, self.ret = cu(c.r, dev), cu(c.term, dev), cu(c.padded, dev), cu(c.ret, dev)


def fused(d, double_q=True, avail=True, ret=False, debug=True):
    """marl_iql_loss_bwd -> dict of host arrays (dq_val, q_taken, q_next, out2)"""
    from marl_amd import ops
    c = d.c
    bufs = {k: out_buf(d.dev, n) for k, n in (("dq_val", c.R), ("q_taken", c.R), ("q_next", c.R), ("out2", 2))}
    bufs["out2"][1].fill_(3.5)                           # overwritten, not accumulated into
    ops.iql_loss_bwd(d.q, d.u, d.q_sel if double_q and not ret else None, None if ret else d.q_tgt, d.avail if avail and not ret else None,
                     d.ret if ret else None, None if ret else d.r, None if ret else d.term, d.padded, io.GAMMA, io.MASK_BIG,
                     bufs["dq_val"][1], bufs["out2"][1], c.B, c.T, c.N, c.A,
                     q_taken=bufs["q_taken"][1] if debug else None, q_next=bufs["q_next"][1] if debug else None)
    torch.cuda.synchronize()
    for k, (whole, v) in bufs.items():
        assert tail_ok(whole, v.numel()), k
    if not debug or ret:
        assert bool((bufs["q_next"][0] == SENT).all()), "q_next is optional (and not written in ret mode)"
    if not debug:
        assert bool((bufs["q_taken"][0] == SENT).all())
    return {k: host(v).copy() for k, (_, v) in bufs.items()}


def select(d, double_q=True, avail=True, want_taken=True):
    from marl_amd import ops
    c = d.c
    wt, qt = out_buf(d.dev, c.R)
    wn, qn = out_buf(d.dev, c.R)
    ops.iql_select(d.q, d.u, d.q_sel if double_q else None, d.q_tgt, d.avail if avail else None, d.padded, io.MASK_BIG,
                   qt if want_taken else None, qn, c.B, c.T, c.N, c.A)
    torch.cuda.synchronize()
    assert tail_ok(wt, c.R) and tail_ok(wn, c.R)
    if not want_taken:
        assert bool((wt == SENT).all())
    return host(qt).copy(), host(qn).copy().reshape(c.B, c.N, c.T)


def reference(c, double_q=True, avail=True, ret=False):
    r = torch.tensor(c.ret.astype(np.float64)).permute(0, 2, 1).reshape(-1) if ret else None
    return io.rows(c.q, c.u, c.q_sel if double_q else None, c.q_tgt, c.avail if avail else None, c.r, c.term, c.padded, io.GAMMA, c.N,
                   ret=r)


def existing_kernels(d, double_q, avail):
    """q_taken and q_next of the three launches the fused pass replaces (padded rows read NaN: only live rows are compared)"""
    from marl_amd import ops
    c = d.c
    qt, qn = torch.zeros(c.R, device=d.dev), torch.zeros(c.R, device=d.dev)
    ops.q_gather(d.q, d.u, qt, c.R, c.A)
    av = d.avail if avail else None
    if double_q:
        ops.q_double_select(d.q_sel, d.q_tgt, av, io.MASK_BIG, qn, None, c.R, c.A)
    else:
        ops.q_masked_max(d.q_tgt, av, io.MASK_BIG, qn, None, c.R, c.A)
    torch.cuda.synchronize()
    return host(qt), host(qn)


def check(c, got, o, ret=False, what=""):
    """the outputs of one marl_iql_loss_bwd call against the oracle's"""
    live, dead = ~c.dead, c.dead
    for k in ("dq_val", "q_taken") + (() if ret else ("q_next",)):
        assert np.isfinite(got[k]).all(), (what, k)
        assert (got[k][dead] == 0).all(), (what, k)                              # padded rows: exact zeros
    qt64, qn64 = o.q_taken.numpy(), o.q_next.numpy()
    assert (got["q_taken"].astype(np.float64) == qt64).all(), what           # a read: exact
    if ret:
        mag = np.abs(np.where(live, np.nan_to_num(c.ret.transpose(0, 2, 1).reshape(-1).astype(np.float64)), 0)) + np.abs(qt64)
    else:
        assert (got["q_next"].astype(np.float64) == qn64).all(), what        # reads and comparisons: exact
        mag = np.repeat(np.abs(c.r.astype(np.float64)), c.N) + io.GAMMA * np.abs(qn64) + np.abs(qt64)
    err = np.abs(got["dq_val"].astype(np.float64) - o.dq_val.numpy())
    bound = 8 * io.U * mag
    frac = float((err[live] / bound[live]).max()) if live.any() and (bound[live] > 0).all() else 0.0
    print("%s dq_val: worst %.3f of 8 u (|r| + gamma |q_next| + |q_taken|)" % (what, frac))
    assert (err[live] <= bound[live]).all(), "%s: dq_val at %.3f of the bound" % (what, frac)
    assert float(got["out2"][1]) == float(o.den), what                        # N sum m: exact
    num_err, num_bound = abs(float(got["out2"][0]) - float(o.num)), ro.K_TD_NUM * ro.U * float(o.mag_num)
    print("%s sum m td^2: %.3f of the bound %g u mag" % (what, num_err / num_bound if num_bound else 0.0, ro.K_TD_NUM))
    assert num_err <= num_bound, (what, num_err, num_bound)


def run_case(dev, B, T, N, A, seed=0):
    c = io.kernel_case(B, T, N, A, seed=seed)
    d = Dev(c, dev)
    what = "iql B%d T%d N%d A%d" % (B, T, N, A)
    first = None
    for double_q, avail in ((True, True), (False, True), (True, False), (False, False)):
        w = "%s dq=%d avail=%d" % (what, double_q, avail)
        got = fused(d, double_q, avail)
        check(c, got, reference(c, double_q, avail), what=w)
        live = ~c.dead
        qt, qn = existing_kernels(d, double_q, avail)
        assert got["q_taken"][live].tobytes() == qt[live].tobytes(), w
        assert got["q_next"][live].tobytes() == qn[live].tobytes(), w
        # the selection half alone: (B, N, T) layout, the same bits
        st, sn = select(d, double_q, avail)
        assert st.tobytes() == got["q_taken"].tobytes(), w
        assert np.ascontiguousarray(sn.transpose(0, 2, 1)).reshape(-1).tobytes() == got["q_next"].tobytes(), w
        if first is None:
            first = got
            again = fused(d, double_q, avail)                                 # two calls: the same bits
            assert all(first[k].tobytes() == again[k].tobytes() for k in first), w
            lean = fused(d, double_q, avail, debug=False)                      # the optional outputs left out
            assert lean["dq_val"].tobytes() == first["dq_val"].tobytes() and lean["out2"].tobytes() == first["out2"].tobytes()
    got = fused(d, ret=True)
    check(c, got, reference(c, ret=True), ret=True, what=what + " ret")
    assert got["q_taken"].tobytes() == first["q_taken"].tobytes()
    again = fused(d, ret=True)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)
    return c, d, first


@pytest.mark.parametrize("B,T", io.BT_SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("N", io.N_SIZES)
@pytest.mark.parametrize("A", io.A_SIZES)
def test_loss_bwd_and_select_vs_oracle(dev, A, N, B, T):
    run_case(dev, B, T, N, A, seed=A + N)


@pytest.mark.parametrize("A", io.A_SIZES + io.A_TWO_OPERANDS + io.A_ONE_OPERAND)
def test_two_workgroups_and_a_partly_filled_wave(dev, A):
    """R = 385 = 64 * 6 + 1 rows: seven wave tiles over two workgroups, the last tile holds one row.  A = 31 | 33 brackets the staging
    switch of the calls with two row operands (q_sel or avail_next NULL; with three it lies at 21 | 22), A = 63 | 64 that of the
    calls with one (both NULL): 63 is the largest staged tile, 4 waves x 4032 floats"""
    B, T, N = io.BIG
    run_case(dev, B, T, N, A, seed=A)


def test_an_operand_off_the_16_byte_grid(dev):
    B, T, N = io.BIG
    c = io.kernel_case(B, T, N, 11, seed=5)
    a = fused(Dev(c, dev))
    d = Dev(c, dev, off_sel=1)
    assert d.q_sel.data_ptr() % 16 == 4
    b = fused(d)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_more_tiles_than_one_sweep_of_the_grid(dev):
    """1024 workgroups x 4 waves x 64 rows = 262 144 rows per sweep: the grid-stride loop and the 1024 rows of partial sums"""
    B, T, N, A = 1311, 40, 5, 11                      # R = 262 200
    c = io.kernel_case(B, T, N, A, seed=9)
    got = fused(Dev(c, dev))
    check(c, got, reference(c), what="iql second sweep")


def test_invalid_arguments(dev):
    from marl_amd import _lib, ops
    lib, s = _lib.load(), ops._stream
    c = io.kernel_case(3, 5, 3, 11)
    d = Dev(c, dev)
    p = ops._p
    outs = [torch.full((c.R + PAD,), SENT, device=dev) for _ in range(3)]
    out2 = torch.full((2,), SENT, device=dev)
    ws = ops.WS.get("loss", lib.marl_loss_workspace(c.R), dev)
    good = dict(q=d.q, u=d.u, q_sel=d.q_sel, q_tgt=d.q_tgt, avail=d.avail, ret=None, r=d.r, term=d.term, padded=d.padded,
                dq_val=outs[0], q_taken=outs[1], q_next=outs[2], out2=out2, ws=ws, B=c.B, T=c.T, N=c.N, A=c.A)

    def loss(**over):
        k = dict(good, **over)
        return lib.marl_iql_loss_bwd(p(k["q"]), p(k["u"]), p(k["q_sel"]), p(k["q_tgt"]), p(k["avail"]), p(k["ret"]), p(k["r"]), p(k["term"]),
                                     p(k["padded"]), io.GAMMA, io.MASK_BIG, p(k["dq_val"]), p(k["q_taken"]), p(k["q_next"]), p(k["out2"]),
                                     p(k["ws"]), k["B"], k["T"], k["N"], k["A"], s())

    def sel(**over):
        k = dict(good, **over)
        return lib.marl_iql_select(p(k["q"]), p(k["u"]), p(k["q_sel"]), p(k["q_tgt"]), p(k["avail"]), p(k["padded"]), io.MASK_BIG,
                                   p(k["q_taken"]), p(k["q_next"]), k["B"], k["T"], k["N"], k["A"], s())

    for name in ("q", "u", "q_tgt", "r", "term", "padded", "dq_val", "out2", "ws"):
        assert loss(**{name: None}) == INVALID, name
    for name in ("q", "u", "padded", "dq_val", "out2", "ws"):                  # the ret mode's required pointers
        assert loss(ret=d.ret, **{name: None}) == INVALID, name
    for name in ("q", "u", "q_tgt", "padded", "q_next"):
        assert sel(**{name: None}) == INVALID, name
    for over in (dict(A=0), dict(N=0), dict(A=-1), dict(N=-3)):
        assert loss(**over) == INVALID and sel(**over) == INVALID, over
    # an output on an input, or on another output
    qbuf = d.q.view(-1)
    for over in (dict(dq_val=qbuf), dict(q_taken=d.q_tgt.view(-1)), dict(q_next=d.avail.view(-1)), dict(q_next=outs[0]), dict(q_taken=outs[0][4:]),
                 dict(dq_val=d.r), dict(out2=d.term), dict(out2=outs[0][8:])):
        assert loss(**over) == INVALID, list(over)
    assert loss(ret=d.ret, dq_val=d.ret.view(-1)) == INVALID
    assert sel(q_next=d.q_sel.view(-1)) == INVALID and sel(q_taken=outs[2]) == INVALID
    torch.cuda.synchronize()
    assert all(bool((o == SENT).all()) for o in outs + [out2]), "a refused call wrote something"
    for x, w in ((d.q, c.q), (d.q_tgt, c.q_tgt), (d.avail, c.avail)):
        assert host(x).tobytes() == w.tobytes()
    # empty shapes: 0, no launch, nothing looked at
    for over in (dict(B=0), dict(T=0), dict(B=-2)):
        assert loss(**over) == 0 and sel(**over) == 0
    assert lib.marl_iql_loss_bwd(None, None, None, None, None, None, None, None, None, 0.99, -1.0, None, None, None, None, None, 0, 5, 3, 11, s()) == 0
    assert lib.marl_iql_select(None, None, None, None, None, None, -1.0, None, None, 4, 0, 3, 11, s()) == 0
    torch.cuda.synchronize()
    assert all(bool((o == SENT).all()) for o in outs + [out2])
    assert loss() == 0                                                         # and the table of good arguments is one
    torch.cuda.synchronize()
    assert not bool((outs[0][:c.R] == SENT).any()) and bool((outs[0][c.R:] == SENT).all())
