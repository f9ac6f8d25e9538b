"""Everything QTRAN trains through and the two-hyper-layer QMIX tail - the kernels of csrc/qtran_fused.hip behind marl_qtran_head_fwd /
_fwd2 / _bwd, marl_qtran_state_parts, marl_qmix_tail_fwd and marl_qtran_wgrad_rows - against the float64 statement of each operation
(tests/qtran_oracle.py) at every seam of the launch code: the second and third tile round of the head kernels (beyond 32 768 rows),
the agent walk at N = 1 .. 4, action values outside [0, A), A = 1 and A = 16, every chunk bucket of the state-part kernel for one and
two weight sets and its equal-share rounds, the four row-gradient instantiations, their multi-block walk and 256-slab reduce, and
the Python wiring of the mixer modules.  Needs a real MI355X: ``pytest -m gpu``.

Every test first ASKS THE LIBRARY which plan it will run (marl_qtran_plan: the host functions the launches themselves decide with) and
fails with "the plan moved" if that is not the plan its shape was picked for.  Every output, saved activation and workspace is a view
into a longer sentinel-filled buffer whose tail must be intact; for S % 4 != 0 the states sit in 16-byte padded rows whose pad is NaN.
  exact data   == float64 (small integers: any summation order gives the same bits; relu pre-activations of exactly 0 are frequent)
  probe data   heads: exact data on the seam rows alone; row kernels: |got - ref| <= (nnz + 3) u sum |terms|, all-zero elements exact
  real data    forward values: the running error bound of qtran_oracle.forward, k = 1; gradients: the ceilings of the older tests,
               against float64, the used fraction printed beside fp32 torch-CPU's own error against the same reference
Every backward and every weight gradient runs twice into fresh buffers: the same bits."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import parity
import qtran_oracle as qo
from test_gpu_dense import padded
from test_gpu_rowwise import SENT, held, host, out_buf, same, tail_ok
from test_qtran_oracle_cpu import head_got, module_weights

pytestmark = pytest.mark.gpu
NS = types.SimpleNamespace
U = qo.U


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from marl_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def cu(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def ceiling(case, name, got, ref, ceil, cpu=None):
    """|got - ref| <= ceil per element (a ceiling of the older tests); the used fraction is printed and recorded, beside fp32 torch-CPU's"""
    got = host(got).astype(np.float64) if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (case, name, got.shape, ref.shape)
    assert np.isfinite(got).all(), (case, name)
    frac = np.abs(got - ref) / ceil
    own = "" if cpu is None else "; fp32 torch-CPU %.4f" % (np.abs(np.asarray(cpu, np.float64).reshape(ref.shape) - ref) / ceil).max()
    print("%s / %s: worst %.4f of the ceiling%s" % (case, name, frac.max() if frac.size else 0.0, own))
    assert (frac <= 1.0).all(), "%s / %s: %.3f of the ceiling at %d" % (case, name, frac.max(), frac.argmax())
    parity.close(case, name + own, frac, np.zeros_like(frac), tol=1.0, scale=1.0)


def qt_struct(w, dev, S):
    """marl_qtran_weights_t over device copies of an oracle weight set"""
    from marl_amd._lib import MarlQtranWeights
    t = {k: cu(np.asarray(getattr(w, k), np.float32), dev) for k in qo.WNAMES}
    st = MarlQtranWeights()
    for k in ("enc0", "enc2", "q2", "q4"):
        setattr(st, k + "_w", t[k + "_w"].data_ptr())
        setattr(st, k + "_b", t[k + "_b"].data_ptr())
    st.q0_w, st.q0_ld, st.q0_s = t["q0_w"].data_ptr(), t["q0_w"].shape[1], S
    st._keep = t
    return st


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def cpu32_head_grads(i, c):
    """fp32 torch-CPU autograd of the reference composition (per-agent encoder, agent sum, head) on the same inputs"""
    w = {k: torch.from_numpy(np.asarray(getattr(i.w, k), np.float32)).clone().requires_grad_() for k in qo.WNAMES}
    h = torch.from_numpy(i.h).clone().requires_grad_()
    x = torch.cat([h, torch.from_numpy(qo.onehot(i.u, c.A).astype(np.float32))], 1) if c.A else h
    e1 = torch.relu(x @ w["enc0_w"].t() + w["enc0_b"])
    e2 = (e1 @ w["enc2_w"].t() + w["enc2_b"]).view(c.BT, c.N, -1).sum(1)
    y1 = torch.relu(torch.from_numpy(i.sp) + e2 @ w["q0_w"][:, c.S:].t())
    y2 = torch.relu(y1 @ w["q2_w"].t() + w["q2_b"])
    out = y2 @ w["q4_w"].view(-1) + w["q4_b"]
    (out * torch.from_numpy(i.d_out)).sum().backward()
    return NS(dhidden=h.grad.numpy(), enc0_w=w["enc0_w"].grad.numpy(), enc0_b=w["enc0_b"].grad.numpy(), enc2_b=w["enc2_b"].grad.numpy())


# ================================================================================================ the heads
def run_head(ops, dev, c, kind):
    from marl_amd import _lib
    lib = _lib.load()
    what = "%s[%s]" % (c.name, kind)
    case = "qtran head %s [%s]" % (c.name, kind)
    i = qo.head_inputs(c.name, kind)
    BT, N, A, AE = c.BT, c.N, c.A, c.AE
    AEP, R = (AE + 15) // 16 * 16, BT * N
    for w_ in ("fwd", "bwd") + (("fwd2",) if A else ()):
        pl = ops.qtran_plan(w_, BT, N=N, A=A, AE=AE)
        assert pl is not None and head_got(pl) == qo.head_plan(c, w_), "the plan moved: %s %s runs %r" % (what, w_, pl)
    st = qt_struct(i.w, dev, c.S)
    hd, spd = cu(i.h, dev), cu(i.sp, dev)
    ud = cu(i.u, dev) if A else None
    exact = kind != "real"
    f, g = i.f, i.g

    def fwd_bufs():
        b = NS()
        for k, shp in (("out", (BT,)), ("out2", (BT,)), ("s1", (BT, AEP)), ("e2", (BT, AEP)), ("y1", (BT, 64)), ("y2", (BT, 64))):
            whole, v = out_buf(dev, shp)
            setattr(b, "w_" + k, whole); setattr(b, k, v)
        return b

    def check_fwd(b, dual):
        torch.cuda.synchronize()
        for k in ("out", "s1", "e2", "y1", "y2") + (("out2",) if dual else ()):
            assert tail_ok(getattr(b, "w_" + k), getattr(b, k).numel()), "%s: wrote outside %s" % (what, k)
        assert bool((b.s1[:, AE:] == 0).all()) and bool((b.e2[:, AE:] == 0).all()), what + ": pad columns of s1 / e2"
        for k, ref, err in (("s1", f.s1, f.err_s1), ("e2", f.e2, f.err_e2), ("y1", f.y1, f.err_y1), ("y2", f.y2, f.err_y2),
                            ("out", f.out, f.err_out)):
            got = getattr(b, k)[:, :AE] if k in ("s1", "e2") else getattr(b, k)
            if exact:
                same(got, ref, "%s %s" % (what, k))
            else:
                held(case, ("fwd2 " if dual else "fwd ") + k, got, ref, err / U, 1.0)
        if dual:
            if exact:
                same(b.out2, i.f2.out, what + " out2")
            else:
                keep = ~i.kink2
                held(case, "fwd2 out2", host(b.out2)[keep], i.f2.out[keep], i.f2.err_out[keep] / U, 1.0)

    b1 = fwd_bufs()
    ops.qtran_head_fwd(st, hd, ud, spd, b1.out, b1.s1, b1.e2, b1.y1, b1.y2, BT, N, A, AE)
    check_fwd(b1, False)
    assert bool((b1.w_out2 == SENT).all())
    # nothing saved: the same output bits
    wn, on = out_buf(dev, (BT,))
    ops.qtran_head_fwd(st, hd, ud, spd, on, None, None, None, None, BT, N, A, AE)
    torch.cuda.synchronize()
    assert tail_ok(wn, BT) and torch.equal(on, b1.out), what + ": forward without saving"
    if A:
        b2 = fwd_bufs()
        ops.qtran_head_fwd2(st, hd, ud, cu(i.u2, dev), spd, b2.out, b2.out2, b2.s1, b2.e2, b2.y1, b2.y2, BT, N, A, AE)
        check_fwd(b2, True)
        for k in ("out", "s1", "e2", "y1", "y2"):
            assert torch.equal(getattr(b1, k), getattr(b2, k)), "%s: fwd2's first set %s is not the single call's" % (what, k)

    # ---- backward from the activations the forward has just saved
    dd = cu(i.d_out, dev)
    ws_bytes = lib.marl_qtran_bwd_workspace(BT, AE)
    rng = np.random.default_rng(qo.case_seed(what))
    base = NS(dhidden=rng.integers(-3, 4, size=(R, 64)).astype(np.float32), enc0_w=rng.integers(-3, 4, size=(AE, AE)).astype(np.float32),
              enc0_b=rng.integers(-3, 4, size=AE).astype(np.float32), enc2_b=rng.integers(-3, 4, size=AE).astype(np.float32))

    def bwd(accumulate):
        o = NS()
        for k, shp in (("dy1", (BT, 64)), ("dy2", (BT, 64)), ("de2", (BT, AEP)), ("dhidden", (R, 64)), ("enc0_w", (AE, AE)), ("enc0_b", (AE,)),
                       ("enc2_b", (AE,)), ("ws", (ws_bytes // 4,))):
            whole, v = out_buf(dev, shp)
            setattr(o, "w_" + k, whole); setattr(o, k, v)
        for k in ("enc0_w", "enc0_b", "enc2_b"):
            getattr(o, k).copy_(cu(getattr(base, k), dev))
        if accumulate:
            o.dhidden.copy_(cu(base.dhidden, dev))
        rc = lib.marl_qtran_head_bwd(C.byref(st), p(hd), p(ud), p(dd), p(b1.y1), p(b1.y2), p(o.dy1), p(o.dy2), p(o.de2), p(o.dhidden),
                                     1 if accumulate else 0, p(o.enc0_w), p(o.enc0_b), p(o.enc2_b), p(o.ws), ws_bytes, BT, N, A, AE, stream())
        assert rc == 0, (what, rc)
        torch.cuda.synchronize()
        for k in ("dy1", "dy2", "de2", "dhidden", "enc0_w", "enc0_b", "enc2_b", "ws"):
            assert tail_ok(getattr(o, "w_" + k), getattr(o, k).numel()), "%s: wrote outside %s" % (what, k)
        return o

    o1, o2 = bwd(0), bwd(0)
    for k in ("dy1", "dy2", "de2", "dhidden", "enc0_w", "enc0_b", "enc2_b"):
        assert torch.equal(getattr(o1, k), getattr(o2, k)), "%s: two runs, different bits in %s" % (what, k)
    assert bool((o1.de2[:, AE:] == 0).all()), what + ": pad columns of de2"
    rows_ref = (("dy2", g.dy2), ("dy1", g.dy1), ("de2", g.de2), ("dhidden", g.dhidden))
    if exact:
        for k, ref in rows_ref:
            same(getattr(o1, k)[:, :AE] if k == "de2" else getattr(o1, k), ref, "%s %s" % (what, k))
        for k in ("enc0_w", "enc0_b", "enc2_b"):
            same(getattr(o1, k), getattr(base, k).astype(np.float64) + getattr(g, k), "%s d_%s" % (what, k))
        o3 = bwd(1)          # accumulate = 1 onto an integer base: the sum is exact too
        same(o3.dhidden, base.dhidden.astype(np.float64) + g.dhidden, what + " dhidden (accumulate)")
        for k in ("dy1", "dy2", "de2", "enc0_w", "enc0_b", "enc2_b"):
            assert torch.equal(getattr(o1, k), getattr(o3, k)), "%s: accumulate changed %s" % (what, k)
        return
    cpu = cpu32_head_grads(i, c)
    for k, ref in rows_ref:
        got = getattr(o1, k)[:, :AE] if k == "de2" else getattr(o1, k)
        ceiling(case, k, got, ref, qo.dhidden_ceiling(ref), cpu.dhidden if k == "dhidden" else None)
        zero = np.flatnonzero(i.d_out == 0)          # rows without a gradient (the kink rows among them): exact zeros
        if zero.size:
            rr = zero if k != "dhidden" else (zero[:, None] * N + np.arange(N)).reshape(-1)
            assert not host(got)[rr].any(), "%s %s: non-zero in a row whose d_out is 0" % (what, k)
    for k in ("enc0_w", "enc0_b", "enc2_b"):
        ref = getattr(g, k)
        ceiling(case, "d_" + k, host(getattr(o1, k)).astype(np.float64) - getattr(base, k), ref, qo.param_ceiling(ref, R), getattr(cpu, k))
    print("%s: %d of %d rows left out on a relu kink" % (case, int(i.kink.sum()), BT))


HEAD_PARAMS = [(c, k) for c in qo.HEAD_CASES for k in qo.head_kinds(c)]


@pytest.mark.parametrize("c,kind", HEAD_PARAMS, ids=["%s-%s" % (c.name, k) for c, k in HEAD_PARAMS])
def test_heads(dev, c, kind):
    """marl_qtran_head_fwd, _fwd2 (joint-Q) and _bwd on one case: forward values and saved activations, the second action set, the
    output without saving, the row-level backward tensors, dhidden with accumulate 0 / 1 and the gradients of the first encoder layer
    and the second encoder bias accumulated into pre-filled buffers"""
    from marl_amd import ops
    run_head(ops, dev, c, kind)


# ================================================================================================ state parts and the QMIX tail
def dev_states(ops, i, S, dev):
    """the states on the device as the case stores them: dense rows or (T+1)-slot storage behind an episode map; S % 4 != 0: in 16-byte
    padded rows whose pad holds NaN"""
    ld = (S + 3) // 4 * 4
    if i.store is None:
        return padded(i.s, ld, dev)
    flat = padded(i.store.reshape(-1, S), ld, dev)
    return ops.Rows(flat, (i.T, i.T + 1, 1), cu(i.emap, dev))


def sp_layouts(BT):
    return (False, True) if BT in qo.SP_REMAP_BT else (False,)


@pytest.mark.parametrize("nsets", (1, 2))
@pytest.mark.parametrize("S", qo.SP_S)
def test_state_parts(dev, S, nsets):
    """marl_qtran_state_parts at one state width (a chunk bucket from one of its edges), for one or two weight sets, over the batch
    sizes either side of a 64-row block and of the equal-share rounds, dense and through the (T+1)-slot remap with an episode map"""
    from marl_amd import ops
    assert ops.qtran_state_parts_supported(S)
    for BT in qo.SP_BT:
        pl = ops.qtran_plan("state_parts", BT, S=S, nsets=nsets)
        assert pl is not None and (pl.KCT, pl.nsets, pl.grid, pl.rounds) == qo.sp_plan(BT, S, nsets), \
            "the plan moved: state parts S%d BT%d x%d runs %r" % (S, BT, nsets, pl)
        for kind in qo.sp_kinds(BT):
            for remap in sp_layouts(BT):
                what = "sp S%d BT%d x%d [%s]%s" % (S, BT, nsets, kind, " remap" if remap else "")
                i = qo.sp_inputs(S, BT, kind, nsets, remap)
                s = dev_states(ops, i, S, dev)
                assert ops.qtran_state_parts_supported(S, s)
                sets, wholes = [], []
                for k in range(nsets):
                    whole, v = out_buf(dev, (BT, 64))
                    wholes.append(whole)
                    sets.append((cu(i.W[k], dev), cu(i.b[k], dev), v))
                ops.qtran_state_parts(s, BT, S, sets)
                torch.cuda.synchronize()
                for k in range(nsets):
                    assert tail_ok(wholes[k], BT * 64), what + ": wrote outside sp"
                    got = sets[k][2]
                    if kind == "exact":
                        same(got, i.ref[k], what)
                        continue
                    if kind == "probe":          # a zero state row gives the bias itself
                        off = np.ones(BT, bool); off[i.rows] = False
                        same(host(got)[off], np.broadcast_to(i.b[k], (int(off.sum()), 64)), what + " rows of zero states")
                    held("qtran state parts S%d x%d [%s]" % (S, nsets, kind), "BT%d%s set %d" % (BT, " remap" if remap else "", k), got, i.ref[k],
                         i.mag[k], qo.sp_k(S))


@pytest.mark.parametrize("S", qo.SP_S)
def test_qmix_tail(dev, S):
    """marl_qmix_tail_fwd: two plain tiles (hyper_b1) and two relu tiles (hyper_b2.0) at column offsets inside a wider hy - every other
    column of hy still holds the sentinel afterwards"""
    from marl_amd import ops
    LD, CB1, CH = 100, 8, 60
    for BT in qo.SP_BT:
        pl = ops.qtran_plan("qmix_tail", BT, S=S)
        assert pl is not None and (pl.KCT, pl.nsets, pl.grid, pl.rounds) == qo.sp_plan(BT, S, 1), "the plan moved: QMIX tail S%d BT%d runs %r" % (S, BT, pl)
        for kind in ("exact", "real"):
            for remap in sp_layouts(BT):
                what = "tail S%d BT%d [%s]%s" % (S, BT, kind, " remap" if remap else "")
                i = qo.sp_inputs(S, BT, kind, 2, remap, outs=32)
                b1, hh, m1, mh = qo.qmix_tail(i.W[0][:, :S], i.b[0], i.W[1][:, :S], i.b[1], i.s)
                s = dev_states(ops, i, S, dev)
                whole, hy = out_buf(dev, (BT, LD))
                ops.qmix_tail_fwd(s, BT, S, cu(i.W[0], dev), cu(i.b[0], dev), cu(i.W[1], dev), cu(i.b[1], dev), hy, CB1, CH)
                torch.cuda.synchronize()
                assert tail_ok(whole, BT * LD), what + ": wrote outside hy"
                other = torch.ones(LD, dtype=torch.bool, device=dev)
                other[CB1:CB1 + 32] = False
                other[CH:CH + 32] = False
                assert bool((hy[:, other] == SENT).all()), what + ": wrote a column of hy outside its four tiles"
                if kind == "exact":
                    same(hy[:, CB1:CB1 + 32], b1, what + " hyper_b1")
                    same(hy[:, CH:CH + 32], hh, what + " relu(hyper_b2.0)")
                    assert (b1 < 0).any() and (hh == 0).any()
                else:
                    case = "qmix tail S%d [%s]" % (S, kind)
                    held(case, "BT%d%s hyper_b1" % (BT, " remap" if remap else ""), hy[:, CB1:CB1 + 32], b1, m1, qo.sp_k(S))
                    held(case, "BT%d%s relu(hyper_b2.0)" % (BT, " remap" if remap else ""), hy[:, CH:CH + 32], hh, mh, qo.sp_k(S))


# ================================================================================================ row-level weight gradients
@pytest.mark.parametrize("AE", qo.WG_AE)
@pytest.mark.parametrize("S", qo.WG_S)
def test_wgrad_rows(dev, S, AE):
    """marl_qtran_wgrad_rows at one instantiation over the batch sizes either side of a 32-row block and of the 256-workgroup cap: seven
    gradients accumulated into pre-filled buffers (d_q0_w a column block of a wider tensor), twice, the same bits"""
    from marl_amd import _lib, ops
    lib = _lib.load()
    assert ops.qtran_wgrad_rows_supported(S, AE)
    AEP = (AE + 15) // 16 * 16
    ws_bytes = lib.marl_qtran_wgrad_rows_workspace(S, AE)
    shapes = dict(q0_w=(64, S + AE + 4), q0_b=(64,), q2_w=(64, 64), q2_b=(64,), q4_w=(64,), q4_b=(1,), enc2_w=(AE, AE))
    for BT in qo.WG_BT:
        pl = ops.qtran_plan("wgrad_rows", BT, S=S, AE=AE)
        assert pl is not None and (pl.FT, pl.SMAX, pl.grid, pl.rounds, pl.slabs) == qo.wg_plan(BT, S, AE), \
            "the plan moved: wgrad rows S%d AE%d BT%d runs %r" % (S, AE, BT, pl)
        for kind in qo.wg_kinds(BT):
            what = "wg S%d AE%d BT%d [%s]" % (S, AE, BT, kind)
            case = "qtran wgrad rows S%d AE%d [%s]" % (S, AE, kind)
            i = qo.wg_inputs(S, AE, BT, kind)
            t = {k: cu(getattr(i, k), dev) for k in ("s", "s1", "e2", "y1", "y2", "d_out", "dy1", "dy2", "de2")}
            x = ops.src(t["s"])
            runs = []
            for rep in range(2):
                o, wh = {}, {}
                for k, shp in shapes.items():
                    wh[k], o[k] = out_buf(dev, shp)
                wh["ws"], ws = out_buf(dev, (ws_bytes // 4,))
                q0 = o["q0_w"][:, :S + AE]
                for k in qo.ROW_GRADS:
                    (q0 if k == "q0_w" else o[k]).copy_(cu(getattr(i.base, k), dev))
                rc = lib.marl_qtran_wgrad_rows(C.byref(x), p(t["s1"]), p(t["e2"]), p(t["y1"]), p(t["y2"]), p(t["d_out"]), p(t["dy1"]), p(t["dy2"]),
                                               p(t["de2"]), p(q0), q0.stride(0), p(o["q0_b"]), p(o["q2_w"]), p(o["q2_b"]), p(o["q4_w"]),
                                               p(o["q4_b"]), p(o["enc2_w"]), p(ws), ws_bytes, BT, S, AE, stream())
                assert rc == 0, (what, rc)
                torch.cuda.synchronize()
                for k in list(shapes) + ["ws"]:
                    assert tail_ok(wh[k], (ws_bytes // 4) if k == "ws" else int(np.prod(shapes[k]))), "%s: wrote outside %s" % (what, k)
                assert bool((o["q0_w"][:, S + AE:] == SENT).all()), what + ": wrote outside its column block of d_q0_w"
                runs.append({k: host(q0 if k == "q0_w" else o[k]).copy() for k in qo.ROW_GRADS})
            for k in qo.ROW_GRADS:
                assert np.array_equal(runs[0][k], runs[1][k]), "%s: two runs, different bits in d_%s" % (what, k)
                got, base, ref = runs[0][k], getattr(i.base, k).astype(np.float64), getattr(i.g, k)
                if kind == "exact":
                    same(got, base + ref, "%s d_%s" % (what, k))
                elif kind == "probe":
                    held(case, "BT%d d_%s" % (BT, k), got, ref, (getattr(i.g.nnz, k) + 3) * getattr(i.g.mag, k), 1.0)
                else:
                    G, X = dict(q0_w=(i.dy1, np.concatenate([i.s, i.e2[:, :AE]], 1)), q2_w=(i.dy2, i.y1), q4_w=(i.d_out[:, None], i.y2),
                                enc2_w=(i.de2[:, :AE], i.s1[:, :AE]), q0_b=(i.dy1, None), q2_b=(i.dy2, None), q4_b=(i.d_out[:, None], None))[k]
                    G32 = torch.from_numpy(np.ascontiguousarray(G))
                    cpu = (G32.t() @ torch.from_numpy(np.ascontiguousarray(X))).numpy() if X is not None else G32.sum(0).numpy()
                    ceiling(case, "BT%d d_%s" % (BT, k), got.astype(np.float64) - base, ref, qo.param_ceiling(ref, BT), cpu.reshape(ref.shape))


# ================================================================================================ through the modules
@pytest.mark.parametrize("kind", ("exact", "real"))
@pytest.mark.parametrize("c", qo.SEAM_CASES, ids=lambda c: c.name)
def test_through_the_modules(dev, c, kind):
    """QtranQBase / QtranV.hip_forward and hip_backward (the Python wiring of _QtranFusedHead: state part, fused head, row gradients)
    with the fused kernels and with the marl_linear composition (no_fused), against the same oracle"""
    from marl_amd.network.mixer import QtranQBase, QtranV
    from marl_amd.hostutil import FlatParams
    i = qo.head_inputs(c.name, kind)
    BT, N, A, S, R = c.BT, c.N, c.A, c.S, c.BT * c.N
    args = NS(n_agents=N, n_actions=max(A, 1), state_shape=S, rnn_hidden_dim=64, qtran_hidden_dim=64)
    mod = (QtranQBase if c.head == "q" else QtranV)(args)
    _, ls = module_weights(mod, c.head)
    with torch.no_grad():
        for name, lin in zip(("enc0", "enc2", "q0", "q2", "q4"), ls):
            lin.weight.copy_(torch.from_numpy(getattr(i.w, name + "_w")))
            lin.bias.copy_(torch.from_numpy(getattr(i.w, name + "_b")))
    # the generic composition reads a one-hot COLUMN by its index: only -1 stands for "no action" there
    u = None if not A else np.where((i.u >= 0) & (i.u < A), i.u, -1).astype(np.int32)
    sp = qo.state_part(i.w.q0_w, i.w.q0_b, i.s, S)
    err_sp = qo.sp_k(S) * U * (np.abs(i.s.astype(np.float64)) @ np.abs(i.w.q0_w.astype(np.float64))[:, :S].T + np.abs(i.w.q0_b.astype(np.float64)))
    f = qo.forward(i.w, i.h, u, sp, BT, N, A, bound=True, err_sp=err_sp)
    d_out = np.random.default_rng(5).integers(-2, 3, size=BT).astype(np.float32) if kind == "exact" else \
        np.random.default_rng(5).standard_normal(BT).astype(np.float32)
    kink = qo.kink_rows(f)
    if kind == "real":
        assert kink.mean() <= qo.KINK_CAP
        d_out[kink] = 0
    g = qo.backward(i.w, f, i.s, d_out, BT, N, A)
    mod.to(dev)
    fp = FlatParams(list(mod.parameters()), dev, with_grad=True)
    sd, hd, dd = cu(i.s, dev), cu(i.h, dev), cu(d_out, dev)
    ud = cu(u, dev) if A else None
    assert mod._qt_ok(hd)
    base = np.random.default_rng(6).integers(-3, 4, size=fp.n).astype(np.float32)
    for fused in (True, False):
        case = "qtran modules %s [%s] %s" % (c.name, kind, "fused" if fused else "composed")
        mod.no_fused = not fused
        fp.grad.copy_(cu(base, dev))
        ctx = {}
        out = mod.hip_forward(sd, hd, ud, BT, ctx=ctx) if c.head == "q" else mod.hip_forward(sd, hd, BT, ctx=ctx)
        assert bool(ctx.get("fused")) == fused
        whole, dh = out_buf(dev, (R, 64))
        dh.fill_(2.0)
        mod.hip_backward(ctx, dd, BT, dh, accumulate=True)
        torch.cuda.synchronize()
        assert tail_ok(whole, R * 64)
        grads = {}
        for (name, p_), lin_name in zip(mod.named_parameters(), [n + s for n in ("enc0", "enc2", "q0", "q2", "q4") for s in ("_w", "_b")]):
            off = fp.offsets[[id(q) for q in fp.params].index(id(p_))]
            grads[lin_name] = (host(p_.grad).astype(np.float64) - base[off:off + p_.numel()].reshape(p_.shape), getattr(g, lin_name))
        if kind == "exact":
            same(out, f.out, case + " out")
            same(dh, 2.0 + g.dhidden, case + " dhidden")
            for k, (got, ref) in grads.items():
                same(got, ref.reshape(got.shape), "%s d_%s" % (case, k))
            continue
        held(case, "out", out, f.out, f.err_out / U, 1.0)
        ceiling(case, "dhidden", host(dh).astype(np.float64) - 2.0, g.dhidden, qo.dhidden_ceiling(g.dhidden))
        for k, (got, ref) in grads.items():
            ceiling(case, "d_" + k, got, ref.reshape(got.shape), qo.param_ceiling(ref, R))
