"""The glue every update of every learner passes through - marl_replay_gather, the selection / scatter / agent-sum kernels, the QMIX
mixing epilogue, the TD and QTRAN losses (csrc/mixers.hip) and clip + RMSprop / Adam (csrc/optim.hip) - against the float64
statement of each operation (tests/rowwise_oracle.py), at the sizes where the launch code changes behaviour (grid-stride sweeps,
the row-per-thread / LDS-tiled switch, the 1024-float chunks of the gather) and with the arguments include/marl_hip.h documents
(NULL outputs, NULL avail, idx < 0, one scatter pair, padded strides, den == NULL).  Needs a real MI355X: ``pytest -m gpu``.

Every output is a view of a longer buffer pre-filled with a sentinel; the tail must be intact afterwards.  Integers and copied
floats are compared with ==.  Computed floats are held to (operations on the path + 2) * 2^-24 * magnitude per element, the
constants and their derivations being rowwise_oracle.K_* / k_*; tests/test_rowwise_oracle_cpu.py checks that they stay under the
ceilings of the older tests of the same kernels and that the inputs have the edges the cases are named for.  The achieved fraction
of each bound goes through parity.close (terminal summary)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import parity
import rowwise_oracle as ro

pytestmark = pytest.mark.gpu

SENT, ISENT, PAD = -77.25, -777, 16
NS = types.SimpleNamespace
INVALID = 1          # hipErrorInvalidValue


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from marl_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def cu(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def out_buf(dev, shape, dtype=torch.float32, off=0):
    """a sentinel-filled buffer PAD elements longer than `shape` (+ off in front: a view `off` elements off the 16-byte grid)"""
    n = int(np.prod(shape))
    whole = torch.full((off + n + PAD,), ISENT if dtype == torch.int32 else SENT, dtype=dtype, device=dev)
    assert whole.data_ptr() % 16 == 0
    return whole, whole[off:off + n].view(*shape)


def tail_ok(whole, n, off=0):
    s = ISENT if whole.dtype == torch.int32 else SENT
    return bool((whole[off + n:] == s).all()) and bool((whole[:off] == s).all())


def untouched(whole):
    return bool((whole == (ISENT if whole.dtype == torch.int32 else SENT)).all())


def shifted(x, dev, off=1):
    """x on the device, `off` floats off the 16-byte grid"""
    x = np.ascontiguousarray(x)
    whole = torch.zeros(x.size + off + 3, dtype=torch.from_numpy(x).dtype, device=dev)
    v = whole[off:off + x.size].view(*x.shape)
    v.copy_(torch.from_numpy(x))
    assert v.data_ptr() % 16 == 4 * off
    return v


def host(t):
    return t.detach().cpu().numpy()


def same(got, want, what=""):
    got, want = host(got) if torch.is_tensor(got) else np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1).astype(got.dtype))
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %r want %r" % (
        what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def held(case, name, got, ref, mag, k):
    """|got - ref| <= k u mag per element (exactly equal where the magnitude is 0); the worst used fraction is recorded"""
    got = host(got).astype(np.float64) if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    ref, mag = np.asarray(ref, dtype=np.float64), np.broadcast_to(np.asarray(mag, dtype=np.float64), np.shape(ref))
    assert got.shape == ref.shape, (case, name, got.shape, ref.shape)
    assert np.isfinite(got).all(), (case, name)
    err = np.abs(got - ref)
    z = mag == 0
    assert (err[z] == 0).all(), "%s / %s: non-zero where the magnitude is 0" % (case, name)
    frac = np.zeros_like(err)
    frac[~z] = err[~z] / (k * ro.U * mag[~z])
    print("%s / %s: worst %.3f of the bound %g u mag" % (case, name, frac.max() if frac.size else 0.0, k))
    assert (frac <= 1.0).all(), "%s / %s: %.3f of the bound (%g u x magnitude) at %d" % (case, name, frac.max(), k, frac.argmax())
    parity.close(case, name, frac, np.zeros_like(frac), tol=1.0, scale=1.0)


# =========================================================================================== replay gather
def _ring_on_device(dev, ring):
    from marl_amd.env.synthetic_smac import EpisodeRecord
    rec = EpisodeRecord(ro.REPLAY_RING, ring.T, ring.N, 1, 1, ring.A, dev)
    for f in ("u", "r", "term", "padded", "length", "won", "avail"):
        getattr(rec, f).copy_(torch.from_numpy(getattr(ring, f)))
    return rec


def _check_sample(out, want, with_cur, what):
    for f in ("o_map", "u", "u_act", "r", "term", "padded", "length", "won", "avail_next"):
        same(getattr(out, f), getattr(want, f), "%s %s" % (what, f))
    if with_cur:
        same(out.avail_cur, want.avail_cur, what + " avail_cur")


@pytest.mark.parametrize("with_cur", [False, True], ids=["next", "next+cur"])
@pytest.mark.parametrize("T,N,A", ro.REPLAY_SHAPES)
def test_replay_gather(dev, T, N, A, with_cur):
    from marl_amd import ops
    ring, idx = ro.replay_case(T, N, A)
    rec = _ring_on_device(dev, ring)
    B = len(idx)
    # through EpisodeRecord.select_small, then again into the buffers of the first result with other episodes
    out = rec.select_small(cu(idx, dev), avail_cur=with_cur)
    torch.cuda.synchronize()
    assert out.obs is None and out.avail is None and (out.avail_cur is not None) == with_cur
    _check_sample(out, ro.replay_sample(ring, idx), with_cur, "select_small")
    idx2 = (idx[::-1] + 4) % ro.REPLAY_RING
    ptrs = [getattr(out, f).data_ptr() for f in ("u", "avail_next", "o_map")]
    again = rec.select_small(cu(idx2, dev), out=out, avail_cur=with_cur)
    torch.cuda.synchronize()
    assert again is out and ptrs == [getattr(out, f).data_ptr() for f in ("u", "avail_next", "o_map")]
    _check_sample(out, ro.replay_sample(ring, idx2), with_cur, "select_small(out=)")
    # through ops.replay_gather into sentinel-padded buffers
    i32 = torch.int32
    spec = dict(o_map=((B,), i32), u=((B, T, N), i32), u_act=((B, T, N), i32), r=((B, T), None), term=((B, T), None),
                padded=((B, T), None), length=((B,), i32), won=((B,), i32), avail_next=((B, T, N, A), None),
                avail_cur=((B, T, N, A), None))
    whole, o = {}, NS()
    for f, (shape, dt) in spec.items():
        whole[f], v = out_buf(dev, shape, dt or torch.float32)
        setattr(o, f, v)
    if not with_cur:
        o.avail_cur = None
    ops.replay_gather(cu(idx, dev), rec, o)
    torch.cuda.synchronize()
    _check_sample(o, ro.replay_sample(ring, idx), with_cur, "replay_gather")
    for f, (shape, _) in spec.items():
        assert tail_ok(whole[f], int(np.prod(shape))), f
    if not with_cur:
        assert untouched(whole["avail_cur"])
    for f in ("u", "r", "avail", "length"):           # the ring itself is only read
        same(getattr(rec, f), getattr(ring, f), "ring " + f)


# =========================================================================================== selection
@pytest.mark.parametrize("A", [1, 11, 32])
@pytest.mark.parametrize("rows", [1, 255, 256, 257])
def test_q_gather(dev, rows, A):
    from marl_amd import ops
    c = ro.select_case(rows, A, seed=rows + A)
    q, idx, av = cu(c.q_sel, dev), cu(c.idx, dev), cu(c.avail, dev)
    for avail in (None, av):
        whole, out = out_buf(dev, (rows,))
        ops.q_gather(q, idx, out, rows, A, avail=avail, mask_val=ro.MASK_VAL)
        torch.cuda.synchronize()
        same(out, ro.q_gather(c.q_sel, c.idx, None if avail is None else c.avail, ro.MASK_VAL), "q_gather")
        assert tail_ok(whole, rows)


def _masked_max(dev, q, avail, rows, A, want_max=True, want_arg=True):
    from marl_amd import ops
    wm, om = out_buf(dev, (rows,))
    wa, oa = out_buf(dev, (rows,), torch.int32)
    ops.q_masked_max(q, avail, ro.MASK_VAL, om if want_max else None, oa if want_arg else None, rows, A)
    torch.cuda.synchronize()
    assert tail_ok(wm, rows) and tail_ok(wa, rows)
    if not want_max:
        assert untouched(wm)
    if not want_arg:
        assert untouched(wa)
    return om, oa


def test_q_masked_max_row_and_tiled_kernels_agree(dev):
    """4095 rows run one thread per row, 4096 rows the LDS-tiled kernel: the same data, the same results"""
    A = 14
    c = ro.select_case(4096, A)
    q, av = cu(c.q_sel, dev), cu(c.avail, dev)
    mx, arg = ro.q_masked_max(c.q_sel, c.avail, ro.MASK_VAL)
    for rows in (4095, 4096):
        om, oa = _masked_max(dev, q, av, rows, A)
        same(om, mx[:rows], "max %d" % rows)
        same(oa, arg[:rows], "arg %d" % rows)


def test_q_masked_max_second_sweep_and_ragged_last_tile(dev):
    """2048 workgroups x 4 waves x 64 rows = 524 288 rows per sweep of the tiled kernel"""
    rows, A = 524288 + 323, 14
    c = ro.select_case(rows, A)
    om, oa = _masked_max(dev, cu(c.q_sel, dev), cu(c.avail, dev), rows, A)
    mx, arg = ro.q_masked_max(c.q_sel, c.avail, ro.MASK_VAL)
    same(om, mx, "max")
    same(oa, arg, "arg")


@pytest.mark.parametrize("A", [1, 32, 33])
def test_q_masked_max_action_counts(dev, A):
    """A = 32 requests exactly 64 KiB of LDS, A = 33 falls back to one thread per row"""
    rows = 4096 + 70
    c = ro.select_case(rows, A)
    om, oa = _masked_max(dev, cu(c.q_sel, dev), cu(c.avail, dev), rows, A)
    mx, arg = ro.q_masked_max(c.q_sel, c.avail, ro.MASK_VAL)
    same(om, mx, "max")
    same(oa, arg, "arg")


@pytest.mark.parametrize("rows", [300, 4096 + 70])
def test_q_masked_max_optional_arguments(dev, rows):
    A = 11
    c = ro.select_case(rows, A)
    q, av = cu(c.q_sel, dev), cu(c.avail, dev)
    mx, arg = ro.q_masked_max(c.q_sel, c.avail, ro.MASK_VAL)
    om, _ = _masked_max(dev, q, av, rows, A, want_arg=False)
    same(om, mx, "max only")
    _, oa = _masked_max(dev, q, av, rows, A, want_max=False)
    same(oa, arg, "arg only")
    om, oa = _masked_max(dev, q, None, rows, A)                     # no mask
    mx0, arg0 = ro.q_masked_max(c.q_sel, None, ro.MASK_VAL)
    same(om, mx0, "max, no mask")
    same(oa, arg0, "arg, no mask")
    for qs, avs in ((shifted(c.q_sel, dev), av), (q, shifted(c.avail, dev)), (shifted(c.q_sel, dev, 3), None)):
        om, oa = _masked_max(dev, qs, avs, rows, A)                 # an operand 4 (12) bytes off the 16-byte grid
        same(om, mx if avs is not None else mx0, "max, unaligned")
        same(oa, arg if avs is not None else arg0, "arg, unaligned")


def _double_select(dev, qs, qv, av, rows, A, want_arg=True):
    from marl_amd import ops
    wv, ov = out_buf(dev, (rows,))
    wa, oa = out_buf(dev, (rows,), torch.int32)
    ops.q_double_select(qs, qv, av, ro.MASK_VAL, ov, oa if want_arg else None, rows, A)
    torch.cuda.synchronize()
    assert tail_ok(wv, rows) and tail_ok(wa, rows)
    if not want_arg:
        assert untouched(wa)
    return ov, oa


@pytest.mark.parametrize("rows,A", [(1, 11), (63, 11), (64, 11), (65, 11), (524288 + 323, 11), (321, 1), (321, 21), (321, 22),
                                    (321, 30), (321, 32), (4096 + 70, 22)])
def test_q_double_select(dev, rows, A):
    """every action count the agent kernels serve (<= 32): up to 21 the LDS-tiled kernel, from 22 on one thread per row"""
    c = ro.select_case(rows, A)
    qs, qv, av = cu(c.q_sel, dev), cu(c.q_val, dev), cu(c.avail, dev)
    val, arg = ro.q_double_select(c.q_sel, c.q_val, c.avail, ro.MASK_VAL)
    ov, oa = _double_select(dev, qs, qv, av, rows, A)
    same(ov, val, "value")
    same(oa, arg, "arg")
    if rows > 100000:
        return
    ov2, _ = _double_select(dev, qs, qv, av, rows, A, want_arg=False)
    same(ov2, val, "value, out_arg NULL")
    val0, arg0 = ro.q_double_select(c.q_sel, c.q_val, None, ro.MASK_VAL)
    ov0, oa0 = _double_select(dev, qs, qv, None, rows, A)           # avail NULL: everything available
    same(ov0, val0, "value, avail NULL")
    same(oa0, arg0, "arg, avail NULL")
    for k in range(3):                                              # each operand in turn 4 bytes off the 16-byte grid
        ops_ = [qs, qv, av]
        ops_[k] = shifted((c.q_sel, c.q_val, c.avail)[k], dev)
        ovu, oau = _double_select(dev, ops_[0], ops_[1], ops_[2], rows, A)
        assert torch.equal(ovu, ov) and torch.equal(oau, oa), "unaligned operand %d" % k


@pytest.mark.parametrize("gdiv", [1, 5])
@pytest.mark.parametrize("rows", [5, 255, 260])
def test_q_scatter(dev, rows, gdiv):
    from marl_amd import ops
    A = 7
    g = np.random.default_rng(rows + gdiv)
    i1, i2 = g.integers(-1, A, rows).astype(np.int32), g.integers(-1, A, rows).astype(np.int32)
    i1[0], i1[1], i2[2] = 2, -1, -1                                 # (the smallest case has too few rows to leave these to chance)
    i2[::3] = i1[::3]                                               # equal columns: the two values add
    assert ((i1 == i2) & (i1 >= 0)).any() and (i1 < 0).any() and (i2 < 0).any() and rows % gdiv == 0
    g1, g2 = g.standard_normal(rows // gdiv).astype(np.float32), g.standard_normal(rows // gdiv).astype(np.float32)
    for second in (False, True):
        whole, dq = out_buf(dev, (rows, A))
        ops.q_scatter(dq, cu(i1, dev), cu(g1, dev), cu(i2, dev) if second else None, cu(g2, dev) if second else None, rows, A, gdiv)
        torch.cuda.synchronize()
        want = ro.q_scatter(i1, g1, i2 if second else None, g2 if second else None, rows, A, gdiv)
        same(dq, want.astype(np.float32), "dq")                     # at most one addition of two fp32 values: correctly rounded
        assert tail_ok(whole, rows * A)


@pytest.mark.parametrize("N", [1, 10])
@pytest.mark.parametrize("D,ld", [(1, 1), (64, 64), (78, 80)])
def test_agent_sum_and_bcast(dev, D, ld, N):
    from marl_amd import ops
    rows = 333
    g = np.random.default_rng(D + N)
    x = g.standard_normal((rows, N, D)).astype(np.float32)
    xin = torch.full((rows * N, ld), SENT, device=dev)
    xin[:, :D] = cu(x.reshape(rows * N, D), dev)
    whole, o = out_buf(dev, (rows, ld))
    ops.agent_sum(xin[:, :D], o[:, :D], rows, N, D)
    torch.cuda.synchronize()
    s, mag = ro.agent_sum(x)
    if N == 1:
        same(o[:, :D], x[:, 0], "sum of one agent")
    else:
        held("agent_sum D%d N%d" % (D, N), "out", o[:, :D], s, mag, (N - 1) + 2)      # N - 1 additions
    assert tail_ok(whole, rows * ld) and bool((o[:, D:] == SENT).all()), "pad columns written"
    # broadcast of the fp32 sums back over the agents, overwriting and accumulating
    sums = host(o[:, :D]).copy()
    for acc in (0, 1):
        wb, ob = out_buf(dev, (rows * N, ld))
        ob[:, :D] = cu(x.reshape(rows * N, D), dev)
        ops.agent_bcast(o[:, :D], ob[:, :D], rows, N, D, accumulate=bool(acc))
        torch.cuda.synchronize()
        want = np.repeat(sums[:, None, :], N, axis=1)
        if acc:
            want = x + want                                         # one fp32 addition: correctly rounded, as numpy's
        same(ob[:, :D], want.reshape(rows * N, D), "bcast acc=%d" % acc)
        assert tail_ok(wb, rows * N * ld) and bool((ob[:, D:] == SENT).all()), "pad columns written"


def test_agent_sum_and_bcast_refuse_a_short_stride(dev):
    from marl_amd import _lib, ops
    lib, rows, N, D = _lib.load(), 50, 3, 8
    x = torch.ones(rows * N * D, device=dev)
    whole = torch.full((rows * N * D,), SENT, device=dev)
    for ld_in, ld_out in ((D - 1, D), (D, D - 1)):
        assert lib.marl_agent_sum(ops._p(x), ld_in, ops._p(whole), ld_out, rows, N, D, ops._stream()) == INVALID
        assert lib.marl_agent_bcast(ops._p(x), ld_in, ops._p(whole), ld_out, rows, N, D, 0, ops._stream()) == INVALID
    torch.cuda.synchronize()
    assert untouched(whole)


def test_vec_add_second_sweep(dev):
    """4096 workgroups x 256 = 1 048 576 elements per sweep"""
    from marl_amd import ops
    n = 1048576 + 300
    g = np.random.default_rng(1)
    a, b = g.standard_normal(n).astype(np.float32), g.standard_normal(n).astype(np.float32)
    whole, o = out_buf(dev, (n,))
    ops.vec_add(cu(a, dev), cu(b, dev), o, n)
    torch.cuda.synchronize()
    same(o, a + b, "a + b")                                          # one fp32 addition
    assert (ro.vec_add(a, b).astype(np.float32) == a + b).all() and tail_ok(whole, n)


# =========================================================================================== QMIX mixing
SMALL_NE = [(N, E) for N in (1, 5, 10, 16) for E in (16, 32, 64)]
QMIX_CASES = [(R, N, E) for R in (1, 2, 3) for N, E in SMALL_NE] + [(131, 16, 64), (65536, 5, 32), (65536 + 131, 10, 16),
                                                                    (65536 + 131, 1, 64)]


@pytest.mark.parametrize("R,N,E", QMIX_CASES)
def test_qmix_mix_forward_and_backward(dev, R, N, E):
    """8192 workgroups x 4 waves x 2 rows = 65 536 rows per sweep; hy rows at a stride 4 floats wider than their content"""
    from marl_amd import ops
    c = ro.qmix_case(R, N, E, seed=N + E)
    W, ld = c.W, c.W + 4
    hy = torch.full((R, ld), SENT, device=dev)
    hy[:, :W] = cu(c.hy, dev)
    q, b2, w22, b22, g = (cu(x, dev) for x in (c.q, c.b2, c.w22, c.b22, c.dq_tot))
    case = "qmix_mix R%d N%d E%d" % (R, N, E)
    for form in ("b2", "w22"):
        whole, qt = out_buf(dev, (R,))
        if form == "b2":
            ops.qmix_mix_fwd(hy[:, :W], b2, q, qt, R, N, E)
            f = ro.qmix_mix(c.hy, c.q, N, E, b2=c.b2)
        else:
            ops.qmix_mix_fwd(hy[:, :W], None, q, qt, R, N, E, w22=w22, b22=b22)
            f = ro.qmix_mix(c.hy, c.q, N, E, w22=c.w22, b22=c.b22)
        torch.cuda.synchronize()
        held(case, "q_tot (%s)" % form, qt, f.q_tot, f.mag, ro.k_qmix_fwd(N, E))
        assert tail_ok(whole, R)
    for with_w22 in (False, True):
        dhy = torch.full((R + 1, ld), SENT, device=dev)
        wb, db2 = out_buf(dev, (R,))
        wq, dq = out_buf(dev, (R, N))
        ops.qmix_mix_bwd(hy[:, :W], q, g, dhy[:R, :W], db2, dq, R, N, E, w22=w22 if with_w22 else None)
        torch.cuda.synchronize()
        o = ro.qmix_mix_grad(c.hy, c.q, c.dq_tot, N, E, w22=c.w22 if with_w22 else None)
        d = host(dhy)
        held(case, "d w1raw", d[:R, :N * E].reshape(R, N, E), o.d_w1, o.mag_w1, ro.k_qmix_dw1(N))
        held(case, "d b1", d[:R, N * E:N * E + E], o.d_b1, o.mag_b1, ro.k_qmix_dpre(N))
        held(case, "d w2raw", d[:R, N * E + E:N * E + 2 * E], o.d_w2, o.mag_w2, ro.k_qmix_dw2(N))
        held(case, "dq", dq, o.dq, o.mag_q, ro.k_qmix_dq(N, E))
        same(db2, c.dq_tot, "db2")
        if with_w22:
            held(case, "d relu block", d[:R, N * E + 2 * E:W], o.d_hb, o.mag_hb, 1 + 2)        # one product
        else:
            assert (d[:R, N * E + 2 * E:W] == SENT).all(), "the fourth block belongs to the caller"
        assert (d[:R, W:] == SENT).all() and (d[R] == SENT).all() and tail_ok(wb, R) and tail_ok(wq, R * N)
        # planted zeros: exactly zero gradient
        assert (d[:R, :N * E][c.hy[:, :N * E] == 0] == 0).all() and (d[:R, N * E + E:N * E + 2 * E][c.hy[:, N * E + E:N * E + 2 * E] == 0] == 0).all()


def test_qmix_mix_backward_refuses_more_than_16_agents(dev):
    from marl_amd import _lib, ops
    R, N, E = 9, 17, 32
    W = N * E + 3 * E
    hy, q, g = torch.ones(R, W, device=dev), torch.ones(R, N, device=dev), torch.ones(R, device=dev)
    outs = [torch.full((n,), SENT, device=dev) for n in (R * W, R, R * N)]
    code = _lib.load().marl_qmix_mix_bwd(ops._p(hy), W, ops._p(q), ops._p(g), None, ops._p(outs[0]), ops._p(outs[1]), ops._p(outs[2]),
                                         R, N, E, ops._stream())
    torch.cuda.synchronize()
    assert code == INVALID and all(untouched(o) for o in outs)


# =========================================================================================== losses
LOSS_CASES = [(R, "mixed") for R in (1, 255, 256, 257, 262144, 262145)] + [(R, k) for R in (257, 262145) for k in ro.LOSS_KINDS[1:]]


@pytest.mark.parametrize("R,kind", LOSS_CASES)
def test_td_and_qtran_losses(dev, R, kind):
    """1024 workgroups x 256 = 262 144 rows per sweep.  lam_opt = 0.7, lam_nopt = 1.9: swapped lambdas are another function."""
    from marl_amd import ops
    c = ro.loss_case(R, kind, seed=R)
    d = {k: cu(getattr(c, k), dev) for k in ("q_tot", "q_tgt", "r", "term", "padded", "jq", "jq_tgt", "v", "jq_hat", "qs_opt", "qs_nopt")}
    case = "losses R%d %s" % (R, kind)
    wd, dq = out_buf(dev, (R,))
    w2, out2 = out_buf(dev, (2,))
    out2.fill_(3.5)                                                  # overwritten, not accumulated into
    ops.td_loss(d["q_tot"], d["q_tgt"], d["r"], d["term"], d["padded"], ro.GAMMA, dq, out2, R)
    torch.cuda.synchronize()
    o = ro.td_loss(c.q_tot, c.q_tgt, c.r, c.term, c.padded, ro.GAMMA)
    assert tail_ok(wd, R) and tail_ok(w2, 2)
    assert float(out2[1]) == o.out2[1], "sum mask is exact"
    if kind == "all_padded":
        assert bool((dq == 0).all()) and bool((out2 == 0).all())
    else:
        held(case, "td dq_tot", dq, o.dq_tot, o.mag_dq, ro.K_TD)
        held(case, "td sum td^2", out2[:1], o.out2[:1], [o.mag_num], ro.K_TD_NUM)
    outs = [out_buf(dev, (R,)) for _ in range(4)]
    w4, out4 = out_buf(dev, (4,))
    out4.fill_(3.5)
    ops.qtran_loss(d["jq"], d["jq_tgt"], d["v"], d["jq_hat"], d["qs_opt"], d["qs_nopt"], d["r"], d["term"], d["padded"], ro.GAMMA,
                   ro.LAM_OPT, ro.LAM_NOPT, *[v for _, v in outs], out4, R)
    torch.cuda.synchronize()
    o = ro.qtran_loss(c.jq, c.jq_tgt, c.v, c.jq_hat, c.qs_opt, c.qs_nopt, c.r, c.term, c.padded, ro.GAMMA, ro.LAM_OPT, ro.LAM_NOPT)
    assert all(tail_ok(w, R) for w, _ in outs) and tail_ok(w4, 4)
    assert float(out4[3]) == o.out4[3], "sum mask is exact"
    d_jq, d_v, d_so, d_sn = [v for _, v in outs]
    if kind == "all_padded":
        assert all(bool((x == 0).all()) for x in (d_jq, d_v, d_so, d_sn, out4))
        return
    held(case, "qtran d_jq", d_jq, o.d_jq, o.mag_jq, ro.K_QTRAN_G)
    held(case, "qtran d_v", d_v, o.d_v, o.mag_v, ro.K_QTRAN_G + 1)                          # + the addition of the two parts
    held(case, "qtran d_qsum_opt", d_so, o.d_qs_opt, o.mag_qs_opt, ro.K_QTRAN_G)
    held(case, "qtran d_qsum_nopt", d_sn, o.d_qs_nopt, o.mag_qs_nopt, ro.K_QTRAN_G)
    assert bool((d_sn[cu(o.nraw >= 0, dev)] == 0).all()), "the non-optimal term is clamped at 0"
    held(case, "qtran numerators", out4[:3], o.out4[:3], o.mag_num, ro.K_QTRAN_NUM)


# =========================================================================================== optimizer
OPT_N = [1, 255, 256, 257, 65537, 262144, 262145, 1100003]
DENS = [None, 37.0, 9000.0]
REGIMES = list(ro.OPT_REGIMES)
OPT_CASES = ([(n, REGIMES[i % 4], DENS[i % 3]) for i, n in enumerate(OPT_N)] + [(n, REGIMES[(i + 2) % 4], DENS[(i + 1) % 3]) for i, n in enumerate(OPT_N)]
             + [(65537, r, d) for r in REGIMES for d in DENS])
OPT_CASES = sorted(set(OPT_CASES), key=lambda t: (t[0], t[1], t[2] or 0))


def _sumsq_on_device(dev, c, case):
    from marl_amd import ops
    ws, ss = out_buf(dev, (1,))
    ss.fill_(123.0)                                                  # marl_grad_sumsq overwrites its output word
    gd = cu(c.g, dev)
    ops.grad_sumsq(gd, c.n, ss)
    torch.cuda.synchronize()
    ref = ro.sumsq(c.g)
    held(case, "sumsq", ss, [ref], [ref], ro.K_SUMSQ)
    assert tail_ok(ws, 1)
    return gd, ss


@pytest.mark.parametrize("n,regime,den", OPT_CASES)
def test_clip_and_rmsprop_step(dev, n, regime, den):
    """one step from given fp32 state; blocks of 256, at most 1024 of them: n = 262 145 starts the second sweep"""
    from marl_amd import ops
    c = ro.optim_case(n, regime, den, seed=n)
    case = "rmsprop n%d %s den %s" % (n, regime, den)
    gd, ss = _sumsq_on_device(dev, c, case)
    dend = None if den is None else cu(np.array([den], dtype=np.float32), dev)
    wp, p = out_buf(dev, (n,))
    wsq, sq = out_buf(dev, (n,))
    p.copy_(cu(c.p, dev))
    sq.copy_(cu(c.sq, dev))
    ops.rmsprop_step(p, gd, sq, n, ro.LR, ro.ALPHA, ro.EPS, ro.CLIP, ss, dend)
    torch.cuda.synchronize()
    o = ro.rmsprop_step(c.p, c.g, c.sq, ro.LR, ro.ALPHA, ro.EPS, ro.CLIP, den)
    assert (o.coef >= 1) == (regime in ("under", "just_under"))
    held(case, "square_avg", sq, o.sq, o.sq, ro.K_SQ)
    held(case, "p", p, o.p, np.abs(o.p) + ro.K_RMS_DP * o.mag_dp, 1)          # one rounding of p + K u |dp|
    assert tail_ok(wp, n) and tail_ok(wsq, n)
    same(gd, c.g, "the gradient is only read")


@pytest.mark.parametrize("n,regime,den", OPT_CASES)
def test_clip_and_adam_step(dev, n, regime, den):
    from marl_amd import ops
    c = ro.optim_case(n, regime, den, seed=n)
    case = "adam n%d %s den %s" % (n, regime, den)
    gd, ss = _sumsq_on_device(dev, c, case)
    dend = None if den is None else cu(np.array([den], dtype=np.float32), dev)
    for step in (1, 1000):
        bc1, bc2s = ro.bias_corrections(step)
        bufs = [out_buf(dev, (n,)) for _ in range(3)]
        (wp, p), (wm, m), (wv, v) = bufs
        p.copy_(cu(c.p, dev)); m.copy_(cu(c.m, dev)); v.copy_(cu(c.v, dev))
        ops.adam_step(p, gd, m, v, n, ro.LR, ro.BETA1, ro.BETA2, ro.EPS, bc1, bc2s, ro.CLIP, ss, dend)
        torch.cuda.synchronize()
        o = ro.adam_step(c.p, c.g, c.m, c.v, ro.LR, ro.BETA1, ro.BETA2, ro.EPS, bc1, bc2s, ro.CLIP, den)
        held(case, "exp_avg (step %d)" % step, m, o.m, o.mag_m, ro.K_ADAM_M)
        held(case, "exp_avg_sq (step %d)" % step, v, o.v, o.v, ro.K_ADAM_V)
        held(case, "p (step %d)" % step, p, o.p, np.abs(o.p) + ro.K_ADAM_DP * o.mag_dp, 1)
        assert all(tail_ok(w, n) for w, _ in bufs)
