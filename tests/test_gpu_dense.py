"""The dense-layer kernels every learner runs through - marl_linear and marl_linear_wgrad (csrc/gemm.hip) - against the float64
statement of the operation (tests/dense_oracle.py) at every dispatch: the three operand paths, both weight layouts, gate, bf16 and
4 / 5 column tiles of the forward kernel; the generic, full-width, direct (alone and in column passes), tall and thin weight-gradient
kernels at every instantiation, and the slab reduce either side of its 16 slab groups.  Needs a real MI355X: ``pytest -m gpu``.

Every test first ASKS THE LIBRARY which plan it will run (marl_linear_plan / marl_linear_wgrad_plan: the host functions the launches
themselves decide with) and fails with "the plan moved" if that is not the plan its shape was picked for.  Outputs are views into
longer sentinel-filled buffers whose tail and pad columns must be intact; the pad columns of padded inputs hold NaN.
  exact data   == float64 (small integers: any summation order gives the same bits)
  probe data   |got - ref| <= (nnz + 3) u sum |g||x| per element, nnz the nonzero terms of that element; all-zero elements exact
  real data    forward / dX: (terms + 3) u (sum |x||w| + |b| + |beta Y0|); weight gradients: the ceilings of the older tests, with
               the used fraction printed beside fp32 torch-CPU's error against the same float64 reference
Every weight gradient runs twice into fresh buffers: the same bits."""
import numpy as np
import pytest
import torch

import dense_oracle as do
import parity
from test_dense_oracle_cpu import tall_switch, wg_expect, wg_got, wg_plan
from test_gpu_rowwise import SENT, held, host, out_buf, same, tail_ok

pytestmark = pytest.mark.gpu
KINDS = ("exact", "probe", "real")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from marl_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def padded(x, ld, dev, off=0, fill=float("nan"), dtype=torch.float32):
    """x [rows, cols] on the device as the leading columns of a [rows, ld] buffer filled with `fill`, its base `off` floats off the
    16-byte grid; returns the [rows, cols] view"""
    x = np.ascontiguousarray(x)
    rows, cols = x.shape
    whole = torch.full((off + rows * ld + 4,), fill, dtype=dtype, device=dev)
    assert whole.data_ptr() % 16 == 0
    v = whole[off:off + rows * ld].view(rows, ld)
    v[:, :cols] = torch.from_numpy(x).to(dev)
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v[:, :cols]


def dev_src(ops, s, d, dev):
    kw = {}
    x0 = padded(d.store0[:, :s.k0], s.ld0, dev, s.off0) if s.k0 else None
    if s.gate:
        kw["gate"] = padded(d.gate0[:, :s.k0], s.ldm, dev, s.moff)
    if s.k1:
        kw["x1"] = torch.from_numpy(d.x1).to(dev)
    if s.nhot:
        kw.update(idx=torch.from_numpy(d.idx).to(dev), nhot=s.nhot, hot_w=s.hot_w, remapi=s.remapi)
    if s.emap:
        kw["emap0"] = torch.from_numpy(d.emap).to(dev)
    return ops.src(x0, nid=s.nid, remap0=s.remap0, **kw)


# ================================================================================================ marl_linear
def run_linear(ops, dev, c, kind, M=None, N=None, want_plan=None):
    M, N = c.M if M is None else M, c.N if N is None else N
    what = "%s[%s] M%d N%d" % (c.name, kind, M, N)
    i = do.lin_inputs(c, kind, M, N)
    lay = do.lin_layout(c, N)
    x = dev_src(ops, c.src, i.d, dev)
    G = c.groups
    if G > 1:
        flat = np.concatenate([np.concatenate([i.W[g].reshape(-1), i.b[g]]) for g in range(G)])
        fd = torch.from_numpy(flat).to(dev)
        W, b = fd[:N * c.K].view(N, c.K), fd[N * c.K:lay.gs_w]
        grp = ops.group(G, w=lay.gs_w, b=lay.gs_b, y=lay.gs_y)
    else:
        W = padded(i.W[0].T if c.kmajor else i.W[0], lay.ldw, dev, c.woff)
        b = torch.from_numpy(i.b[0]).to(dev) if c.bias else None
        grp = None
    p = ops.linear_plan(x, W, lay.ldw, lay.ldy, M, N, c.K, act=c.act, w_kmajor=c.kmajor, grp=grp, bf16=c.bf16, bias=b)
    if want_plan is None:          # a named case: (path, tiles, gate, k-major, bf16, wvec) and the grid that follows
        want_plan = c.plan + (((M + 127) // 128, (N + 16 * c.plan[1] - 1) // (16 * c.plan[1]), G),)
        got_plan = tuple(p)
    else:                          # the sweep: (path, tiles, grid)
        got_plan = (p.path, p.tiles, p.grid)
    assert got_plan == tuple(want_plan), "the plan moved: %s runs %r" % (what, p)
    whole, Yf = out_buf(dev, (M, lay.ldy))
    cols = G * N
    Yf[:, :cols] = torch.from_numpy(i.Y0).to(dev) if c.beta != 0.0 else float("nan")
    ops.linear(x, W, b, Yf[:, :cols], M, N, c.K, act=c.act, beta=c.beta, w_kmajor=c.kmajor, ldw=lay.ldw, grp=grp, bf16=c.bf16)
    torch.cuda.synchronize()
    assert tail_ok(whole, M * lay.ldy) and bool((Yf[:, cols:] == SENT).all()), what + ": wrote outside Y"
    if kind == "exact":
        same(Yf[:, :cols], i.Y, what)
    else:
        held("dense fwd %s [real]" % c.name, "Y M%d N%d" % (M, N), Yf[:, :cols], i.Y, i.mag, do.k_dot(c.src))


@pytest.mark.parametrize("kind", ("exact", "real"))
@pytest.mark.parametrize("c", do.LIN_CASES, ids=lambda c: c.name)
def test_linear(dev, c, kind):
    from marl_amd import ops
    run_linear(ops, dev, c, kind)


@pytest.mark.parametrize("kind", ("exact", "real"))
@pytest.mark.parametrize("k0", do.LIN_K0)
def test_linear_sweep(dev, k0, kind):
    """M x N of the table at one K0: partial row blocks, partial and clamped column tiles, the 5-tile kernel at 65 .. 80 and the step back
    to 4 tiles in two column blocks at 81, K with and without a tail chunk; act and beta alternate"""
    from marl_amd import ops
    for M in do.LIN_M:
        for N in do.LIN_N:
            c = do.lin("sweep-K%d" % k0, M, N, do.src(k0=k0), act=(M + N) % 2, beta=float(N % 2))
            run_linear(ops, dev, c, kind, want_plan=do.lin_sweep_plan(M, N, k0))


# ================================================================================================ marl_linear_wgrad
def run_wgrad(ops, dev, c, kind):
    what = "%s[%s]" % (c.name, kind)
    lay = do.wg_layout(c)
    G, N, K, M = c.groups, c.N, c.K, c.M
    cols = G * N
    grp = ops.group(G, w=lay.gs_w, b=lay.gs_b, y=lay.gs_y, m0=lay.gs_y) if G > 1 else None
    with tall_switch(c.tall):
        # the plan needs pointers of the right alignment only: ask before the data exists (the probe rows follow its slab count)
        p0 = wg_plan(ops, c)
        assert wg_got(p0) == wg_expect(c), "the plan moved: %s runs %r" % (what, p0)
        i = do.wg_inputs(c, kind, slabs=p0.slabs)
        x = dev_src(ops, c.src, i.d, dev)
        dY = padded(i.dY, lay.ldg, dev, c.goff)
        Ya = padded(i.Yact, lay.ldg, dev) if c.gate else None
        p = ops.linear_wgrad_plan(dY, lay.ldg, x, M, N, K, Yact=Ya, ldya=lay.ldg if c.gate else 0, grp=grp, bf16=c.bf16)
        assert wg_got(p) == wg_expect(c), "the plan moved: %s runs %r" % (what, p)
        runs = []
        for rep in range(2):
            if G > 1:
                whole, flat = out_buf(dev, (G * lay.gs_w,))
                base = np.concatenate([np.concatenate([i.base_w[g].reshape(-1), i.base_b[g]]) for g in range(G)])
                flat.copy_(torch.from_numpy(base).to(dev))
                ops.linear_wgrad(dY, x, flat[:N * K].view(N, K), flat[N * K:lay.gs_w], M, N, K, Yact=Ya, grp=grp, bf16=c.bf16)
                torch.cuda.synchronize()
                assert tail_ok(whole, G * lay.gs_w), what + ": wrote outside the gradients"
                got = host(flat).reshape(G, lay.gs_w)
                runs.append((got[:, :N * K].reshape(G, N, K), got[:, N * K:]))
            else:
                e = c.dw_extra
                whole, Wf = out_buf(dev, (N, lay.lddw))
                Wf[:, e:e + K] = torch.from_numpy(i.base_w[0]).to(dev)
                bwhole, bv = out_buf(dev, (N,))
                bv.copy_(torch.from_numpy(i.base_b[0]).to(dev))
                ops.linear_wgrad(dY, x, Wf[:, e:e + K], bv if c.db else None, M, N, K, Yact=Ya, bf16=c.bf16)
                torch.cuda.synchronize()
                assert tail_ok(whole, N * lay.lddw) and bool((Wf[:, :e] == SENT).all()) and bool((Wf[:, e + K:] == SENT).all()), \
                    what + ": wrote outside its column block of dW"
                assert tail_ok(bwhole, N), what + ": wrote outside db"
                if not c.db:
                    same(bv, i.base_b[0], what + " db (NULL: untouched)")
                runs.append((host(Wf[:, e:e + K]).reshape(1, N, K), host(bv).reshape(1, N)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), what + ": two runs, different bits"
    gW, gb = runs[0]
    assert np.isfinite(gW).all() and np.isfinite(gb).all(), what
    refW, refb = i.base_w.astype(np.float64) + i.dW, i.base_b.astype(np.float64) + (i.db if c.db else 0.0)
    case = "dense wgrad %s [%s]" % (c.name, kind)
    if kind == "exact":
        same(gW, refW, what + " dW")
        same(gb, refb, what + " db")
        return
    for g in range(G):
        sl = slice(g * N, (g + 1) * N)
        Ya_g = None if i.Yact is None else i.Yact[:, sl]
        if kind == "probe":
            mag, nnz, magb, nnzb = do.wgrad_mag(i.Gr[:, sl], Ya_g, i.Xr)
            held(case, "probe dW g%d" % g, gW[g], refW[g], (nnz + 3) * mag, 1.0)
            if c.db:
                held(case, "probe db g%d" % g, gb[g], refb[g], (nnzb + 3) * magb, 1.0)
            continue
        # real data: the ceilings of the older tests; fp32 torch on the CPU against the same float64 reference as the yardstick
        G32 = torch.from_numpy(do.gated(i.Gr[:, sl], Ya_g).astype(np.float32))
        X32 = torch.from_numpy(np.asarray(i.Xr, dtype=np.float32))
        for name, got, ref, cpu in (("dW", gW[g], i.dW[g], (G32.t() @ X32).numpy()), ("db", gb[g], i.db[g], G32.sum(0).numpy())):
            if name == "db" and not c.db:
                continue
            base = (i.base_w if name == "dW" else i.base_b)[g].astype(np.float64)
            ceil = do.wgrad_ceiling(ref, M)
            frac = np.abs(got.astype(np.float64) - (base + ref)) / ceil
            frac_cpu = np.abs(cpu.astype(np.float64) - ref) / ceil
            print("%s / real %s g%d: worst %.4f of the ceiling; fp32 torch-CPU %.4f" % (case, name, g, frac.max(), frac_cpu.max()))
            assert (frac <= 1.0).all(), "%s %s: %.3f of the ceiling at %d" % (what, name, frac.max(), frac.argmax())
            parity.close(case, "real %s g%d (fp32 torch-CPU: %.4f)" % (name, g, frac_cpu.max()), frac, np.zeros_like(frac), tol=1.0, scale=1.0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", do.WG_CASES, ids=lambda c: c.name)
def test_wgrad(dev, c, kind):
    from marl_amd import ops
    run_wgrad(ops, dev, c, kind)
