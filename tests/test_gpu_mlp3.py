"""The fused 64-wide head kernels - the fp32 pair of csrc/mlp3_fused.hip and the bf16 six-product split pair of csrc/mlp3_x6.hip, with
the input tile, weight staging, workgroup map and slab reduce they share (csrc/mlp3_common.h) - against the float64 statement of the
operation (tests/mlp3_oracle.py) at every instantiation the dispatch can select.  Needs a real MI355X: ``pytest -m gpu``.

Every run first ASKS THE LIBRARY which plan it will launch (marl_mlp3_plan: the host functions the launches themselves decide with) and
fails with "the plan moved" if that is not the plan the oracle's restated host arithmetic names for the case.
  exact data   == float64 (small integers below 2^24 in absolute sum: any summation order, and the split, give the same bits)
  probe, real  the oracle's propagated bound, computed from the case's data: outputs |got - ref| <= eY; gradients after two
               accumulating runs |got - (base + 2 ref)| <= 2 E + 4 u (|base| + 2 |ref| + 2 E)
Outputs, gradients, kept activations and the workspace live in sentinel- or NaN-filled buffers: pad columns, the gaps between the
gradient tensors, the rows past M and the guard tails must be intact, a slab a stripe failed to write shows up as NaN, and the pad
columns of the state rows and storage episode 0 hold NaN.  Every run is repeated into fresh buffers: the same bits.  The worst
error / bound ratio of each family is printed (DESIGN.md records them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mlp3_oracle as mo
from test_gpu_dense import dev_src
from test_gpu_rowwise import SENT, host
from test_mlp3_oracle_cpu import same_plan

pytestmark = pytest.mark.gpu
GUARD = 64
RATIOS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from marl_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def ratio_table():
    yield
    for fam in sorted(RATIOS):
        print("mlp3 worst error / bound: %-22s %.3f  (%s)" % ((fam,) + RATIOS[fam]))


# ================================================================================================ buffers
def pack(c, t, fill):
    """the tensors of NS t ([G, ...] each) in the flat layout of mo.w_layout, `fill` in the gaps and in the unused slots of a shared
    layer; returns the float32 array"""
    off, per, gs, sizes = mo.w_layout(c)
    flat = np.full(c.G * per, fill, dtype=np.float32)
    for n, o in off.items():
        v = getattr(t, n)
        for g in range(c.G if gs[n] else 1):
            flat[g * per + o:g * per + o + sizes[n]] = v[g].reshape(-1)
    return flat


def unpack(c, flat, n):
    off, per, gs, sizes = mo.w_layout(c)
    G = c.G if gs[n] else 1
    return np.stack([flat[g * per + off[n]:g * per + off[n] + sizes[n]] for g in range(G)])


def gaps(c, flat):
    off, per, gs, sizes = mo.w_layout(c)
    m = np.ones(flat.shape, bool)
    for n, o in off.items():
        for g in range(c.G if gs[n] else 1):
            m[g * per + o:g * per + o + sizes[n]] = False
    return flat[m]


def w_struct(c, buf, boff=0):
    from marl_amd._lib import MarlMlp3Weights
    off, per, gs, _ = mo.w_layout(c)
    assert buf.data_ptr() % 16 == 0
    w = MarlMlp3Weights()
    for n, o in off.items():
        setattr(w, n, buf.data_ptr() + 4 * (o + (boff if n == "b1" else 0)))
        setattr(w, "gs_" + n, gs[n])
    w._keep = buf
    return w


def laid(c, lay, dev, values=None, fill=SENT):
    """a buffer holding [G, M, N3] `values` in layout `lay` (None: nothing), `fill` everywhere else, GUARD floats of it behind and
    lay.off in front; returns (whole, the tensor mlp3_fwd / mlp3_bwd take, the [G, M, N3] positions in whole)"""
    n = mo.lay_size(c, lay)
    whole = np.full(lay.off + n + GUARD, fill, dtype=np.float32)
    pos = lay.off + mo.lay_index(c, lay)
    if values is not None:
        whole[pos] = values
    wd = torch.from_numpy(whole).to(dev)
    assert wd.data_ptr() % 16 == 0
    return wd, wd[lay.off:lay.off + n], pos


def call_fwd(ops, w, x, Yv, lay, c, hs, x6, hs_floats=None):
    from marl_amd import _lib
    lib = _lib.load()
    fn = lib.marl_mlp3_x6_fwd_save if x6 else lib.marl_mlp3_fwd_save
    hp, hn = (C.c_void_p(hs.data_ptr()), hs.numel() if hs_floats is None else hs_floats) if hs is not None else (None, 0)
    return fn(C.byref(w), C.byref(x), C.c_void_p(Yv.data_ptr()), lay.ld, lay.gs, hp, hn, c.M, c.K1, c.N3, c.G,
              C.c_void_p(torch.cuda.current_stream().cuda_stream))


def workspace(ops, c, dev):
    """the entry of the shared grow-only workspace that ops.mlp3_bwd uses, NaN-filled"""
    from marl_amd import _lib
    ws = ops.WS.get("mlp3", _lib.load().marl_mlp3_bwd_workspace(c.M, c.K1, c.N3, c.G), dev)
    ws.fill_(float("nan"))
    return ws


def call_bwd(ops, w, x, dYv, lay, gw, c, hs, x6, dev, ws_bytes=None, hs_floats=None):
    from marl_amd import _lib
    lib = _lib.load()
    ws = workspace(ops, c, dev)
    fn = lib.marl_mlp3_x6_bwd_saved if x6 else lib.marl_mlp3_bwd_saved
    hp, hn = (C.c_void_p(hs.data_ptr()), hs.numel() if hs_floats is None else hs_floats) if hs is not None else (None, 0)
    return fn(C.byref(w), C.byref(x), C.c_void_p(dYv.data_ptr()), lay.ld, lay.gs, C.byref(gw), C.c_void_p(ws.data_ptr()),
              ws.numel() * 4 if ws_bytes is None else ws_bytes, hp, hn, c.M, c.K1, c.N3, c.G,
              C.c_void_p(torch.cuda.current_stream().cuda_stream))


def hsave_buf(ops, c, dev):
    need = ops.mlp3_save_floats(c.M, c.nl == 3, c.G)
    whole = torch.full((need + GUARD,), float("nan"), device=dev)
    whole[need:] = SENT
    return whole, whole[:need]


def note(fam, name, ratio):
    if ratio > RATIOS.get(fam, (-1.0, ""))[0]:
        RATIOS[fam] = (float(ratio), name)


def check(what, fam, got, ref, tol, exact):
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s: not finite" % what
    if exact:
        bad = np.flatnonzero(got.reshape(-1) != ref.reshape(-1))
        assert bad.size == 0, "%s: %d of %d differ, first at %d: got %r want %r" % (
            what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], ref.reshape(-1)[bad[0]])
        return
    err = np.abs(got - ref)
    z = tol == 0
    assert (err[z] == 0).all(), "%s: non-zero where the bound is 0" % what
    r = np.zeros_like(err)
    r[~z] = err[~z] / tol[~z]
    worst = float(r.max()) if r.size else 0.0
    note(fam, what, worst)
    assert worst <= 1.0, "%s: %.3f of the oracle's bound at %d (error %.3g)" % (what, worst, r.argmax(), err.reshape(-1)[r.argmax()])


# ================================================================================================ one case
def planned(ops, c, call, kept, w, x, Yv, lay, gw, hs):
    p = ops.mlp3_plan(call, w, x, c.M, c.K1, c.N3, c.G, Y=Yv, ld=lay.ld, gs=lay.gs, grads=gw, hsave=hs if kept else None)
    want = mo.expected_plan(c, call, kept, lay)
    assert same_plan(p, want), "the plan moved: %s %s kept=%d runs %r, named for %r" % (c.name, call, kept, p, want)
    for f, v in c.want.get((call, kept), {}).items():
        assert getattr(p, f) == v, "the plan moved: %s %s kept=%d: %s = %r" % (c.name, call, kept, f, getattr(p, f))
    return p


def run_pair(ops, dev, c, kind, x6, state):
    """forward (kept and not), backward (kept and, where it exists, recomputing) of one pair; returns the bits for the repeat"""
    i = mo.inputs(c, kind)
    exact = kind == "exact"
    pair = "x6" if x6 else "fp32"
    what = "%s[%s] %s" % (c.name, kind, pair)
    x, w = state.x, state.w
    lay, dlay = mo.y_layout(c), mo.dy_layout(c)
    fams = "%s %s" % (pair, "wide" if c.N3 > 16 else "%d-layer" % c.nl)
    bits = []
    # ---- forward, keeping the activations
    hs_whole, hs = hsave_buf(ops, c, dev)
    Yw, Yv, pos = laid(c, lay, dev)
    planned(ops, c, "x6_fwd" if x6 else "fwd", True, w, x, Yv, lay, state.gw0, hs)
    assert call_fwd(ops, w, x, Yv, lay, c, hs, x6) == 0, what
    got = host(Yw)
    out = np.ones(got.shape, bool)
    out[pos] = False
    assert (got[out] == SENT).all(), what + ": the forward wrote outside the heads' columns / past row M"
    eY = np.stack([f.eY for f in (i.fx if x6 else i.f)])
    check(what + " Y", fams + " Y", got[pos], i.Y, eY, exact)
    hsg = host(hs_whole)
    assert (hsg[hs.numel():] == SENT).all(), what + ": wrote past marl_mlp3_save_floats"
    bits.append(got)
    # ---- forward without keeping: the same bits
    needs_kept = mo.needs_kept(c)
    Yw2, Yv2, _ = laid(c, lay, dev)
    planned(ops, c, "x6_fwd" if x6 else "fwd", False, w, x, Yv2, lay, state.gw0, None)
    assert call_fwd(ops, w, x, Yv2, lay, c, None, x6) == 0, what
    assert torch.equal(Yw2, Yw), what + ": outputs with and without hsave differ"
    # ---- backward: twice into nonzero base contents
    dYw, dYv, _ = laid(c, dlay, dev, i.dY, fill=float("nan"))
    base = pack(c, i.base, SENT)
    kept_grads = None
    for kept in ((True,) if (x6 or needs_kept) else (True, False)):
        gd = torch.from_numpy(base).to(dev)
        gw = w_struct(c, gd)
        p = planned(ops, c, "x6_bwd" if x6 else "bwd", kept, w, x, dYv, dlay, gw, hs)
        for rep in range(2):
            assert call_bwd(ops, w, x, dYv, dlay, gw, c, hs if kept else None, x6, dev) == 0, what
        gg = host(gd)
        assert (gaps(c, gg) == SENT).all(), what + ": the backward wrote between the gradient tensors"
        ref = mo.grads(c, i, x6, p.slabs)
        for n in (mo.W_NAMES if c.nl == 3 else ("w1", "b1", "w3", "b3")):
            b = unpack(c, base, n).astype(np.float64)
            r = np.stack([ref[g][n][0] for g in range(b.shape[0])]).reshape(b.shape)
            E = np.stack([ref[g][n][1] for g in range(b.shape[0])]).reshape(b.shape)
            tol = 2 * E + 4 * mo.U * (np.abs(b) + 2 * np.abs(r) + 2 * E)
            check("%s d%s %s" % (what, n, "kept" if kept else "recomputed"), "%s d%s" % (fams, n), unpack(c, gg, n), b + 2 * r, tol, exact)
        if exact and kept_grads is not None:
            assert np.array_equal(gg, kept_grads), what + ": kept and recomputed gradients differ on exact data"
        kept_grads = gg if kept else kept_grads
        bits.append(gg)
    if needs_kept and not x6:          # recompute requested where only the kept backward exists: an error, nothing written
        gd = torch.from_numpy(base).to(dev)
        assert planned(ops, c, "bwd", False, w, x, dYv, dlay, w_struct(c, gd), None) is None
        assert call_bwd(ops, w, x, dYv, dlay, w_struct(c, gd), c, None, False, dev) != 0
        torch.cuda.synchronize()
        assert np.array_equal(host(gd), base, equal_nan=True) and bool(torch.isnan(ops.WS.bufs["mlp3"]).all())
    return bits


def run_case(ops, dev, c, kind):
    i = mo.inputs(c, kind)
    state = mo.NS(x=dev_src(ops, c.src, i.d, dev))
    wd = torch.from_numpy(pack(c, i.w, float("nan"))).to(dev)
    state.w = w_struct(c, wd)
    state.gw0 = w_struct(c, torch.from_numpy(pack(c, i.base, SENT)).to(dev))
    for x6 in ((False, True) if c.x6 else (False,)):
        first = run_pair(ops, dev, c, kind, x6, state)
        again = run_pair(ops, dev, c, kind, x6, state)
        for a, b in zip(first, again):
            assert np.array_equal(a, b), "%s[%s] x6=%d: two runs differ" % (c.name, kind, x6)


CASE_KINDS = [(c, k) for c in mo.CASES for k in c.kinds]


@pytest.mark.parametrize("c,kind", CASE_KINDS, ids=lambda v: v if isinstance(v, str) else v.name)
def test_case(dev, c, kind):
    from marl_amd import ops
    run_case(ops, dev, c, kind)


# ================================================================================================ refusals
@pytest.mark.parametrize("name", ["rows65", "wide32"])
def test_refusals_write_nothing(dev, name):
    """short hsave, short workspace, unaligned b1, a WIDE dY off the 16-byte grid: an error code, and outputs, gradients and workspace
    keep their contents"""
    from marl_amd import ops
    c = mo.BY_NAME[name]
    i = mo.inputs(c, "exact")
    x = dev_src(ops, c.src, i.d, dev)
    wd = torch.from_numpy(pack(c, i.w, float("nan"))).to(dev)
    w, w_bad = w_struct(c, wd), w_struct(c, wd, boff=1)
    lay = mo.y_layout(c)
    base = pack(c, i.base, SENT)
    dYw, dYv, _ = laid(c, lay, dev, i.dY, fill=0.0)
    from marl_amd import _lib
    ws_need = _lib.load().marl_mlp3_bwd_workspace(c.M, c.K1, c.N3, c.G)
    for x6 in ((False, True) if c.x6 else (False,)):
        Yw, Yv, _ = laid(c, lay, dev)
        hs_whole, hs = hsave_buf(ops, c, dev)
        assert call_fwd(ops, w, x, Yv, lay, c, hs, x6, hs_floats=hs.numel() - 1) != 0          # short hsave
        assert call_fwd(ops, w_bad, x, Yv, lay, c, hs, x6) != 0                                 # b1 off the 16-byte grid
        torch.cuda.synchronize()
        assert bool((Yw == SENT).all()) and bool(torch.isnan(hs).all())
        assert call_fwd(ops, w, x, Yv, lay, c, hs, x6) == 0
        gd = torch.from_numpy(base).to(dev)
        gw = w_struct(c, gd)
        bad = [call_bwd(ops, w, x, dYv, lay, gw, c, hs, x6, dev, hs_floats=hs.numel() - 1),
               call_bwd(ops, w, x, dYv, lay, gw, c, hs, x6, dev, ws_bytes=ws_need - 4)]
        if not x6:
            bad.append(call_bwd(ops, w_bad, x, dYv, lay, gw, c, hs, x6, dev))
        if c.N3 > 16:
            off = mo.NS(ld=lay.ld, gs=lay.gs, off=1)
            dYw1, dYv1, _ = laid(c, off, dev, i.dY, fill=0.0)
            assert ops.mlp3_plan("bwd", w, x, c.M, c.K1, c.N3, c.G, Y=dYv1, ld=off.ld, gs=off.gs, grads=gw, hsave=hs) is None
            bad.append(call_bwd(ops, w, x, dYv1, off, gw, c, hs, x6, dev))
        torch.cuda.synchronize()
        assert all(e != 0 for e in bad), bad
        assert np.array_equal(host(gd), base) and bool(torch.isnan(ops.WS.bufs["mlp3"]).all())
        assert call_bwd(ops, w, x, dYv, lay, gw, c, hs, x6, dev) == 0
        torch.cuda.synchronize()
        assert not np.array_equal(host(gd), base)


def test_refused_shapes_launch_nothing(dev):
    from marl_amd import ops
    for c in mo.REFUSED:
        d = mo.make_src(c.src, c.M, np.random.default_rng(1), "exact")
        x = dev_src(ops, c.src, d, dev)
        z = mo.NS(**{n: np.zeros((c.G,) + s, np.float32) for n, s in (("w1", (64, c.K1)), ("b1", (64,)), ("w2", (64, 64)), ("b2", (64,)),
                                                                        ("w3", (c.N3, 64)), ("b3", (c.N3,)))})
        w = w_struct(c, torch.from_numpy(pack(c, z, 0.0)).to(dev))
        lay = mo.NS(ld=c.G * c.N3, gs=c.N3, off=0)
        Yw, Yv, _ = laid(c, lay, dev)
        hs_whole, hs = hsave_buf(ops, c, dev)
        for x6 in (False, True):
            assert call_fwd(ops, w, x, Yv, lay, c, hs, x6) != 0, c.name
        torch.cuda.synchronize()
        assert bool((Yw == SENT).all()) and bool(torch.isnan(hs).all()), c.name


# ================================================================================================ module wiring (network/mixer.py)
class HeadSpy:
    """records every ops.mlp3_fwd / ops.mlp3_bwd call a mixer makes (arguments, the plan of the call, dY's values)"""

    def __init__(self, monkeypatch, ops):
        self.fwd, self.bwd = [], []
        f0, b0 = ops.mlp3_fwd, ops.mlp3_bwd

        def fwd(w, x, Y, M, K1, N3, groups, hsave=None, x6=False):
            ld, gs = ops._head_layout(Y, M, N3, groups)
            p = ops.mlp3_plan("x6_fwd" if x6 else "fwd", w, x, M, K1, N3, groups, Y=Y, ld=ld, gs=gs, hsave=hsave)
            f0(w, x, Y, M, K1, N3, groups, hsave=hsave, x6=x6)
            self.fwd.append(mo.NS(Y=Y, M=M, K1=K1, N3=N3, G=groups, kept=hsave is not None, x6=x6, plan=p))

        def bwd(w, x, dY, grads, M, K1, N3, groups, hsave=None, x6=False):
            ld, gs = ops._head_layout(dY, M, N3, groups)
            p = ops.mlp3_plan("x6_bwd" if x6 else "bwd", w, x, M, K1, N3, groups, Y=dY, ld=ld, gs=gs, grads=grads, hsave=hsave)
            self.bwd.append(mo.NS(dY=dY.clone(), M=M, K1=K1, N3=N3, G=groups, kept=hsave is not None, x6=x6, plan=p))
            b0(w, x, dY, grads, M, K1, N3, groups, hsave=hsave, x6=x6)

        monkeypatch.setattr(ops, "mlp3_fwd", fwd)
        monkeypatch.setattr(ops, "mlp3_bwd", bwd)


def _set_head_params(stacks, rng):
    """the oracle's real-data scales on the nn.Linear layers of head stacks"""
    for lins in stacks:
        for li, l in enumerate(lins):
            last = li == len(lins) - 1
            sw = 0.2 if last else (0.5 / l.in_features ** 0.5 if li == 0 else 0.03)
            with torch.no_grad():
                l.weight.copy_(torch.from_numpy(rng.standard_normal(tuple(l.weight.shape)) * sw))
                l.bias.copy_(torch.from_numpy(rng.standard_normal(tuple(l.bias.shape)) * (1.0 if last else 4.0)))


def _family_case(name, rows, stacks, S, NH, HW, x6, shared_groups=0):
    """(pseudo case of the oracle, float64 weights) for the heads `stacks` (lists of nn.Linear) over [state | NH one-hot blocks];
    shared_groups: ONE Linear-ReLU-Linear stack evaluated as that many column blocks sharing layer 1"""
    nl = len(stacks[0])
    G = shared_groups or len(stacks)
    N3 = stacks[0][-1].out_features // (shared_groups or 1)
    c = mo.case(name, rows, G, N3, nl, mo.src(k0=S, nhot=NH, hot_w=HW), shared=bool(shared_groups))
    c.x6 = x6
    g64 = lambda t: t.detach().double().cpu().numpy()
    w = mo.NS(w2=None, b2=None)
    w.w1, w.b1 = np.stack([g64(s[0].weight) for s in stacks]), np.stack([g64(s[0].bias) for s in stacks])
    if nl == 3:
        w.w2, w.b2 = np.stack([g64(s[1].weight) for s in stacks]), np.stack([g64(s[1].bias) for s in stacks])
    if shared_groups:
        w.w3, w.b3 = g64(stacks[0][-1].weight).reshape(G, N3, 64), g64(stacks[0][-1].bias).reshape(G, N3)
    else:
        w.w3, w.b3 = np.stack([g64(s[-1].weight) for s in stacks]), np.stack([g64(s[-1].bias) for s in stacks])
    return c, w


def _to_gmn(t, G, M, N3):
    t = host(t).astype(np.float64)
    return t if t.ndim == 3 else t.reshape(M, G, N3).transpose(1, 0, 2)


def _check_family(what, c, w, X, rec_f, rec_b, stacks):
    """one recorded forward / backward pair of a mixer against the oracle: outputs, then the parameter gradients the module holds"""
    k = mo.k_x6 if rec_f.x6 else mo.k_fp32
    f = mo.forward(c, X, w, k)
    assert not np.stack([h.kink for h in f]).any(), what + ": the states were to be free of kink rows"
    check(what + " Y", "wiring", _to_gmn(rec_f.Y, c.G, c.M, c.N3), np.stack([h.Y for h in f]), np.stack([h.eY for h in f]), False)
    dY = _to_gmn(rec_b.dY, c.G, c.M, c.N3)
    ref = mo.backward(c, X, w, f, dY, k, rec_b.plan.slabs)
    names = ("w1", "b1", "w2", "b2", "w3", "b3") if c.nl == 3 else ("w1", "b1", "w3", "b3")
    for g, lins in enumerate(stacks):
        params = [p for l in lins for p in (l.weight, l.bias)]
        for n, p in zip(names, params):
            got = host(p.grad).astype(np.float64)
            if c.shared and n in ("w3", "b3"):
                r = np.concatenate([ref[j][n][0] for j in range(c.G)]).reshape(got.shape)
                E = np.concatenate([ref[j][n][1] for j in range(c.G)]).reshape(got.shape)
            else:
                r, E = ref[g][n][0].reshape(got.shape), ref[g][n][1].reshape(got.shape)
            check("%s head %d d%s" % (what, g, n), "wiring", got, r, E + 4 * mo.U * (np.abs(r) + E), False)


def _kink_free(rows, S, N, A, families, rng):
    """states (and actions) whose rows lie on no relu kink of any family, by the oracle's bound: rows on one are drawn again"""
    s = rng.standard_normal((rows, S)).astype(np.float32)
    u = rng.integers(0, A, size=(rows, N)).astype(np.int32)
    for _ in range(60):
        oh = np.zeros((rows, N, A))
        oh[np.arange(rows)[:, None], np.arange(N)[None], u] = 1.0
        bad = np.zeros(rows, bool)
        for c, w, with_u in families:
            X = np.concatenate([s.astype(np.float64), oh.reshape(rows, -1)], 1) if with_u else s.astype(np.float64)
            for kf in ((mo.k_fp32, mo.k_x6) if c.x6 else (mo.k_fp32,)):
                bad |= np.stack([h.kink for h in mo.forward(c, X, w, kf)]).any(0)
        if not bad.any():
            return s, u, oh
        s[bad] = rng.standard_normal((int(bad.sum()), S)).astype(np.float32)
        u[bad] = rng.integers(0, A, size=(int(bad.sum()), N))
    raise AssertionError("no kink-free states found")


@pytest.mark.parametrize("keep,mode", [(1, "f32"), (0, "f32"), (1, "bf16x6")])
@pytest.mark.parametrize("mapname", ["2s3z", "MMM2"])
def test_qplex_heads_through_the_mixer(dev, monkeypatch, mapname, keep, mode):
    """DMAQer.hip_forward / hip_backward (network/mixer.py): the transformation nets (one two-head launch) and the key / agents / action
    extractor families run the fused pairs the switches select - kept or recomputing, fp32 or split; the K1 > 192 families of an
    MMM2-sized map only with kept activations, else the marl_linear composition - and every such launch agrees with float64
    nn.Linear / ReLU stacks of the module's own parameters: outputs, and the gradients left in the parameters' .grad"""
    from marl_amd import experiments, ops
    from marl_amd.hostutil import FlatParams
    from marl_amd.network.mixer import DMAQer, _linears
    from oracle import seeded
    args = seeded.make_args(mapname, "qplex")
    args.gemm_mode = mode
    N, A, S, K = args.n_agents, args.n_actions, int(np.prod(args.state_shape)), args.num_kernel
    rows = 130
    torch.manual_seed(3)
    mod = DMAQer(args)
    rng = np.random.default_rng(mo.case_seed(mapname))
    fams = [(name, [_linears(m) for m in mods], nout) for name, mods, nout in mod.si_weight.families()]
    trans = [_linears(mod.hyper_w_final), _linears(mod.V)]
    _set_head_params([st for _, stacks, _ in fams for st in stacks] + trans, rng)
    mod.to(dev)
    fp = FlatParams(list(mod.parameters()), dev, with_grad=True)
    x6 = mode == "bf16x6" and keep == 1
    three = len(fams[0][1][0]) == 3
    cases = [("wv",) + _family_case("wv-" + mapname, rows, trans, S, 0, 0, False) + (False, trans)]
    for name, stacks, nout in fams:
        NH = N if name == "ac" else 0
        c, w = _family_case(name + "-" + mapname, rows, stacks, S, NH, A if NH else 0, False)
        c.x6 = x6 and three and mo.x6_supported(c)
        cases.append((name, c, w, name == "ac", stacks))
    s, u, oh = _kink_free(rows, S, N, A, [(c, w, wu) for _, c, w, wu, _ in cases], rng)
    store = torch.full((rows, (S + 3) // 4 * 4), float("nan"), device=dev)
    store[:, :S] = torch.from_numpy(s).to(dev)
    sd = store[:, :S]
    q, max_q = (torch.from_numpy(rng.standard_normal((rows, N)).astype(np.float32)).to(dev) for _ in range(2))
    g = torch.from_numpy(rng.standard_normal(rows).astype(np.float32)).to(dev)
    spy = HeadSpy(monkeypatch, ops)
    with experiments.override(mlp3_keep=keep):
        ctx = {}
        mod.hip_forward(q, sd, rows, u_idx=torch.from_numpy(u.reshape(-1)).to(dev), max_q=max_q, ctx=ctx)
        mod.hip_backward(ctx, g, rows)
    torch.cuda.synchronize()
    fused = [(n_, c, w, wu, st) for n_, c, w, wu, st in cases if mo.supported(c) and (keep or not mo.needs_kept(c)) and c.nl in (2, 3)]
    assert len(spy.fwd) == len(spy.bwd) == len(fused), "%d fused forwards, %d backwards; %d families qualify" % (
        len(spy.fwd), len(spy.bwd), len(fused))
    assert len(fused) == len(cases) or (mapname == "MMM2" and keep == 0)
    for (n_, c, w, wu, st), rf in zip(fused, spy.fwd):
        rb = [b for b in spy.bwd if (b.K1, b.N3, b.G) == (rf.K1, rf.N3, rf.G)]
        rb = rb[0] if n_ != "ac" or len(rb) == 1 else rb[-1]
        assert (rf.K1, rf.N3, rf.G) == (c.K1, c.N3, c.G), n_
        assert rf.kept == rb.kept == bool(keep) and rf.x6 == rb.x6 == c.x6, (n_, rf.kept, rf.x6)
        for call, r in ((("x6_" if c.x6 else "") + "fwd", rf), (("x6_" if c.x6 else "") + "bwd", rb)):
            lay = mo.NS(ld=c.N3, gs=rows * c.N3, off=0) if n_ == "wv" else mo.NS(ld=c.G * c.N3, gs=c.N3, off=0)
            assert same_plan(r.plan, mo.expected_plan(c, call, bool(keep), lay)), "the plan moved: %s %s runs %r" % (n_, call, r.plan)
        X = np.concatenate([s.astype(np.float64), oh.reshape(rows, -1)], 1) if wu else s.astype(np.float64)
        _check_family("qplex %s %s keep=%d %s" % (mapname, n_, keep, mode), c, w, X, rf, rb, st)
    assert not torch.isnan(fp.grad).any()


@pytest.mark.parametrize("keep", [1, 0])
@pytest.mark.parametrize("N,S", [(5, 120), (10, 322)])
def test_qmix_two_hyper_wide_heads_through_the_mixer(dev, monkeypatch, N, S, keep):
    """QMixMixer(two_hyper_layers).hip_forward / hip_backward: hyper_w1 (N x 32 outputs: one group of 160, or two column blocks of 160
    that share layer 1) and hyper_w2 (32 outputs) run the WIDE kept pair - with mlp3_keep = 0 the marl_linear composition - and agree
    with float64 stacks of the module's parameters"""
    import types
    from marl_amd import experiments, ops
    from marl_amd.hostutil import FlatParams
    from marl_amd.network.mixer import QMixMixer, _linears
    args = types.SimpleNamespace(n_agents=N, state_shape=S, qmix_hidden_dim=32, hyper_hidden_dim=64, two_hyper_layers=True)
    rows = 130
    torch.manual_seed(5)
    mod = QMixMixer(args)
    rng = np.random.default_rng(N + S)
    heads = [("w1", _linears(mod.hyper_w1), (N * 32 + 159) // 160), ("w2", _linears(mod.hyper_w2), 1)]
    _set_head_params([st for _, st, _ in heads], rng)
    mod.to(dev)
    fp = FlatParams(list(mod.parameters()), dev, with_grad=True)
    cases = [(n_,) + _family_case("qmix-%s-%d" % (n_, S), rows, [st], S, 0, 0, False, shared_groups=G) + (False, [st]) for n_, st, G in heads]
    s, u, oh = _kink_free(rows, S, 1, 1, [(c, w, False) for _, c, w, _, _ in cases], rng)
    store = torch.full((rows, (S + 3) // 4 * 4), float("nan"), device=dev)
    store[:, :S] = torch.from_numpy(s).to(dev)
    q = torch.from_numpy(rng.standard_normal((rows, N)).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.standard_normal(rows).astype(np.float32)).to(dev)
    spy = HeadSpy(monkeypatch, ops)
    with experiments.override(mlp3_keep=keep):
        ctx = {}
        mod.hip_forward(q, store[:, :S], rows, ctx=ctx)
        mod.hip_backward(ctx, g, rows)
    torch.cuda.synchronize()
    assert len(spy.fwd) == len(spy.bwd) == (2 if keep else 0)
    for (n_, c, w, _, st), rf in zip(cases if keep else [], spy.fwd):
        rb = [b for b in spy.bwd if (b.N3, b.G) == (rf.N3, rf.G)][0]
        assert (rf.K1, rf.N3, rf.G, rf.kept, rb.kept) == (S, c.N3, c.G, True, True) and rf.plan.wide and rb.plan.wide
        assert (c.G, c.N3) == ((1, 160) if N == 5 else (2, 160)) if n_ == "w1" else (c.G, c.N3) == (1, 32)
        _check_family("qmix two_hyper %s S=%d" % (n_, S), c, w, s.astype(np.float64), rf, rb, st)
    assert not torch.isnan(fp.grad).any()
