"""tests/mlp3_oracle.py on the CPU: its float64 operation is held to torch float64 autograd of the plain nn.Linear / ReLU stacks, its
restated host arithmetic and its case table to the library's own plan query (marl_mlp3_plan: the host functions the four launches
themselves decide with - no GPU, pointer VALUES of the right alignment stand for device memory), its exact cases to the 2^24 limit and
the 8-bit condition of the split, its probe and real cases to the kink cap."""
import os

import numpy as np
import pytest
import torch

import dense_oracle as do
import mlp3_oracle as mo
from test_dense_oracle_cpu import fab_src

BASE = {"W": 16 << 20, "G": 32 << 20, "Y": 48 << 20, "H": 64 << 20}
COMBOS = (("fwd", True), ("fwd", False), ("bwd", False), ("bwd", True), ("x6_fwd", True), ("x6_fwd", False), ("x6_bwd", True),
          ("x6_bwd", False))
PLAN_FIELDS = "KC CF CFT kpad KV three wide n3t kept KH passes wgpc nst per grid lds yvec slabs".split()


@pytest.fixture(scope="module")
def ops():
    from marl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    from marl_amd import ops
    return ops


def fab_weights(c, base, boff=0):
    """a MarlMlp3Weights over a flat buffer at address `base` laid out by mo.w_layout; boff: b1 that many floats off the 16-byte grid"""
    from marl_amd._lib import MarlMlp3Weights
    off, per, gs, _ = mo.w_layout(c)
    w = MarlMlp3Weights()
    for n, o in off.items():
        setattr(w, n, base + 4 * (o + (boff if n == "b1" else 0)))
        setattr(w, "gs_" + n, gs[n])
    return w


def plan_of(ops, c, call, kept, lay=None, **kw):
    """ops.mlp3_plan for a case with fabricated addresses (hsave given when `kept`)"""
    lay = lay or (mo.dy_layout(c) if call.endswith("bwd") else mo.y_layout(c))
    args = dict(Y=BASE["Y"] + 4 * lay.off, ld=lay.ld, gs=lay.gs, grads=fab_weights(c, BASE["G"]), hsave=BASE["H"] if kept else None)
    args.update(kw)
    return ops.mlp3_plan(call, fab_weights(c, BASE["W"]), fab_src(c.src), c.M, c.K1, c.N3, c.G, **args)


def same_plan(got, want):
    if got is None or want is None:
        return got is None and want is None
    return all(getattr(got, f) == getattr(want, f) for f in PLAN_FIELDS)


# ================================================================================================ the operation
def _torch_heads(c, i):
    heads = []
    for g in range(c.G):
        g1 = 0 if c.shared else g
        ps = [i.w.w1[g1], i.w.b1[g1]] + ([i.w.w2[g], i.w.b2[g]] if c.nl == 3 else []) + [i.w.w3[g], i.w.b3[g]]
        heads.append([torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in ps])
    return heads


@pytest.mark.parametrize("name", ["seg-remap", "seg-remap-l2", "kv193-l3", "wide36-kc16", "n3=15-l3", "rows65"])
@pytest.mark.parametrize("kind", mo.KINDS)
def test_oracle_against_torch_float64(name, kind):
    """forward and all gradients of the oracle == torch float64 autograd of Linear-ReLU-(Linear-ReLU-)Linear on the virtual rows"""
    c = mo.BY_NAME[name]
    i = mo.inputs(c, kind)
    X = torch.tensor(i.X)
    gr = mo.grads(c, i, False, 1)
    for g, ps in enumerate(_torch_heads(c, i)):
        h = torch.relu(torch.nn.functional.linear(X, ps[0], ps[1]))
        if c.nl == 3:
            h = torch.relu(torch.nn.functional.linear(h, ps[2], ps[3]))
        y = torch.nn.functional.linear(h, ps[-2], ps[-1])
        np.testing.assert_allclose(i.Y[g], y.detach().numpy(), rtol=1e-12, atol=1e-12)
        y.backward(torch.tensor(i.dY[g], dtype=torch.float64))
        names = mo.W_NAMES if c.nl == 3 else ("w1", "b1", "w3", "b3")
        for n, p in zip(names, ps):
            np.testing.assert_allclose(gr[g][n][0], p.grad.numpy(), rtol=1e-11, atol=1e-11, err_msg="%s head %d d%s" % (name, g, n))
            assert (gr[g][n][1] >= 0).all() and np.isfinite(gr[g][n][1]).all()


@pytest.mark.parametrize("name", ["shared-G2", "shared-G3", "shared-G3-narrow"])
def test_shared_layer_is_one_unsplit_head(name):
    """the column blocks of a shared-layer case are ONE head Linear(K1, 64) - ReLU - Linear(64, G N3): same outputs, and the layer-1
    gradients the oracle sums over the groups are that head's"""
    c = mo.BY_NAME[name]
    i = mo.inputs(c, "real")
    X = torch.tensor(i.X)
    w1, b1 = (torch.tensor(v[0], dtype=torch.float64, requires_grad=True) for v in (i.w.w1, i.w.b1))
    w3 = torch.tensor(i.w.w3.reshape(c.G * c.N3, 64), dtype=torch.float64, requires_grad=True)
    b3 = torch.tensor(i.w.b3.reshape(-1), dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(X, w1, b1)), w3, b3)
    np.testing.assert_allclose(np.concatenate(list(i.Y), 1), y.detach().numpy(), rtol=1e-12, atol=1e-12)
    y.backward(torch.tensor(np.concatenate(list(i.dY), 1), dtype=torch.float64))
    gr = mo.grads(c, i, False, 1)
    for g in range(c.G):
        np.testing.assert_allclose(gr[g]["w1"][0], w1.grad.numpy(), rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(gr[g]["b1"][0], b1.grad.numpy(), rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(gr[g]["w3"][0], w3.grad.numpy()[g * c.N3:(g + 1) * c.N3], rtol=1e-11, atol=1e-11)


def test_split_error_constant():
    """k_x6 as the docstring derives it: worst relative size of the three dropped products of hi + mid + lo splits, measured on
    random fp32 pairs with bf16 rounding done here, stays under 2.02 u; the kept terms' absolute values under 1.016 |a||b|"""
    rng = np.random.default_rng(5)
    a, b = (rng.standard_normal(20000).astype(np.float32) * np.float32(2.0) ** rng.integers(-6, 7, 20000) for _ in range(2))

    def split(v):
        hi = do.bf16_round(v)
        mid = do.bf16_round(v - hi)
        lo = do.bf16_round(v - hi - mid)
        assert ((hi.astype(np.float64) + mid + lo) == v).all(), "the three-term split is exact"
        return hi.astype(np.float64), mid.astype(np.float64), lo.astype(np.float64)
    (ah, am, al), (bh, bm, bl) = split(a), split(b)
    ab = np.abs(a.astype(np.float64) * b)
    dropped = np.abs(am * bl) + np.abs(al * bm) + np.abs(al * bl)
    kept = sum(np.abs(x * y) for x, y in ((am, bm), (ah, bl), (al, bh), (ah, bm), (am, bh), (ah, bh)))
    print("dropped / (u |ab|) <= %.4f, kept / |ab| <= %.5f" % ((dropped / (mo.U * ab)).max(), (kept / ab).max()))
    assert (dropped <= 2.02 * mo.U * ab).all()
    assert (kept <= 1.016 * ab).all()
    assert mo.k_x6(176, 176) == pytest.approx(1.016 * (32 + 36 + 3) + 2.02)


# ================================================================================================ the table against the plan query
@pytest.mark.parametrize("c", mo.CASES, ids=lambda c: c.name)
def test_case_runs_the_plan_it_names(ops, c):
    """every (call, kept) combination: the oracle's restated host arithmetic == marl_mlp3_plan, field by field (refusals included),
    and the fields the case is in the table for"""
    from marl_amd._lib import MarlMlp3Weights  # noqa: F401
    for call, kept in COMBOS:
        got, want = plan_of(ops, c, call, kept), mo.expected_plan(c, call, kept)
        if call.startswith("x6") and not c.x6:
            want = None if not mo.x6_supported(c) else want
        assert same_plan(got, want), "the plan moved: %s %s kept=%d runs %r, named for %r" % (c.name, call, kept, got, want)
        for f, v in c.want.get((call, kept), {}).items():
            assert got is not None and getattr(got, f) == v, "%s %s kept=%d: %s = %r, in the table for %r" % (
                c.name, call, kept, f, got and getattr(got, f), v)
    assert plan_of(ops, c, "fwd", True) is not None, "a case the forward refuses"
    assert c.x6 == mo.x6_supported(c) or not c.x6


def test_table_reaches_every_instantiation(ops):
    """every template instantiation the MLP3_PICK / MLP3_PICK_BIG / MLP3_PICK_WIDE and X6_PICK macros can select is run by a case"""
    reached = set()
    for c in mo.CASES:
        for call, kept in COMBOS:
            if call.startswith("x6") and not c.x6:
                continue          # (the GPU test runs the split pair only where the case says so)
            if call.endswith("fwd") and not kept:
                continue
            p = plan_of(ops, c, call, kept)
            if p is not None:
                reached.add(mo.instance(call, p))
    want = mo.all_instances()
    assert len(want) == len(set(want)) == 64
    missing = [i for i in want if i not in reached]
    assert not missing, "unreached instantiations: %r" % missing
    assert reached <= set(want), "a plan outside the enumeration: %r" % (reached - set(want))


def test_table_reaches_every_listed_seam(ops):
    seen = {"slabs": set(), "kpad": set(), "yvec": set(), "n3": set(), "M": set(), "wide_kc": set(), "kv": set()}
    for c in mo.CASES:
        p = plan_of(ops, c, "fwd", True)
        seen["kpad"].add(p.kpad); seen["n3"].add(c.N3); seen["M"].add(c.M); seen["kv"].add(p.KV)
        if p.wide:
            seen["wide_kc"].add(p.KC)
            seen["yvec"].add(p.yvec)
        for call, kept in (("bwd", False), ("bwd", True), ("x6_bwd", True)):
            q = plan_of(ops, c, call, kept) if (c.x6 or call == "bwd") else None
            if q is not None:
                seen["slabs"].add(q.slabs)
    assert seen["slabs"] >= set(mo.REDUCE_SLABS)
    assert seen["kpad"] == {0, 1, 2, 3}
    assert seen["yvec"] == {True, False}
    assert seen["n3"] >= set(mo.N3_NARROW) | set(mo.N3_WIDE)
    assert seen["M"] >= set(mo.ROWS_M)
    assert seen["wide_kc"] == {8, 16, 24}
    assert seen["kv"] >= set(mo.BUCKETS)
    for KV, KC in mo.BUCKET_KC.items():
        assert mo.kc_bucket(KV) == KC


def test_stripe_walks_the_table_is_named_for(ops):
    """the forward's second tile walk and empty stripes, the backward's second iteration, short last stripe and empty stripes at each
    cap, the iteration whose later waves lie past the end - read off the plans"""
    def shape(c, call, kept, unit):
        p = plan_of(ops, c, call, kept)
        units = (c.M + unit - 1) // unit
        used = (units + p.per - 1) // p.per
        return p, units, used
    p, tiles, used = shape(mo.BY_NAME["fwd-second-walk"], "fwd", True, 16)
    assert p.per > mo.FNW and p.per < 2 * mo.FNW and used == p.nst          # wave 0 walks twice, waves 1 .. 7 once
    for call in ("fwd", "x6_fwd"):
        p, tiles, used = shape(mo.BY_NAME["empty-stripes"], call, True, 16)
        assert (tiles, p.nst, p.per, used) == (193, 24, 9, 22)
    for name, call, kept, nst, per, used_want in (("empty-stripes", "bwd", False, 24, 3, 17), ("empty-stripes", "bwd", True, 48, 2, 25),
                                                 ("empty-stripes", "x6_bwd", True, 48, 2, 25), ("empty-stripes-wide", "bwd", True, 24, 3, 17),
                                                 ("empty-stripes-kc12", "bwd", True, 24, 3, 17)):
        p, its, used = shape(mo.BY_NAME[name], call, kept, 64)
        assert (its, p.nst, p.per, used) == (49, nst, per, used_want), (name, call, kept, p)
        assert its % p.per != 0 and p.per >= 2          # a second iteration, and a last used stripe that is shorter
    assert mo.BY_NAME["rows65"].M % 64 == 1 and mo.BY_NAME["rows17"].M == 17          # iterations whose waves 1 .. 3 / 2, 3 are past the end


# ================================================================================================ data properties
@pytest.mark.parametrize("c", mo.CASES, ids=lambda c: c.name)
def test_case_data_is_what_its_kind_claims(c):
    i = mo.inputs(c, "exact")
    assert i.worst < mo.LIMIT, "%s: a sum of absolute values reaches %g" % (c.name, i.worst)
    assert i.zeros1 > 0 and (c.nl == 2 or i.zeros2 > 0), "no exactly-zero pre-activation: nothing tells > from >="
    assert all((f.p1 > 0).any() and (f.p1 < 0).any() for f in i.f)
    assert (i.dY != 0).any() and all(np.abs(f.Y).max() > 0 for f in i.f)
    for f in i.f:
        assert (f.Y == np.round(f.Y)).all()
    if c.x6:
        assert mo.x6_exact(c, i) <= 8, "%s: a product of the split with two operands wider than 8 bits" % c.name
    for kind in c.kinds:
        if kind == "exact":
            continue
        j = mo.inputs(c, kind)
        assert j.kink.mean() <= mo.KINK_CAP, "%s[%s]: %.3f of the rows on a kink" % (c.name, kind, j.kink.mean())
        assert (j.dY[j.kink] == 0).all()
        if kind == "probe":
            nz = np.flatnonzero((j.dY != 0).any((0, 2)))
            assert set(nz) <= set(j.rows) and {0, c.M - 1} <= set(j.rows)
            assert len(nz) >= min(c.M, 2) - int(j.kink[:, [0, c.M - 1]].all(0).sum())


def test_probe_rows_sit_on_the_planned_seams(ops):
    c = mo.BY_NAME["empty-stripes"]
    rows = set(mo.probe_rows(c))
    for call, kept, unit in (("fwd", True, 16), ("bwd", False, 64), ("bwd", True, 64), ("x6_bwd", True, 64)):
        p = plan_of(ops, c, call, kept)
        step = p.per * unit
        last = (c.M - 1) // step * step
        assert {step - 1, step, last - 1, last} <= rows
    assert {15, 16, 63, 64} <= rows
    c = mo.BY_NAME["seg-remap"]
    assert {14, 15} <= set(mo.probe_rows(c))
    i = mo.inputs(c, "real")
    assert (i.X[:2, :20] == 0).all() and (i.X[15:17, :20] == 0).all() and (i.X[2, :20] != 0).any()          # rows that read as zero
    assert np.isnan(i.d.store0[:18]).all() and (i.d.idx == -1).any()


# ================================================================================================ the capability predicates
def test_predicates_agree_with_the_plan(ops):
    for c in list(mo.CASES) + list(mo.REFUSED):
        x = fab_src(c.src)
        sup = ops.mlp3_supported(x, c.K1, 64, 64 if c.nl == 3 else 0, c.N3, c.G)
        assert sup == mo.supported(c), c.name
        assert sup == (plan_of(ops, c, "fwd", True) is not None), c.name
        assert sup == (plan_of(ops, c, "bwd", True) is not None), c.name
        x6 = ops.mlp3_x6_supported(x, c.K1, 64, 64 if c.nl == 3 else 0, c.N3, c.G)
        assert x6 == mo.x6_supported(c), c.name
        assert x6 == (plan_of(ops, c, "x6_fwd", True) is not None) == (plan_of(ops, c, "x6_bwd", True) is not None), c.name
        if sup:
            nk = ops.mlp3_needs_kept(x, c.K1, c.N3)
            assert nk == mo.needs_kept(c) == (plan_of(ops, c, "bwd", False) is None), c.name
    assert all(not mo.supported(c) for c in mo.REFUSED)


def test_needs_kept_formula_across_the_bucket_seams(ops):
    """the formula tests/test_gpu_kernels.py::test_mlp3_fused asserts, at every state width around every bucket step"""
    for S in list(range(4, 40)) + [s + d for s in (64, 128, 160, 176, 192, 256, 384, 508) for d in range(-4, 5)]:
        for N3 in (1, 16, 20):
            x = fab_src(do.src(k0=S))
            if not ops.mlp3_supported(x, S, 64, 0, N3, 2):
                continue
            assert ops.mlp3_needs_kept(x, S, N3) == ((S + (-S) % 4 + 15) // 16 > 12 or N3 > 16), (S, N3)


def test_wide_kc24_alignment_seam(ops):
    """a WIDE head at 24 chunks needs 165 888 - 128 CF bytes of LDS in the backward: with 16-byte state rows (CF >= 16) it is supported,
    with rows off the grid (CF = 0) marl_mlp3_supported says 0 and every entry point refuses - network/mixer.py then composes
    marl_linear"""
    al, un = mo.BY_NAME["wide160-kc24"], mo.REFUSED[1]
    assert (al.src.k0, al.N3, al.nl) == (un.src.k0, un.N3, un.nl) and mo.vec_rows(al.src) and not mo.vec_rows(un.src)
    p = plan_of(ops, al, "bwd", True)
    assert p is not None and (p.KC, p.CF, p.lds) == (24, 20, 165888 - 128 * 20) and p.lds <= mo.LDS_MAX
    assert mo.bwd_lds(24, 0, True, True, False) == 165888 > mo.LDS_MAX
    for call, kept in COMBOS:
        assert plan_of(ops, un, call, kept) is None
    assert not ops.mlp3_supported(fab_src(un.src), un.K1, 64, 0, un.N3, un.G)
    for off0 in (1, 2, 3):          # a base off the grid does the same
        s = do.src(k0=322, off0=off0)
        assert not ops.mlp3_supported(fab_src(s), 322, 64, 0, 160, 2)
    for CF in range(0, 21):
        assert (mo.bwd_lds(24, CF, True, True, False) <= mo.LDS_MAX) == (CF >= 16)


def test_call_refusals_on_the_host(ops):
    """what the entry points refuse beyond the shape: recompute where needs_kept, WIDE dY off the grid, short hsave, short workspace,
    unaligned b1, a gradient struct of the other depth"""
    c = mo.BY_NAME["kv193-l3"]
    assert plan_of(ops, c, "bwd", False) is None and plan_of(ops, c, "bwd", True) is not None
    w = mo.BY_NAME["wide32"]
    lay = mo.dy_layout(w)
    for bad in (mo.NS(ld=lay.ld + 1, gs=lay.gs, off=0), mo.NS(ld=lay.ld, gs=lay.gs, off=1), mo.NS(ld=w.N3, gs=w.M * w.N3 + 2, off=0)):
        assert plan_of(ops, w, "bwd", True, lay=bad) is None
    for c in (mo.BY_NAME["rows65"], w):
        need = ops.mlp3_save_floats(c.M, c.nl == 3, c.G)
        for call in ("fwd", "bwd") + (("x6_fwd", "x6_bwd") if c.x6 else ()):
            assert plan_of(ops, c, call, True, hsave_floats=need) is not None
            assert plan_of(ops, c, call, True, hsave_floats=need - 1) is None
            assert plan_of(ops, c, call, True, hsave=BASE["H"] + 4, hsave_floats=need) is None
            if call.endswith("bwd"):
                from marl_amd import _lib
                ws = _lib.load().marl_mlp3_bwd_workspace(c.M, c.K1, c.N3, c.G)
                assert plan_of(ops, c, call, True, ws_bytes=ws) is not None and plan_of(ops, c, call, True, ws_bytes=ws - 4) is None
        for call in ("fwd", "bwd") + (("x6_fwd",) if c.x6 else ()):
            assert ops.mlp3_plan(call, fab_weights(c, BASE["W"], boff=1), fab_src(c.src), c.M, c.K1, c.N3, c.G, Y=BASE["Y"],
                                 grads=fab_weights(c, BASE["G"]), hsave=BASE["H"]) is None
    c3, c2 = mo.BY_NAME["n3=4-l3"], mo.BY_NAME["n3=4-l2"]
    assert ops.mlp3_plan("bwd", fab_weights(c3, BASE["W"]), fab_src(c3.src), c3.M, c3.K1, c3.N3, c3.G, Y=BASE["Y"],
                         grads=fab_weights(c2, BASE["G"]), hsave=BASE["H"]) is None
