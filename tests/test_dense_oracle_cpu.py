"""tests/dense_oracle.py on the CPU: its case table is held to the library's own plan queries (marl_linear_plan,
marl_linear_wgrad_plan: the host functions the launches themselves decide with - no GPU, pointer VALUES of the right alignment stand
for device memory), its data to the properties the cases are named for, and its bounds to the ceilings of the older tests."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import dense_oracle as do

BASE = {"p0": 1 << 20, "m0": 2 << 20, "p1": 3 << 20, "idx": 4 << 20, "emap": 5 << 20, "W": 6 << 20, "b": 7 << 20, "dY": 8 << 20, "Ya": 9 << 20}


@pytest.fixture(scope="module")
def ops():
    from marl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    from marl_amd import ops
    return ops


def fab_src(s, ptr=None):
    """a MarlSrc for a source description; ptr: name -> pointer value (default: fabricated values off the grid as the description says)"""
    from marl_amd._lib import MarlSrc
    ptr = ptr or {"p0": BASE["p0"] + 4 * s.off0, "m0": BASE["m0"] + 4 * s.moff, "p1": BASE["p1"], "idx": BASE["idx"], "emap": BASE["emap"]}
    m = MarlSrc()
    if s.k0:
        m.p0, m.ld0, m.k0 = ptr["p0"], s.ld0, s.k0
        if s.gate:
            m.m0, m.ldm0 = ptr["m0"], s.ldm
        if s.remap0:
            m.rpe0, m.bs0, m.off0 = s.remap0
        if s.emap:
            m.emap0 = ptr["emap"]
    if s.k1:
        m.p1, m.ld1, m.k1 = ptr["p1"], s.k1, s.k1
    if s.nhot:
        m.idx, m.nhot, m.hot_w = ptr["idx"], s.nhot, s.hot_w
        if s.remapi:
            m.rpei, m.bsi, m.offi = s.remapi
    m.nid = s.nid
    return m


def lin_plan(ops, c, ptr=None, M=None, N=None, W=None, bias=None):
    M, N = c.M if M is None else M, c.N if N is None else N
    lay = do.lin_layout(c, N)
    grp = ops.group(c.groups, w=lay.gs_w, b=lay.gs_b, y=lay.gs_y) if c.groups > 1 else None
    return ops.linear_plan(fab_src(c.src, ptr), BASE["W"] + 4 * c.woff if W is None else W, lay.ldw, lay.ldy, M, N, c.K, act=c.act,
                           w_kmajor=c.kmajor, grp=grp, bf16=c.bf16, bias=(BASE["b"] if c.bias else None) if bias is None else bias)


def wg_plan(ops, c, ptr=None, dY=None, Ya=None, ws_bytes=None):
    lay = do.wg_layout(c)
    grp = ops.group(c.groups, w=lay.gs_w, b=lay.gs_b, y=lay.gs_y, m0=lay.gs_y) if c.groups > 1 else None
    dY = BASE["dY"] + 4 * c.goff if dY is None else dY
    Ya = (BASE["Ya"] if Ya is None else Ya) if c.gate else None
    return ops.linear_wgrad_plan(dY, lay.ldg, fab_src(c.src, ptr), c.M, c.N, c.K, Yact=Ya, ldya=lay.ldg if c.gate else 0, grp=grp,
                                 bf16=c.bf16, ws_bytes=ws_bytes)


class tall_switch:
    """run under marl_experiment_set("wgrad_tall", v); restores 1"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        from marl_amd import _lib
        assert _lib.load().marl_experiment_set(b"wgrad_tall", self.v) == 0

    def __exit__(self, *a):
        from marl_amd import _lib
        assert _lib.load().marl_experiment_set(b"wgrad_tall", 1) == 0


def wg_expect(c):
    return (c.plan[0], tuple(c.plan[1]), c.plan[2], c.plan[3])


def wg_got(p):
    return None if p is None else (p.family, tuple(p.inst), p.passes, p.slabs)


# ------------------------------------------------------------------------------------------------ the oracle itself
def test_virtual_x_is_the_cat_construction_of_the_older_tests():
    """virtual_x against torch.cat of [x0 | x1 | one-hot blocks | eye(nid)[row % nid]] as tests/test_gpu_kernels.py builds its inputs,
    plain and through the (T+1)-slot remap with the shifted action of test_wgrad_large_rows_and_remap"""
    rng = np.random.default_rng(3)
    M, s = 75, do.src(k0=20, k1=9, nhot=3, hot_w=4, nid=5)
    d = do.make_src(s, M, rng, "real")
    idx = torch.from_numpy(d.idx).long()
    oh = torch.zeros(M, 3, 4)
    for j in range(3):
        v = idx[:, j] >= 0
        oh[v, j, idx[v, j]] = 1
    X = torch.cat([torch.from_numpy(d.store0[:, :20]), torch.from_numpy(d.x1), oh.reshape(M, -1), torch.eye(5)[torch.arange(M) % 5]], 1)
    assert np.array_equal(do.virtual_x(s, d, M), X.double().numpy())
    B, T, N, O = 3, 7, 5, 6
    for t0, uoff in ((0, -1), (1, 0)):
        s = do._learner_src(B, T, N, O, 7, t0=t0, uoff=uoff)
        d = do.make_src(s, B * T * N, rng, "real")
        store = torch.from_numpy(d.store0[:, :O]).reshape(B, T + 1, N, O)
        u = torch.from_numpy(d.idx).long().reshape(B, T, N)
        up = torch.full((B, T, N), -1, dtype=torch.long)
        if uoff == -1:
            up[:, 1:] = u[:, :-1]
        else:
            up = u.clone()
        oh = torch.zeros(B * T * N, 7)
        flat = up.reshape(-1)
        oh[flat >= 0, flat[flat >= 0]] = 1
        X = torch.cat([store[:, t0:t0 + T].reshape(B * T * N, O), oh, torch.eye(N)[torch.arange(B * T * N) % N]], 1)
        assert np.array_equal(do.virtual_x(s, d, B * T * N), X.double().numpy())
    # a gate of 0.0 or -0.0 closes; rows before the first slot read as zero although storage row 0 is NaN
    s = do.src(k0=4, gate=True, remap0=(5, 6, -2), emap=True)
    d = do.make_src(s, 20, rng, "exact")
    X = do.virtual_x(s, d, 20)
    assert np.isnan(d.store0[0]).all() and (X[np.arange(20) % 5 < 2] == 0).all() and d.emap.min() >= 1
    g = d.gate0[:, :4]
    assert (g == 0).any() and np.signbit(g[g == 0]).any() and not np.signbit(g[g == 0]).all()
    r0, ok = do._remap(np.arange(20), s.remap0, d.emap)
    assert (X[ok][d.gate0[r0[ok], :4] <= 0] == 0).all()
    # dX = (dY * (gate > 0)) W is the gated k-major forward case: the stored [K, N] matrix is the layer's own W
    c = next(c for c in do.LIN_CASES if c.name == "lin-gate-misaligned")
    i = do.lin_inputs(c, "exact")
    assert np.array_equal(do.dx(i.d.store0[:, :64], i.d.gate0[:, :64], i.W[0].T) + i.Y0, i.Y)
    assert do.bf16_round(np.float32([1.0, 1.00390625, 1.01171875, -3.0])).tolist() == [1.0, 1.0, 1.015625, -3.0]      # ties to even


def test_exact_data_is_order_free():
    """every exact case: sum |g||x| (+ the base) stays below 2^24 per element, and an fp32 evaluation gives the float64 bits in two row
    orders"""
    for c in do.WG_CASES:
        if c.M > 10000 and c.name not in ("tall-M131009",):
            M = c.M                      # (the large ones: the magnitude argument alone, no second evaluation)
            assert 16.0 * M + 3 < 2 ** 24, c.name
            continue
        i = do.wg_inputs(c, "exact")
        G = do.gated(i.dY, i.Yact)
        N = c.N
        for g in range(c.groups):
            Gg = G[:, g * N:(g + 1) * N]
            assert (np.abs(Gg).T @ np.abs(i.X)).max() + 3 < 2 ** 24 and np.abs(Gg).sum(0).max() + 3 < 2 ** 24, c.name
            perm = np.random.default_rng(1).permutation(c.M)
            for order in (np.arange(c.M), perm):
                acc = np.zeros((N, c.K), np.float32)
                for blk in np.array_split(order, max(1, c.M // 512)):          # fp32 partial sums, block by block
                    acc += (Gg[blk].astype(np.float32).T @ i.X[blk].astype(np.float32))
                assert np.array_equal(acc.astype(np.float64), i.dW[g]), c.name
        assert np.array_equal(do.bf16_round(i.X.astype(np.float32)), i.X.astype(np.float32))       # bf16 holds these operands exactly
    for c in do.LIN_CASES:
        i = do.lin_inputs(c, "exact")
        assert i.mag.max() < 2 ** 24 and np.array_equal(i.Y, i.Y.astype(np.float32).astype(np.float64)), c.name
        Y32 = np.concatenate([i.X[:, ::-1].astype(np.float32) @ i.W[g][:, ::-1].T for g in range(c.groups)], 1).astype(np.float64)
        want = np.concatenate([do.linear(i.X, i.W[g]) for g in range(c.groups)], 1)
        assert np.array_equal(Y32, want), c.name


def test_probe_rows_are_the_seams_of_the_planned_kernel(ops):
    """every probe case: dY is nonzero exactly on the rows named, and the slab seams named are where the slab of a row changes under the
    slab count THE PLAN reports (the kernels' own `per` arithmetic, restated once in dense_oracle.slab_of)"""
    for c in do.WG_CASES:
        if c.M > 10000 and not c.name.startswith("tall-M1310"):
            continue
        with tall_switch(c.tall):
            p = wg_plan(ops, c)
        fam, slabs = p.family, p.slabs
        i = do.wg_inputs(c, "probe", slabs=slabs)
        nz = np.flatnonzero((i.dY != 0).any(1))
        assert np.array_equal(nz, i.rows) and 2 <= len(nz) <= 24 or c.M == 1, (c.name, nz)
        assert 0 in nz and c.M - 1 in nz
        sl = do.slab_of(fam, c.M, slabs, np.arange(c.M))
        assert sl.max() < slabs
        for cut in do.seams(fam, c.M, slabs):
            assert sl[cut - 1] != sl[cut] and cut - 1 in nz and cut in nz, (c.name, cut)
        if fam in ("tall", "thin"):          # contiguous row ranges of ceil(M / slabs) rows
            per = -(-c.M // slabs)
            assert do.seams(fam, c.M, slabs)[0] == per
        if fam in ("generic", "full") and slabs > 1:
            per = -(-(-(-c.M // 64)) // slabs)
            assert do.seams(fam, c.M, slabs)[0] == 64 * per
        if c.src.remap0:
            assert c.src.remap0[0] - 1 in nz and c.src.remap0[0] in nz
        # each gradient element is a sum of at most len(rows) nonzero terms
        _, nnz, _, nnzb = do.wgrad_mag(i.dY[:, :c.N], None if i.Yact is None else i.Yact[:, :c.N], i.X)
        assert nnz.max() <= len(nz) and nnzb.max() <= len(nz)


# ------------------------------------------------------------------------------------------------ the plans
@pytest.mark.parametrize("c", do.WG_CASES, ids=lambda c: c.name)
def test_wgrad_case_runs_the_plan_it_is_named_for(ops, c):
    with tall_switch(c.tall):
        p = wg_plan(ops, c)
    assert wg_got(p) == wg_expect(c), "the plan moved"
    assert p.gvec == (c.goff == 0 and do.wg_layout(c).ldg % 4 == 0 and (c.groups == 1 or c.N % 4 == 0)) and p.xvec == (c.src.off0 == 0 and c.src.ld0 % 4 == 0 and not c.src.gate)
    if c.plan[0] == "passes":
        assert p.c_rest == (128 if c.src.k0 >= 128 else 64)
    if c.name.endswith("-generic"):          # one step past a kernel's range: the generic kernel
        assert p.family == "generic"


@pytest.mark.parametrize("c", do.LIN_CASES, ids=lambda c: c.name)
def test_linear_case_runs_the_plan_it_is_named_for(ops, c):
    p = lin_plan(ops, c)
    nc = c.plan[1]
    assert p[:6] == c.plan, "the plan moved"
    assert p.grid == ((c.M + 127) // 128, (c.N + 16 * nc - 1) // (16 * nc), c.groups)


def test_linear_sweep_plans(ops):
    c = do.lin("sweep", 1, 1, do.src(k0=1))
    for k0 in do.LIN_K0:
        c.src, c.K = do.src(k0=k0), k0
        for M in do.LIN_M:
            for N in do.LIN_N:
                p = lin_plan(ops, c, M=M, N=N)
                assert (p.path, p.tiles, p.grid) == do.lin_sweep_plan(M, N, k0) and not (p.gate or p.kmajor or p.bf16), "the plan moved"
    assert lin_plan(ops, c, M=33, N=80).grid[1] == 1 and lin_plan(ops, c, M=33, N=81).grid[1] == 2      # 5 tiles in one block, 4 in two


def test_tables_reach_every_instantiation(ops):
    """the weight-gradient table reaches every instantiation of every kernel (the direct and the column-pass ones with the tall kernel
    switched on AND off), every slab count either side of the reduce kernel's 16 slab groups, and the forward table every
    (operand path, k-major, gate, bf16, tiles) combination of linear_kernel"""
    seen, seen_sw, slabs = set(), set(), set()
    for c in do.WG_CASES:
        with tall_switch(c.tall):
            p = wg_plan(ops, c)
        seen.add((p.family, tuple(p.inst)))
        seen_sw.add((p.family, c.tall))
        slabs.add(p.slabs)
    assert seen == set(do.WG_INSTANCES), seen ^ set(do.WG_INSTANCES)
    assert {("direct", 0), ("direct", 1), ("passes", 0), ("passes", 1)} <= seen_sw
    assert set(do.REDUCE_SLABS) <= slabs, slabs
    combos = {lin_plan(ops, c)[:5] for c in do.LIN_CASES}
    want = {(path, nc, gate, km, bf) for path in ops.LINEAR_PATHS for km in (False, True) for gate in (False, True)
            for bf, nc in ((False, 4), (False, 5), (True, 4))}
    assert want <= combos, want - combos
    # (bf16 at 5 tiles is no instantiation: the planner never asks for it)
    c = do.lin("bf16-70", 33, 70, do.src(k0=47), bf16=True)
    assert lin_plan(ops, c).tiles == 4


def test_plan_queries_follow_the_switch_the_workspace_and_the_refusals(ops):
    from marl_amd import _lib
    lib = _lib.load()
    c = do.wg("t", 131009, 64, do.src(k0=16), None)
    need = lib.marl_linear_wgrad_workspace(c.M, 64, 16, 1)
    assert wg_plan(ops, c, ws_bytes=need).slabs == 512 and wg_plan(ops, c, ws_bytes=need - 4) is None      # too small: refused, as the launch is
    c = do.wg("t", 4100, 64, do.src(k0=64), None)
    assert wg_plan(ops, c).family == "tall"
    with tall_switch(0):
        assert wg_got(wg_plan(ops, c)) == ("direct", (1, 0), 1, 8)
    assert wg_plan(ops, c).family == "tall"
    c.K = 65          # the source is 64 wide
    assert wg_plan(ops, c) is None
    plan = (C.c_int * 8)()
    assert lib.marl_linear_wgrad_plan(None, 0, None, 0, C.byref(fab_src(c.src)), 0, 64, 64, 0, None, 0, plan) == 0 and plan[0] == -1


# ------------------------------------------------------------------------------------------------ the bounds
def test_bounds_are_never_looser_than_the_older_ceilings():
    """forward / dX: (terms + 3) u (sum |x||w| + |b| + |beta Y0|) on the real data of every case stays under the tightest absolute
    tolerance the older tests hold these kernels to; probe data: (nnz + 3) u sum |g||x| stays under the ceiling used for real data"""
    for c in do.LIN_CASES:
        i = do.lin_inputs(c, "real")
        assert (do.k_dot(c.src) * do.U * i.mag).max() < do.OLD_FWD_CEILING, c.name
    for k0 in do.LIN_K0:
        c = do.lin("sweep", 129, 130, do.src(k0=k0))
        assert (do.k_dot(c.src) * do.U * do.lin_inputs(c, "real").mag).max() < do.OLD_FWD_CEILING
    for c in do.WG_CASES:
        if c.M > 10000:
            continue
        i = do.wg_inputs(c, "probe")
        for g in range(c.groups):
            sl = slice(g * c.N, (g + 1) * c.N)
            mag, nnz, magb, nnzb = do.wgrad_mag(i.Gr[:, sl], None if i.Yact is None else i.Yact[:, sl], i.Xr)
            assert ((nnz + 3) * do.U * mag <= do.wgrad_ceiling(i.dW[g], c.M)).all(), c.name
            assert ((nnzb + 3) * do.U * magb <= do.wgrad_ceiling(i.db[g], c.M)).all(), c.name
