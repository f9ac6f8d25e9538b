"""Float64 statement of the dense-layer kernels of csrc/gemm.hip (marl_linear, marl_linear_wgrad) and the table of cases that
tests/test_gpu_dense.py runs and tests/test_dense_oracle_cpu.py holds to the library's own plan queries (marl_linear_plan,
marl_linear_wgrad_plan).  Plain numpy: nothing here imports marl_amd.

A source description (`src`) says what include/marl_hip.h's marl_src_t says, without pointers: widths, row strides, how far a base
sits off the 16-byte grid (in floats), remaps.  `make_src` fills its storage; `virtual_x` is the [M, K] matrix it denotes.

Three kinds of data:
  exact   every operand a small integer stored as fp32 (|v| <= 4, many zeros; the relu gates hold 0.0, -0.0 and +-1; bias and the
          base contents of Y, dW, db integers): every product is at most 16 and every sum stays below 2^24 at the largest M here,
          so fp32 kernels, bf16-operand kernels and float64 give THE SAME BITS in any summation order
  probe   real-valued X; dY exactly zero but on a few named rows (first, last, either side of the first chunk seam, of the first and
          the last slab seam of the planned kernel and of an episode seam): each gradient element is a sum of at most that many
          nonzero terms, and adding an exact zero is exact in any order
  real    dense Gaussian data
"""
import types

import numpy as np

NS = types.SimpleNamespace
U = 2.0 ** -24
F32, F64 = np.float32, np.float64
NAN = np.float32(np.nan)


# ================================================================================================ sources
def src(k0=0, ld0=None, off0=0, k1=0, nhot=0, hot_w=0, nid=0, gate=False, ldm=None, moff=0, remap0=None, remapi=None, emap=False,
        gs_x0=0):
    """k0 / ld0 / off0: dense segment 0, its row stride (default: k0 rounded up to 4) and its base offset in floats off the 16-byte
    grid; gate / ldm / moff: the relu gate on it; remap0 / remapi: (rpe, bs, off); emap: read episodes through a map that never
    names storage episode 0 (which is then all NaN: storage row 0 is what a row reading as zero makes the kernels load)"""
    ld0 = (k0 + 3) // 4 * 4 if ld0 is None else ld0
    return NS(k0=k0, ld0=ld0, off0=off0, k1=k1, nhot=nhot, hot_w=hot_w, nid=nid, gate=gate, ldm=ld0 if ldm is None else ldm, moff=moff,
              remap0=remap0, remapi=remapi, emap=emap, gs_x0=gs_x0)


def width(s):
    return s.k0 + s.k1 + s.nhot * s.hot_w + s.nid


def terms(s):
    """columns of a row that can be nonzero: the dense ones, one per one-hot block, one of the agent id"""
    return s.k0 + s.k1 + s.nhot + (1 if s.nid else 0)


def _episodes(M, remap):
    return (M + remap[0] - 1) // remap[0]


def _values(rng, shape, kind, zeros=0.4):
    if kind == "exact":
        v = rng.integers(-4, 5, size=shape).astype(F32)
        return np.where(rng.random(shape) < zeros, F32(0), v).astype(F32)
    return rng.standard_normal(shape).astype(F32)


def _gate_values(rng, shape, kind):
    """relu gates: 0.0, -0.0 and +-1 on exact data; Gaussian with exact 0.0 / -0.0 sprinkled in otherwise"""
    pick = rng.integers(0, 4, size=shape)
    four = np.array([0.0, -0.0, 1.0, -1.0], dtype=F32)[pick]
    if kind == "exact":
        return four
    g = rng.standard_normal(shape).astype(F32)
    return np.where(rng.random(shape) < 0.1, four, g).astype(F32)


def make_src(s, M, rng, kind):
    """storage of a source: store0 [rows0, ld0] (pad columns NaN), gate0 [rows0, ldm], x1 [M, k1], idx [rowsi, nhot] int32, emap int32"""
    d = NS(store0=None, gate0=None, x1=None, idx=None, emap=None)
    if s.k0:
        rows0 = M
        if s.remap0:
            E = _episodes(M, s.remap0)
            store_eps = E + 3 if s.emap else E
            rows0 = store_eps * s.remap0[1]
            if s.emap:
                d.emap = (1 + rng.permutation(store_eps - 1)[:E]).astype(np.int32)      # never storage episode 0
        d.store0 = np.full((rows0, s.ld0), NAN, dtype=F32)
        d.store0[:, :s.k0] = _values(rng, (rows0, s.k0), kind)
        if s.gate:
            d.gate0 = np.full((rows0, s.ldm), NAN, dtype=F32)
            d.gate0[:, :s.k0] = _gate_values(rng, (rows0, s.k0), kind)
        if s.emap:
            d.store0[:s.remap0[1]] = NAN
            if s.gate:
                d.gate0[:s.remap0[1]] = NAN
    if s.k1:
        d.x1 = _values(rng, (M, s.k1), kind)
    if s.nhot:
        rowsi = _episodes(M, s.remapi) * s.remapi[1] if s.remapi else M
        d.idx = rng.integers(-1, s.hot_w, size=(rowsi, s.nhot)).astype(np.int32)
    return d


def _remap(rows, remap, emap):
    if remap is None:
        return rows, np.ones(rows.shape, dtype=bool)
    rpe, bs, off = remap
    e, w = rows // rpe, rows % rpe + off
    ok = w >= 0
    e = emap[e].astype(np.int64) if emap is not None else e
    return np.where(ok, e * bs + w, 0), ok


def virtual_x(s, d, M):
    """the [M, K] float64 matrix that the source denotes (include/marl_hip.h: marl_src_t)"""
    rows = np.arange(M, dtype=np.int64)
    parts = []
    if s.k0:
        r0, ok = _remap(rows, s.remap0, d.emap)
        x0 = d.store0[r0, :s.k0].astype(F64)
        if s.gate:
            x0 = np.where(d.gate0[r0, :s.k0] > 0, x0, 0.0)
        parts.append(np.where(ok[:, None], x0, 0.0))
    if s.k1:
        parts.append(d.x1[:, :s.k1].astype(F64))
    if s.nhot:
        ri, ok = _remap(rows, s.remapi, None)
        oh = np.zeros((M, s.nhot, s.hot_w))
        for j in range(s.nhot):
            a = d.idx[ri, j]
            v = ok & (a >= 0)
            oh[rows[v], j, a[v]] = 1.0
        parts.append(oh.reshape(M, -1))
    if s.nid:
        parts.append(np.eye(s.nid)[rows % s.nid])
    X = np.concatenate(parts, 1)
    assert X.shape == (M, width(s)) and np.isfinite(X).all()
    return X


# ================================================================================================ the operations
def bf16_round(x):
    """fp32 -> bf16 -> fp32, round to nearest even (finite inputs)"""
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000
    return b.astype(np.uint32).view(F32).reshape(np.shape(x))


def linear(X, W, b=None, act=0, beta=0.0, Y0=None):
    """Y = act(X W^T + b) + beta Y0 in float64 (beta == 0: Y0 is not read - it may hold NaN)"""
    Y = np.asarray(X, F64) @ np.asarray(W, F64).T
    if b is not None:
        Y = Y + np.asarray(b, F64)
    if act:
        Y = np.maximum(Y, 0.0)
    if beta != 0.0:
        Y = Y + beta * np.asarray(Y0, F64)
    return Y


def linear_mag(X, W, b=None, beta=0.0, Y0=None):
    """sum |x||w| + |b| + |beta Y0|: what the dot-product bound multiplies"""
    m = np.abs(np.asarray(X, F64)) @ np.abs(np.asarray(W, F64)).T
    if b is not None:
        m = m + np.abs(np.asarray(b, F64))
    if beta != 0.0:
        m = m + np.abs(beta * np.asarray(Y0, F64))
    return m


def dx(dY, gate, W):
    """dX = (dY * (gate > 0)) W, W [N, K]"""
    G = np.asarray(dY, F64)
    if gate is not None:
        G = np.where(np.asarray(gate) > 0, G, 0.0)
    return G @ np.asarray(W, F64)


def gated(dY, Yact):
    G = np.asarray(dY, F64)
    return G if Yact is None else np.where(np.asarray(Yact) > 0, G, 0.0)


def wgrad(dY, Yact, X, groups=1):
    """(dW, db) = (G^T X, column sums of G), G = dY * (Yact > 0).  groups > 1: dY / Yact are [M, groups * N], group g owning columns
    [g N, (g + 1) N); X is shared [M, K] or per group [groups, M, K]; returns [groups, N, K], [groups, N]"""
    G = gated(dY, Yact)
    X = np.asarray(X, F64)
    if groups == 1:
        return G.T @ X, G.sum(0)
    N = G.shape[1] // groups
    dW = np.stack([G[:, g * N:(g + 1) * N].T @ (X if X.ndim == 2 else X[g]) for g in range(groups)])
    return dW, np.stack([G[:, g * N:(g + 1) * N].sum(0) for g in range(groups)])


def wgrad_mag(dY, Yact, X):
    """(sum |g||x|, nonzero terms) per element of dW, and the same for db (x = 1)"""
    G = gated(dY, Yact)
    X = np.asarray(X, F64)
    return (np.abs(G).T @ np.abs(X), (G != 0).astype(F64).T @ (X != 0).astype(F64), np.abs(G).sum(0), (G != 0).sum(0).astype(F64))


# ================================================================================================ bounds
def k_dot(s):
    """forward / dX on real data: |got - ref| <= (terms + 3) u (sum |x||w| + |b| + |beta Y0|) - the dot-product bound
    gamma_n ~ n u of an n-term sum in any order, n = the columns of a row that can be nonzero (products with an exact zero add
    nothing), + 3 for the bias add, the beta Y0 multiply-add and the reference's own rounding to fp32-sized magnitudes.  bf16
    operands: the reference rounds its operands the same way and bf16 products are exact in fp32, so the same bound holds."""
    return terms(s) + 3


def wgrad_ceiling(ref, M):
    """weight gradient on real data, per element: the ceilings the older tests of the same kernels hold (test_gpu_kernels.py)"""
    ref = np.abs(np.asarray(ref, F64))
    if M >= 2048:
        return 2e-3 + 1e-3 * ref
    sc = max(1.0, M ** 0.5)
    return (3e-4 + 3e-4 * ref / sc) * sc


OLD_FWD_CEILING = 2e-4          # the tightest absolute tolerance test_gpu_kernels.py holds a forward / dX result to


# ================================================================================================ slabs and seams
CHUNK = {"tall": 32, "generic": 64, "full": 64, "thin": 0, "direct": 16, "passes": 16}


def slab_of(family, M, slabs, rows):
    """the slab (workgroup) that reduces each row, by the kernels' own `per` arithmetic"""
    rows = np.asarray(rows, dtype=np.int64)
    if family in ("generic", "full"):
        chunks = (M + 63) // 64
        per = (chunks + slabs - 1) // slabs
        return (rows // 64) // per
    if family in ("tall", "thin"):
        per = (M + slabs - 1) // slabs
        return rows // per
    return ((rows // 16) // 8) % slabs          # direct: 16-row blocks dealt to the 8 waves of workgroup 0, 1, ... in rounds


def seams(family, M, slabs):
    """(first, last) row that starts a new slab, or () when all rows are in one"""
    sl = slab_of(family, M, slabs, np.arange(M))
    cut = 1 + np.flatnonzero(sl[1:] != sl[:-1])
    return (int(cut[0]), int(cut[-1])) if cut.size else ()


def probe_rows(family, M, slabs, episode=None):
    """the rows on which a probe case's dY is nonzero: first, last, and the two rows either side of the first chunk seam (32 rows in
    the tall kernel, 16 and 64 in the direct one, 64 otherwise), of the first and the last slab seam and of the first episode seam"""
    at = [0, M - 1]
    cuts = [64] + ([CHUNK[family]] if CHUNK[family] else []) + list(seams(family, M, slabs)) + ([episode] if episode else [])
    for c in cuts:
        at += [c - 1, c]
    return np.array(sorted({r for r in at if 0 <= r < M}), dtype=np.int64)


def make_dy(M, cols, rng, kind, rows=None):
    if kind == "probe":
        dY = np.zeros((M, cols), dtype=F32)
        dY[rows] = rng.standard_normal((len(rows), cols)).astype(F32)
        return dY
    return _values(rng, (M, cols), kind)


# ================================================================================================ cases: marl_linear
LIN_M = (1, 31, 32, 33, 127, 128, 129)
LIN_N = (1, 15, 16, 17, 64, 65, 80, 81, 130)
LIN_K0 = (1, 15, 16, 17, 47, 64)


def lin(name, M, N, s, kmajor=False, ldw_pad=0, woff=0, act=0, beta=0.0, bias=True, groups=1, bf16=False, plan=None):
    """plan: (path, tiles, gate, kmajor, bf16, wvec) the case is named for"""
    return NS(name=name, M=M, N=N, src=s, K=width(s), kmajor=kmajor, ldw_pad=ldw_pad, woff=woff, act=act, beta=beta, bias=bias,
              groups=groups, bf16=bf16, plan=plan)


def _lin_cases():
    out = []
    # every (operand path, k-major, gate, bf16, tiles) combination of linear_kernel: 3 x 2 x 2 x (fp32 at 4 and 5 tiles, bf16 at 4)
    for path in ("element", "vector", "dword"):
        for km in (False, True):
            for gate in (False, True):
                for bf, nc in ((False, 4), (False, 5), (True, 4)):
                    k0 = 15 if path == "element" else 47
                    s = src(k0=k0, ld0=49 if path == "dword" else None, gate=gate)
                    N = 70 if nc == 5 else 17
                    out.append(lin("lin-%s-%s-%s-%s-%d" % (path, "kmajor" if km else "rowmajor", "gate" if gate else "plain",
                                                            "bf16" if bf else "fp32", nc), 33, N, s, kmajor=km, act=int(not km),
                                   beta=1.0 if km else 0.0, bias=not km, bf16=bf,
                                   plan=(path, nc, gate, km, bf, not km)))
    # the ways onto the dword path, one at a time
    out.append(lin("lin-base+1", 129, 65, src(k0=64, off0=1), act=1, plan=("dword", 5, False, False, False, True)))
    out.append(lin("lin-gate-misaligned", 129, 64, src(k0=64, gate=True, moff=1), kmajor=True, beta=1.0, bias=False,
                   plan=("dword", 4, True, True, False, False)))
    out.append(lin("lin-gate-odd-ldm", 33, 16, src(k0=32, gate=True, ldm=33), plan=("dword", 4, True, False, False, True)))
    # W rows off the 16-byte grid: no vector reads of W
    out.append(lin("lin-ldw-odd", 129, 81, src(k0=64), ldw_pad=1, act=1, plan=("vector", 4, False, False, False, False)))
    out.append(lin("lin-w-base+1", 33, 17, src(k0=32), woff=1, plan=("vector", 4, False, False, False, False)))
    # the full concat [x0 | x1 | 3 one-hots | id] through a remap that sends rows negative and an episode map; storage row 0 is NaN
    out.append(lin("lin-concat-remap", 75, 13, src(k0=20, k1=9, nhot=3, hot_w=4, nid=5, remap0=(15, 18, -2), emap=True), act=1,
                   plan=("vector", 4, False, False, False, True)))
    out.append(lin("lin-concat-gate", 130, 130, src(k0=17, ld0=17, k1=9, nhot=3, hot_w=4, nid=5, gate=True), beta=1.0,
                   plan=("dword", 4, True, False, False, True)))
    # 4 groups: shared input, weights and biases strided inside one flat buffer, outputs in column blocks of one tensor
    out.append(lin("lin-groups", 75, 6, src(k0=40), act=1, groups=4, plan=("vector", 4, False, False, False, False)))
    return out


LIN_CASES = _lin_cases()


def ceil4(n):
    return (n + 3) // 4 * 4


def lin_layout(c, N=None):
    """how a forward case stores W, b and Y: one group - W rows (k-major: its K rows) padded to 16 bytes plus ldw_pad floats, Y rows
    3 floats longer than N; groups - [W | b] of each group packed back to back in one flat buffer, Y the column blocks of one tensor"""
    N = c.N if N is None else N
    if c.groups > 1:
        per = N * c.K + N
        return NS(ldw=c.K, gs_w=per, gs_b=per, ldy=c.groups * N, gs_y=N)
    return NS(ldw=ceil4(N if c.kmajor else c.K) + c.ldw_pad, gs_w=0, gs_b=0, ldy=N + 3, gs_y=0)


def lin_sweep_plan(M, N, k0):
    """what the sweep M x N x K0 (aligned dense input, row-major W, fp32) is picked for"""
    nc = 5 if 64 < N <= 80 else 4
    return ("element" if k0 < 16 else "vector", nc, ((M + 127) // 128, (N + 16 * nc - 1) // (16 * nc), 1))


# ================================================================================================ cases: marl_linear_wgrad
def wg(name, M, N, s, plan, gate=False, goff=0, groups=1, bf16=False, tall=1, db=True, dw_extra=0, covers=""):
    """plan: (family, (instantiation), passes, slabs).  gate: Yact given.  goff: dY's base off the 16-byte grid (floats).  tall: the
    wgrad_tall switch the case runs under.  dw_extra: dW is a column block of a tensor that many columns wider on each side."""
    return NS(name=name, M=M, N=N, src=s, K=width(s), plan=plan, gate=gate, goff=goff, groups=groups, bf16=bf16, tall=tall, db=db,
              dw_extra=dw_extra, covers=covers)


def _learner_src(B, T, N, O, A, t0=1, uoff=-1):
    """[obs | one-hot(last action) | id] as the learner builds it: (T+1)-slot observation storage, the action shifted by one step"""
    return src(k0=O, nhot=1, hot_w=A, nid=N, remap0=(T * N, (T + 1) * N, t0 * N), remapi=(T * N, T * N, uoff * N))


def _wg_cases():
    c = []
    gen = lambda bf=0: ("generic", (bf, 0), 1)
    # ---- generic 64 x 64-block kernel
    for M, slabs in ((1, 1), (63, 1), (64, 1), (65, 1), (960, 1), (961, 2), (1023, 2), (1024, 2), (1025, 2)):
        c.append(wg("gen-M%d" % M, M, 5, src(k0=63), gen() + (slabs,), covers="reduce over %d slab%s" % (slabs, "s" * (slabs > 1))))
    for N in (5, 64, 65, 130):
        for K in (62, 63, 64):
            c.append(wg("gen-N%d-K%d" % (N, K), 65, N, src(k0=K), gen() + (1,)))
    c.append(wg("gen-dy-misaligned", 130, 64, src(k0=64), gen() + (1,), goff=1))
    c.append(wg("gen-x-gated", 100, 33, src(k0=20, gate=True), gen() + (1,)))
    c.append(wg("gen-concat", 75, 13, src(k0=20, k1=9, nhot=3, hot_w=4, nid=5, remap0=(15, 18, -2), emap=True), gen() + (1,), gate=True))
    c.append(wg("gen-groups-gate", 75, 6, src(k0=40), gen() + (1,), gate=True, groups=4))
    c.append(wg("gen-bf16", 300, 70, src(k0=33), gen(1) + (1,), bf16=True))
    c.append(wg("gen-bf16-tall-shape", 4100, 64, src(k0=64), gen(1) + (8,), bf16=True))
    # ---- full-width kernel: M >= 2048, N <= 80, K + 1 <= 80
    c.append(wg("full-M2047-generic", 2047, 80, src(k0=79), gen() + (4,)))
    c.append(wg("full-M2048", 2048, 80, src(k0=79), ("full", (0, 0), 1, 8)))
    c.append(wg("full-M2049-gate", 2049, 80, src(k0=79), ("full", (1, 0), 1, 8), gate=True))
    c.append(wg("full-78-onehot-gate", 2100, 78, src(k0=64, nhot=1, hot_w=14), ("full", (1, 0), 1, 8), gate=True))
    c.append(wg("full-78-onehot", 2100, 78, src(k0=64, nhot=1, hot_w=14), ("full", (0, 0), 1, 8)))
    c.append(wg("full-33x25-gate", 2100, 33, src(k0=20, nhot=1, hot_w=5), ("full", (1, 0), 1, 8), gate=True))
    c.append(wg("full-33x25", 2100, 33, src(k0=20, nhot=1, hot_w=5), ("full", (0, 0), 1, 8)))
    c.append(wg("full-two-dense", 2100, 33, src(k0=8, k1=12), ("full", (0, 0), 1, 8)))
    c.append(wg("full-N81-generic", 2048, 81, src(k0=79), gen() + (4,)))
    c.append(wg("full-K80-generic", 2048, 80, src(k0=80), gen() + (4,)))
    c.append(wg("full-straddle-generic", 2100, 33, src(k0=6, k1=9), gen() + (4,)))
    c.append(wg("full-nid-generic", 2100, 33, src(k0=20, nid=5), gen() + (4,)))
    # ---- thin one-column kernel: N == 1, M >= 4096, K <= 252
    c.append(wg("thin-M4095-generic", 4095, 1, src(k0=30), gen() + (8,)))
    c.append(wg("thin-M4096", 4096, 1, src(k0=30), ("thin", (0, 0), 1, 8)))
    c.append(wg("thin-M9001", 9001, 1, src(k0=30), ("thin", (0, 0), 1, 17), covers="reduce over 17 slabs"))
    c.append(wg("thin-M8128", 8128, 1, src(k0=4), ("thin", (0, 0), 1, 15), covers="reduce over 15 slabs"))
    c.append(wg("thin-M8129", 8129, 1, src(k0=4), ("thin", (0, 0), 1, 16), covers="reduce over 16 slabs"))
    for K in (1, 4, 132, 252):
        c.append(wg("thin-K%d" % K, 4096, 1, src(k0=K), ("thin", (0, 0), 1, 8)))
    c.append(wg("thin-K253-generic", 4096, 1, src(k0=253), gen() + (8,)))
    # ---- LDS-staged tall kernel: N == 64, M >= 4096, 16 <= k0 <= 224
    for M in (4096, 4097, 4127):
        c.append(wg("tall-M%d" % M, M, 64, src(k0=16), ("tall", (6, 3), 1, 8)))
    c.append(wg("tall-K96", 4100, 64, src(k0=96), ("tall", (6, 3), 1, 8)))
    c.append(wg("tall-K97", 4100, 64, src(k0=97), ("tall", (10, 5), 1, 8)))
    c.append(wg("tall-K160", 4100, 64, src(k0=160), ("tall", (10, 5), 1, 8)))
    c.append(wg("tall-K192+7+5", 4100, 64, src(k0=192, nhot=1, hot_w=7, nid=5), ("tall", (14, 6), 1, 8)))
    c.append(wg("tall-K196", 4100, 64, src(k0=196), ("tall", (14, 7), 1, 8)))
    c.append(wg("tall-K224", 4100, 64, src(k0=224), ("tall", (14, 7), 1, 8)))
    c.append(wg("tall-ragged-K30", 4100, 64, src(k0=30), ("tall", (6, 3), 1, 8)))
    c.append(wg("tall-learner", 17 * 50 * 5, 64, _learner_src(17, 50, 5, 24, 7), ("tall", (6, 3), 1, 8)))
    c.append(wg("tall-negative-rows", 4200, 64, src(k0=24, nhot=1, hot_w=7, nid=5, remap0=(50, 55, -3), remapi=(50, 50, -5), emap=True),
                ("tall", (6, 3), 1, 8)))
    c.append(wg("tall-M131008", 131008, 64, src(k0=16), ("tall", (6, 3), 1, 255), covers="reduce over 255 slabs"))
    c.append(wg("tall-M131009", 131009, 64, src(k0=16), ("tall", (6, 3), 1, 512), covers="reduce over 256 slabs launched as 512"))
    c.append(wg("tall-M140000-K224", 140000, 64, src(k0=224), ("tall", (14, 7), 1, 512), covers="the largest shape"))
    # ---- direct kernel: what production runs with the tall kernel switched off ...
    for K in (16, 32, 48, 64, 80):
        c.append(wg("direct-0-%d" % (K // 16), 4100, 64, src(k0=K, off0=1), ("direct", (0, K // 16), 1, 8), tall=0))
    for K in (64, 80, 96, 112, 128):
        s = src(k0=64, nhot=1 if K > 64 else 0, hot_w=K - 64 if K > 64 else 0)
        c.append(wg("direct-1-%d" % ((K - 64) // 16), 4100, 64, s, ("direct", (1, (K - 64) // 16), 1, 8), tall=0))
    c.append(wg("direct-learner-off", 17 * 50 * 5, 64, _learner_src(17, 50, 5, 64, 7), ("direct", (1, 1), 1, 8), tall=0))
    # ... and what the tall kernel declines with the switch on: two one-hot blocks, a source off the 16-byte grid
    c.append(wg("direct-nhot2", 4100, 64, src(k0=16, nhot=2, hot_w=8), ("direct", (0, 2), 1, 8)))
    c.append(wg("direct-xvec0", 4100, 64, src(k0=32, off0=1), ("direct", (0, 2), 1, 8)))
    c.append(wg("direct-M9001-ragged", 9001, 64, src(k0=70, nid=5), ("direct", (1, 1), 1, 17)))
    # ---- direct kernel in column passes
    for tall in (1, 0):
        sw = "on" if tall else "off"
        c.append(wg("passes-K130-%s" % sw, 4100, 64, src(k0=66, nhot=2, hot_w=32), ("passes", (1, 5), 2, 8), tall=tall, db=bool(tall),
                    dw_extra=0 if tall else 3))
        c.append(wg("passes-K135-%s" % sw, 4100, 64, src(k0=130, nid=5), ("passes", (1, 1), 3, 8), tall=tall, db=not tall,
                    dw_extra=3 if tall else 0))
    c.append(wg("passes-M9001", 9001, 64, src(k0=130, nid=5), ("passes", (1, 1), 3, 17), dw_extra=5))
    return c


WG_CASES = _wg_cases()


def wg_layout(c):
    """how a weight-gradient case stores dY / Yact (rows padded to 16 bytes, base goff floats off the grid) and dW / db (one group: a
    column block of a tensor dw_extra columns wider on each side; groups: [dW | db] packed back to back in one flat buffer)"""
    cols = c.N * c.groups
    if c.groups > 1:
        per = c.N * c.K + c.N
        return NS(ldg=ceil4(cols), lddw=c.K, gs_w=per, gs_b=per, gs_y=c.N)
    return NS(ldg=1 if cols == 1 else ceil4(cols), lddw=c.K + 2 * c.dw_extra, gs_w=0, gs_b=0, gs_y=0)      # (one column: contiguous)

# what the table must reach (tests/test_dense_oracle_cpu.py sweeps it): every instantiation of every weight-gradient kernel ...
WG_INSTANCES = ([("generic", (0, 0)), ("generic", (1, 0)), ("full", (0, 0)), ("full", (1, 0)), ("thin", (0, 0))] +
                [("direct", (0, n)) for n in (1, 2, 3, 4, 5)] + [("direct", (1, n)) for n in (0, 1, 2, 3, 4)] +
                [("tall", t) for t in ((6, 3), (10, 5), (14, 6), (14, 7))] + [("passes", (1, 1)), ("passes", (1, 5))])
# ... and the slab counts either side of the reduce kernel's 16 slab groups
REDUCE_SLABS = (1, 2, 8, 15, 16, 17, 255, 512)


def case_seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31)


def wg_inputs(c, kind, slabs=None):
    """every operand of a weight-gradient case and its float64 result: NS(src data, X, dY, Yact, rows, base_w, base_b, dW, db, mag...)"""
    rng = np.random.default_rng(case_seed(c.name + kind))
    d = make_src(c.src, c.M, rng, "exact" if kind == "exact" else "real")
    X = virtual_x(c.src, d, c.M)
    cols = c.N * c.groups
    rows = None
    if kind == "probe":
        ep = c.src.remap0[0] if c.src.remap0 else (c.src.remapi[0] if c.src.remapi else None)
        rows = probe_rows(c.plan[0], c.M, c.plan[3] if slabs is None else slabs, ep)
    dY = make_dy(c.M, cols, rng, kind, rows)
    Yact = _gate_values(rng, (c.M, cols), "exact" if kind == "exact" else "real") if c.gate else None
    if kind == "exact":
        base_w = rng.integers(-3, 4, size=(c.groups, c.N, c.K)).astype(F32)
        base_b = rng.integers(-3, 4, size=(c.groups, c.N)).astype(F32)
    elif kind == "probe":
        base_w, base_b = np.zeros((c.groups, c.N, c.K), F32), np.zeros((c.groups, c.N), F32)
    else:
        base_w = rng.standard_normal((c.groups, c.N, c.K)).astype(F32)
        base_b = rng.standard_normal((c.groups, c.N)).astype(F32)
    Xr, Gr = (bf16_round(X.astype(F32)), bf16_round(dY)) if c.bf16 else (X, dY)
    dW, db = wgrad(Gr, Yact, Xr, c.groups)
    dW, db = dW.reshape(c.groups, c.N, c.K), db.reshape(c.groups, c.N)
    return NS(d=d, X=X, Xr=Xr, dY=dY, Gr=Gr, Yact=Yact, rows=rows, base_w=base_w, base_b=base_b, dW=dW, db=db)


def lin_inputs(c, kind, M=None, N=None):
    """every operand of a forward case and its float64 result; W is [groups, N, K] whatever the layout it is stored in"""
    M, N = c.M if M is None else M, c.N if N is None else N
    rng = np.random.default_rng(case_seed(c.name + kind) + 7 * M + N)
    d = make_src(c.src, M, rng, kind)
    X = virtual_x(c.src, d, M)
    W = _values(rng, (c.groups, N, c.K), kind)
    if kind == "real":
        W *= F32(0.3)
    b = _values(rng, (c.groups, N), kind) if c.bias else None
    Y0 = _values(rng, (M, c.groups * N), kind)
    Xr, Wr = (bf16_round(X.astype(F32)).astype(F64), bf16_round(W)) if c.bf16 else (X, W)
    Y = np.concatenate([linear(Xr, Wr[g], None if b is None else b[g], c.act, c.beta, Y0[:, g * N:(g + 1) * N]) for g in range(c.groups)], 1)
    mag = np.concatenate([linear_mag(Xr, Wr[g], None if b is None else b[g], c.beta, Y0[:, g * N:(g + 1) * N]) for g in range(c.groups)], 1)
    return NS(d=d, X=X, W=W, b=b, Y0=Y0, Y=Y, mag=mag)
