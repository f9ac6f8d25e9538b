"""Float64 statement of the fused QTRAN heads, the state-row kernels and the row-level weight gradients of csrc/qtran_fused.hip
(marl_qtran_head_fwd / _fwd2 / _bwd, marl_qtran_state_parts, marl_qmix_tail_fwd, marl_qtran_wgrad_rows) and the table of cases
that tests/test_gpu_qtran.py runs and tests/test_qtran_oracle_cpu.py holds to the library's own plan query (marl_qtran_plan).
Plain numpy, no autograd: nothing here imports marl_amd or torch.

The operations (reference network/mixer.py:355-418; the comment at the top of qtran_fused.hip):
  x_i  = [h_i | onehot(u_i)]      u outside [0, A): the all-zero one-hot          e1_i = W_e1 x_i + b_e1
  s1   = sum_i relu(e1_i)         e2 = W_e2 s1 + N b_e2                           sp   = W_q1[:, :S] s + b_q1
  y1   = relu(sp + W_q1[:, S:] e2)   y2 = relu(W_q2 y1 + b_q2)                    out  = w_q3 . y2 + b_q3
backward from d_out, the relu gradient at a pre-activation of exactly 0 being 0.

Three kinds of data:
  exact   small integers, sparse: every intermediate and every sum of |terms| of every gradient stays below 2^24, so fp32 in any
          summation order and float64 give THE SAME BITS.  Pre-activations of exactly 0 are frequent: they pin the `> 0` gate.
          At large BT the rows with d_out != 0 are the seam rows and a few more (the gradient sums stay small).
  probe   heads: exact data on the seam rows only - every other row has h = 0, no action and d_out = 0; row kernels: real-valued
          data, the row gradients (state parts: the states) exactly zero but on the seam rows - every element that is zero in the
          reference must be exactly zero, the others are held to (nnz + 3) u sum |terms|
  real    Gaussian data at the scales of the older tests (nn.Linear's default initialisation, h ~ 0.7 N(0, 1), s ~ N(0, 1)) but for
          the layers behind the agent sum: the running error bound grows by || |W| || per layer (4 to 5 at the default scale, which
          puts 10 to 50 % of the rows within their own bound of a relu kink), so W_e2, W_q1[:, S:] and W_q2 are a quarter of the
          default and b_e1, b_q2 are N(0, 1) - the kink cap of 2 % of the rows then holds (REAL_SALT: the cases whose seed moved)
"""
import functools
import types

import numpy as np

NS = types.SimpleNamespace
U = 2.0 ** -24
F32, F64 = np.float32, np.float64
HD = 64
LIMIT = 2.0 ** 24
KINK_CAP = 0.02
WNAMES = ("enc0_w", "enc0_b", "enc2_w", "enc2_b", "q0_w", "q0_b", "q2_w", "q2_b", "q4_w", "q4_b")


def case_seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31)


# ================================================================================================ the operations
def onehot(u, A):
    """(R, A) one-hot of u; every value outside [0, A) is the all-zero row"""
    u = np.asarray(u).reshape(-1)
    oh = np.zeros((u.size, A))
    ok = (u >= 0) & (u < A)
    oh[np.flatnonzero(ok), u[ok]] = 1.0
    return oh


def state_part(W, b, s, S):
    return np.asarray(s, F64) @ np.asarray(W, F64)[:, :S].T + np.asarray(b, F64)


def forward(w, h, u, sp, BT, N, A, bound=False, err_sp=None):
    """every forward value in float64: NS(x, e1, s1, e2, y1p, y1, y2p, y2, out).  w: NS of WNAMES (q0_w is [64, S + AE]); h (BT*N, 64);
    u (BT*N) or None (A = 0); sp (BT, 64).  bound: also the running error bound of each value, err_* (see `lin_err`)"""
    W = NS(**{k: np.asarray(getattr(w, k), F64) for k in WNAMES})
    AE = HD + A
    S = W.q0_w.shape[1] - AE
    h = np.asarray(h, F64)
    x = np.concatenate([h, onehot(u, A)], 1) if A else h
    e1 = x @ W.enc0_w.T + W.enc0_b
    r1 = np.maximum(e1, 0.0)
    s1 = r1.reshape(BT, N, AE).sum(1)
    e2 = s1 @ W.enc2_w.T + N * W.enc2_b
    sp = np.asarray(sp, F64)
    y1p = sp + e2 @ W.q0_w[:, S:].T
    y1 = np.maximum(y1p, 0.0)
    y2p = y1 @ W.q2_w.T + W.q2_b
    y2 = np.maximum(y2p, 0.0)
    out = y2 @ W.q4_w.reshape(-1) + W.q4_b.reshape(())
    f = NS(x=x, e1=e1, s1=s1, e2=e2, y1p=y1p, y1=y1, y2p=y2p, y2=y2, out=out, S=S, AE=AE)
    if bound:
        # terms of e1: the 64 hidden columns and one one-hot column
        f.err_e1 = lin_err(np.zeros_like(x), x, W.enc0_w, W.enc0_b, HD + 1)
        f.err_s1 = f.err_e1.reshape(BT, N, AE).sum(1) + (N + 1) * U * np.abs(r1).reshape(BT, N, AE).sum(1)
        f.err_e2 = lin_err(f.err_s1, s1, W.enc2_w, N * W.enc2_b, AE)
        f.err_y1 = lin_err(f.err_e2, e2, W.q0_w[:, S:], sp, AE, err_b=err_sp)
        f.err_y2 = lin_err(f.err_y1, y1, W.q2_w, W.q2_b, HD)
        f.err_out = lin_err(f.err_y2, y2, W.q4_w.reshape(1, -1), W.q4_b.reshape(1), HD)[:, 0]
    return f


def lin_err(err_x, x, W, b, K, err_b=None):
    """the running error bound of y = W x + b computed in fp32 in any order from an x that is itself off by err_x:
    err_y = |W| err_x + (K + 3) u (|W||x| + |b|), K the terms of a row that can be nonzero (gamma_K ~ K u of a K-term sum, + 3 for the
    bias add, the table / N b multiply and the rounding of the stored result); relu passes a bound through (|relu a - relu b| <= |a - b|)"""
    aW = np.abs(W)
    e = err_x @ aW.T + (K + 3) * U * (np.abs(x) @ aW.T + np.abs(b))
    return e if err_b is None else e + err_b


def dual_err_e1(f1, f2):
    """the second action set of marl_qtran_head_fwd2: its pre-activation is formed as fl(e1 of the first set) + fl(table row 2 - table
    row 1), so it carries the first set's error, the rounding of both table rows and of the sum: bounded by the sum of both bounds"""
    return f1.err_e1 + f2.err_e1


def forward2(w, h, u, u2, sp, BT, N, A):
    """(first set with bounds, second set with bounds) of marl_qtran_head_fwd2"""
    f1 = forward(w, h, u, sp, BT, N, A, bound=True)
    f2 = forward(w, h, u2, sp, BT, N, A, bound=True)
    W = NS(**{k: np.asarray(getattr(w, k), F64) for k in WNAMES})
    AE, S = f2.AE, f2.S
    f2.err_e1 = dual_err_e1(f1, f2)
    r1 = np.maximum(f2.e1, 0.0)
    f2.err_s1 = f2.err_e1.reshape(BT, N, AE).sum(1) + (N + 1) * U * np.abs(r1).reshape(BT, N, AE).sum(1)
    f2.err_e2 = lin_err(f2.err_s1, f2.s1, W.enc2_w, N * W.enc2_b, AE)
    f2.err_y1 = lin_err(f2.err_e2, f2.e2, W.q0_w[:, S:], sp, AE)
    f2.err_y2 = lin_err(f2.err_y1, f2.y1, W.q2_w, W.q2_b, HD)
    f2.err_out = lin_err(f2.err_y2, f2.y2, W.q4_w.reshape(1, -1), W.q4_b.reshape(1), HD)[:, 0]
    return f1, f2


def backward(w, f, s, d_out, BT, N, A, mags=False):
    """every backward value and parameter gradient in float64 from the forward values f.  s (BT, S) the states (for d_q0_w).
    mags: the same sums over |terms| (what an exact case must keep below 2^24) in NS .mag"""
    W = NS(**{k: np.asarray(getattr(w, k), F64) for k in WNAMES})
    AE, S = f.AE, f.S
    d = np.asarray(d_out, F64)
    g = NS()
    g.dy2 = np.where(f.y2p > 0, d[:, None] * W.q4_w.reshape(1, -1), 0.0)
    g.dy1 = np.where(f.y1p > 0, g.dy2 @ W.q2_w, 0.0)
    g.de2 = g.dy1 @ W.q0_w[:, S:]
    g.ds1 = g.de2 @ W.enc2_w
    g.de1 = np.where(f.e1 > 0, np.repeat(g.ds1, N, axis=0), 0.0)
    g.dhidden = g.de1 @ W.enc0_w[:, :HD]
    se = np.concatenate([np.asarray(s, F64), f.e2], 1)
    g.enc0_w, g.enc0_b = g.de1.T @ f.x, g.de1.sum(0)
    g.enc2_w, g.enc2_b = g.de2.T @ f.s1, N * g.de2.sum(0)
    g.q0_w, g.q0_b = g.dy1.T @ se, g.dy1.sum(0)
    g.q2_w, g.q2_b = g.dy2.T @ f.y1, g.dy2.sum(0)
    g.q4_w, g.q4_b = (d @ f.y2).reshape(1, -1), d.sum().reshape(1)
    if mags:
        a = np.abs
        m = g.mag = NS()
        m.dy1 = a(g.dy2) @ a(W.q2_w)
        m.de2 = a(g.dy1) @ a(W.q0_w[:, S:])
        m.ds1 = a(g.de2) @ a(W.enc2_w)
        m.dhidden = a(g.de1) @ a(W.enc0_w[:, :HD])
        m.enc0_w, m.enc0_b = a(g.de1).T @ a(f.x), a(g.de1).sum(0)
        m.enc2_w, m.enc2_b = a(g.de2).T @ a(f.s1), N * a(g.de2).sum(0)
        m.q0_w, m.q0_b = a(g.dy1).T @ a(se), a(g.dy1).sum(0)
        m.q2_w, m.q2_b = a(g.dy2).T @ a(f.y1), a(g.dy2).sum(0)
        m.q4_w, m.q4_b = (a(d) @ a(f.y2)).reshape(1, -1), a(d).sum().reshape(1)
    return g


def forward_mags(w, f, sp, N):
    """sums over |terms| of every forward value (exact cases: all below 2^24)"""
    a = np.abs
    W = NS(**{k: np.asarray(getattr(w, k), F64) for k in WNAMES})
    BT = f.s1.shape[0]
    m = NS()
    m.e1 = a(f.x) @ a(W.enc0_w).T + a(W.enc0_b)
    m.s1 = np.maximum(m.e1, 0).reshape(BT, N, f.AE).sum(1)
    m.e2 = m.s1 @ a(W.enc2_w).T + N * a(W.enc2_b)
    m.y1 = a(np.asarray(sp, F64)) + m.e2 @ a(W.q0_w[:, f.S:]).T
    m.y2 = m.y1 @ a(W.q2_w).T + a(W.q2_b)
    m.out = m.y2 @ a(W.q4_w).reshape(-1) + a(W.q4_b).reshape(())
    return m


def kink_rows(f, f2=None):
    """rows (of BT) with a pre-activation - e1 of any agent, y1, y2 - smaller in magnitude than its own running error bound: two
    correct fp32 evaluations may gate it differently, so the gradient of that row is not defined to fp32 accuracy"""
    BT = f.s1.shape[0]
    k = (np.abs(f.e1) < f.err_e1).reshape(BT, -1).any(1) | (np.abs(f.y1p) < f.err_y1).any(1) | (np.abs(f.y2p) < f.err_y2).any(1)
    return k


def row_grads(s, s1, e2, y1, y2, d_out, dy1, dy2, de2, AE):
    """marl_qtran_wgrad_rows on given row tensors (s1, e2, de2 [BT, AEP]: columns AE.. are not part of any product):
    NS(q0_w [64, S + AE], q0_b, q2_w, q2_b, q4_w [64], q4_b [1], enc2_w [AE, AE]), and .mag / .nnz: sum |terms| and nonzero terms"""
    c = lambda t: np.asarray(t, F64)
    se = np.concatenate([c(s), c(e2)[:, :AE]], 1)
    d = c(d_out)
    pairs = dict(q0_w=(c(dy1), se), q2_w=(c(dy2), c(y1)), q4_w=(d[:, None], c(y2)), enc2_w=(c(de2)[:, :AE], c(s1)[:, :AE]),
                 q0_b=(c(dy1), None), q2_b=(c(dy2), None), q4_b=(d[:, None], None))
    g = NS(mag=NS(), nnz=NS())
    for k, (G, X) in pairs.items():
        if X is None:
            v, m, n = G.sum(0), np.abs(G).sum(0), (G != 0).sum(0).astype(F64)
        else:
            v, m, n = G.T @ X, np.abs(G).T @ np.abs(X), (G != 0).astype(F64).T @ (X != 0).astype(F64)
        if k == "q4_w":
            v, m, n = v.reshape(-1), m.reshape(-1), n.reshape(-1)
        setattr(g, k, v); setattr(g.mag, k, m); setattr(g.nnz, k, n)
    return g


ROW_GRADS = ("q0_w", "q0_b", "q2_w", "q2_b", "q4_w", "q4_b", "enc2_w")
PARAMS = ("enc0_w", "enc0_b", "enc2_w", "enc2_b", "q0_w", "q0_b", "q2_w", "q2_b", "q4_w", "q4_b")


def qmix_tail(Wb1, bb1, Wh, bh, s):
    """(hyper_b1(s), relu(hyper_b2.0(s))) [rows, 32] each, and the sums over |terms|"""
    s = np.asarray(s, F64)
    b1 = s @ np.asarray(Wb1, F64).T + np.asarray(bb1, F64)
    hh = s @ np.asarray(Wh, F64).T + np.asarray(bh, F64)
    m1 = np.abs(s) @ np.abs(np.asarray(Wb1, F64)).T + np.abs(np.asarray(bb1, F64))
    mh = np.abs(s) @ np.abs(np.asarray(Wh, F64)).T + np.abs(np.asarray(bh, F64))
    return b1, np.maximum(hh, 0.0), m1, mh


# ================================================================================================ the older tests' ceilings
def dhidden_ceiling(ref):
    return 2e-5 + 1e-4 * np.abs(ref)


def param_ceiling(ref, R):
    """3e-5 max(1, sqrt(R / 64)) max(1, max |ref|) + 1e-4 |ref| (test_gpu_kernels.py: test_qtran_fused_heads), R the reduced rows"""
    ref = np.abs(np.asarray(ref, F64))
    return 3e-5 * max(1.0, (R / 64.0) ** 0.5) * max(1.0, float(ref.max()) if ref.size else 0.0) + 1e-4 * ref


# ================================================================================================ data
def _ints(rng, shape, lim, zeros):
    v = rng.integers(-lim, lim + 1, size=shape).astype(F32)
    return np.where(rng.random(shape) < zeros, F32(0), v).astype(F32)


def weights(rng, kind, A, S):
    AE = HD + A
    shapes = dict(enc0_w=(AE, AE), enc0_b=(AE,), enc2_w=(AE, AE), enc2_b=(AE,), q0_w=(HD, S + AE), q0_b=(HD,), q2_w=(HD, HD), q2_b=(HD,),
                  q4_w=(1, HD), q4_b=(1,))
    w = NS()
    for k in WNAMES:
        shp = shapes[k]
        if kind == "real":
            fan = shapes[k[:-1] + "w"][1]
            v = rng.uniform(-1.0, 1.0, size=shp).astype(F32) / F32(fan ** 0.5)
            if k in ("enc0_b", "q2_b"):
                v = rng.standard_normal(shp).astype(F32)
            if k in ("enc2_w", "q2_w"):
                v = v * F32(0.25)
            if k == "q0_w":
                v[:, S:] *= F32(0.25)
        else:
            v = _ints(rng, shp, 1, 0.0 if k.endswith("_b") else 0.85)
        setattr(w, k, np.ascontiguousarray(v, dtype=F32))
    return w


def draw_u(rng, n, A):
    """actions from {-1, 0 .. A-1, A .. 15 (A < 16), 16, 1000}: 60 % in [0, A), the rest from the values that must act as no action"""
    other = np.array([-1] + list(range(A, 16)) + [16, 1000], dtype=np.int32)
    u = rng.integers(0, A, size=n).astype(np.int32)
    out = rng.random(n) < 0.4
    u[out] = other[rng.integers(0, other.size, size=int(out.sum()))]
    return u


# ================================================================================================ seams
HEAD_ROUND = 256 * 8 * 16          # rows of one round of the head kernels: 256 workgroups x 8 waves x 16-row tiles
SP_BLOCK, SP_CAP = 64, 256
WG_BLOCK, WG_CAP = 32, 256


def _pick(rows, BT):
    return np.array(sorted({int(r) for r in rows if 0 <= r < BT}), dtype=np.int64)


def head_seams(BT):
    """first / last row of a tile, of a round and of the batch"""
    at = [0, 15, 16, BT - 1, (BT - 1) // 16 * 16, (BT - 1) // 16 * 16 - 1]
    for k in range(1, (BT + HEAD_ROUND - 1) // HEAD_ROUND + 1):
        at += [k * HEAD_ROUND - 16, k * HEAD_ROUND - 1, k * HEAD_ROUND, k * HEAD_ROUND + 15]
    return _pick(at, BT)


def sp_seams(BT, grid):
    """first / last row of a 16-row tile and a 64-row block, of a workgroup's rounds (block b runs in round b // grid) and of the batch"""
    at = [0, 15, 16, 63, 64, BT - 1, (BT - 1) // 64 * 64, (BT - 1) // 64 * 64 - 1]
    nblk = (BT + 63) // 64
    for k in range(1, (nblk + grid - 1) // grid + 1):
        at += [k * grid * 64 - 1, k * grid * 64]
    return _pick(at, BT)


def wg_seams(BT, grid):
    """first / last row of a 16-row chunk and a 32-row block, of the last slab (workgroup grid - 1), of a round and of the batch"""
    at = [0, 15, 16, 31, 32, BT - 1, (BT - 1) // 32 * 32, (BT - 1) // 32 * 32 - 1, 32 * (grid - 1), 32 * grid - 1]
    nblk = (BT + 31) // 32
    for k in range(1, (nblk + grid - 1) // grid + 1):
        at += [k * grid * 32 - 1, k * grid * 32]
    return _pick(at, BT)


# ================================================================================================ cases: heads
HEAD_BT_SMALL = (1, 15, 16, 17, 128, 129)
HEAD_BT_LARGE = (32768, 32769, 32768 + 2048 * 16 + 5)
HEAD_KINDS = (("q", 1), ("q", 3), ("q", 16), ("v", 0))
HEAD_S = 8          # width of the state block of q.0 in the head cases (the head kernels read only its column offset)


def head_case(head, A, N, BT):
    return NS(name="%s-A%d-N%d-BT%d" % (head, A, N, BT), head=head, A=A, N=N, BT=BT, AE=HD + A, S=HEAD_S)


def _head_cases():
    out = []
    for head, A in HEAD_KINDS:
        for BT in HEAD_BT_SMALL:
            for N in (1, 2, 3, 4):
                out.append(head_case(head, A, N, BT))
        for BT in HEAD_BT_LARGE:
            for N in (1, 2):
                out.append(head_case(head, A, N, BT))
    return out


HEAD_CASES = _head_cases()


def head_plan(c, what):
    """(FT, hot, dual, grid, rounds, slabs) the case is picked for"""
    tiles = (c.BT + 15) // 16
    grid = min(256, (tiles + 7) // 8)
    rounds = (tiles + 8 * grid - 1) // (8 * grid)
    return (5 if c.A else 4, c.A > 0, what == "fwd2", grid, rounds, grid if what == "bwd" else 0)


def head_kinds(c):
    return ("exact", "probe", "real") if c.BT > 4096 else ("exact", "real")


# real data: the cases whose first seed put more than 2 % of the rows (at these sizes: a single row) on a relu kink
REAL_SALT = {"q-A1-N4-BT15": 2, "q-A1-N3-BT17": 2, "q-A1-N2-BT128": 1, "q-A1-N3-BT129": 2, "q-A3-N2-BT15": 1, "q-A3-N2-BT16": 1,
             "q-A3-N4-BT129": 1, "q-A16-N4-BT1": 1, "q-A16-N1-BT15": 1, "q-A16-N2-BT15": 1, "q-A16-N4-BT15": 3, "q-A16-N3-BT16": 1,
             "q-A16-N2-BT17": 2, "v-A0-N4-BT17": 1, "seam-q": 1, "seam-v": 1}


@functools.lru_cache(maxsize=2)
def head_inputs(name, kind):
    """every operand of a head case and its float64 results: NS(w, h, u, u2, sp, d_out, rows, f, f2, g, kink, kink2).  Real data: d_out
    is zero on the kink rows.  Treat as read-only (shared between tests)."""
    c = {x.name: x for x in HEAD_CASES + SEAM_CASES}[name]
    rng = np.random.default_rng(case_seed(name + kind) + (REAL_SALT.get(name, 0) if kind == "real" else 0))
    BT, N, A = c.BT, c.N, c.A
    R = BT * N
    real = kind == "real"
    w = weights(rng, "real" if real else "exact", A, c.S)
    seam = head_seams(BT)
    if real:
        h = (rng.standard_normal((R, HD)) * 0.7).astype(F32)
        sp = rng.standard_normal((BT, HD)).astype(F32)
        d_out = rng.standard_normal(BT).astype(F32)
        rows = np.arange(BT)
    else:
        h = _ints(rng, (R, HD), 2, 0.7)
        sp = _ints(rng, (BT, HD), 3, 0.3)
        # the rows with a gradient: all of a small batch; the seam rows and 64 more of a large one (probe: the seam rows alone)
        rows = np.arange(BT) if BT <= 129 else _pick(list(seam) + ([] if kind == "probe" else list(rng.integers(0, BT, size=64))), BT)
        d_out = np.zeros(BT, dtype=F32)
        d_out[rows] = rng.integers(1, 3, size=rows.size) * rng.choice([-1, 1], size=rows.size)
    u = draw_u(rng, R, A) if A else None
    u2 = draw_u(rng, R, A) if A else None
    if kind == "probe":
        off = np.ones(BT, dtype=bool)
        off[rows] = False
        h.reshape(BT, N, HD)[off] = 0
        if A:
            u.reshape(BT, N)[off] = -1
            u2.reshape(BT, N)[off] = -1
    i = NS(c=c, w=w, h=h, u=u, u2=u2, sp=sp, rows=rows, kink=None, kink2=None, f2=None)
    if A:
        i.f, i.f2 = forward2(w, h, u, u2, sp, BT, N, A)
    else:
        i.f = forward(w, h, None, sp, BT, N, A, bound=True)
    if real:
        i.kink = kink_rows(i.f)
        d_out[i.kink] = 0
        if A:
            i.kink2 = kink_rows(i.f2)
    i.d_out = d_out
    i.s = _ints(rng, (BT, c.S), 2, 0.5) if not real else rng.standard_normal((BT, c.S)).astype(F32)
    i.g = backward(w, i.f, i.s, d_out, BT, N, A, mags=not real)
    return i


# ================================================================================================ cases: state parts and the QMIX tail
SP_S = (1, 4, 64, 65, 128, 129, 192, 193, 224, 225, 256, 257, 320, 321, 384)
SP_BT = (1, 63, 64, 65, 16384, 16385, 16384 + 64 * 3 + 1)
SP_BUCKETS = (4, 8, 12, 14, 16, 20, 24)
SP_REMAP_BT = (65, 16384 + 64 * 3 + 1)          # the (T+1)-slot storage read through an episode map, at one small and one large batch
SP_T = 13


def sp_plan(BT, S, nsets):
    """(KCT, nsets, grid, rounds)"""
    kc = (S + 15) // 16
    kct = next(b for b in SP_BUCKETS if kc <= b)
    nblk = (BT + 63) // 64
    r = (nblk + SP_CAP - 1) // SP_CAP
    grid = (nblk + r - 1) // r
    return (kct, nsets, grid, (nblk + grid - 1) // grid)


def sp_kinds(BT):
    return ("exact", "probe", "real") if BT > 4096 else ("exact", "real")


def sp_inputs(S, BT, kind, nsets, remap=False, outs=64):
    """states [BT, S] (remap: in (T+1)-slot storage [episodes + 3, T + 1, S] read from slot 1 on through an episode map that never names
    storage episode 0, which holds NaN), `nsets` weight sets ([outs, S + 5]: the kernel reads the first S columns of wider rows) and the
    float64 results with their sums over |terms|"""
    rng = np.random.default_rng(case_seed("sp-%d-%d-%s-%d-%d" % (S, BT, kind, nsets, remap)))
    grid = sp_plan(BT, S, nsets)[2]
    if kind == "exact":
        s = _ints(rng, (BT, S), 4, 0.4)
    else:
        s = rng.standard_normal((BT, S)).astype(F32)
        if kind == "probe":
            keep = sp_seams(BT, grid)
            z = np.zeros_like(s)
            z[keep] = s[keep]
            s = z
    i = NS(s=s, store=None, emap=None, T=SP_T, rows=sp_seams(BT, grid))
    if remap:
        T = SP_T
        E = (BT + T - 1) // T          # (the last episode may be read in part)
        i.emap = (1 + rng.permutation(E + 2)[:E]).astype(np.int32)
        i.store = (rng.standard_normal((E + 3, T + 1, S)).astype(F32) if kind != "exact" else _ints(rng, (E + 3, T + 1, S), 4, 0.4))
        i.store[0] = np.nan
        full = i.store[i.emap, 1:].reshape(E * T, S)
        full[:BT] = s
        i.store[i.emap, 1:] = full.reshape(E, T, S)
    i.W, i.b, i.ref, i.mag = [], [], [], []
    for k in range(nsets):
        if kind == "exact":
            W, b = _ints(rng, (outs, S + 5), 2, 0.3), _ints(rng, (outs,), 3, 0.2)
        else:
            W = (rng.uniform(-1, 1, size=(outs, S + 5)) / (S + 64) ** 0.5).astype(F32)
            b = rng.uniform(-0.1, 0.1, size=outs).astype(F32)
        i.W.append(W); i.b.append(b)
        i.ref.append(state_part(W, b, s, S))
        i.mag.append(np.abs(s.astype(F64)) @ np.abs(W.astype(F64))[:, :S].T + np.abs(b.astype(F64)))
    return i


def sp_k(S):
    """|got - ref| <= (S + 3) u (sum |s||w| + |b|): an S-term dot product in any order, the bias add, the stored rounding"""
    return S + 3


# ================================================================================================ cases: row-level weight gradients
WG_S = (4, 224, 228, 384)
WG_AE = (64, 80, 65)
WG_BT = (1, 31, 32, 33, 8192, 8193, 8192 + 32 * 5 + 7)


def wg_plan(BT, S, AE):
    """(FT, SMAX, grid, rounds, slabs)"""
    nblk = (BT + 31) // 32
    grid = min(nblk, WG_CAP)
    return ((AE + 15) // 16, 384 if S > 224 else 224, grid, (nblk + grid - 1) // grid, grid)


def wg_kinds(BT):
    return ("exact", "probe", "real") if BT > 4096 else ("exact", "real")


@functools.lru_cache(maxsize=2)
def wg_inputs(S, AE, BT, kind):
    """the nine row tensors of marl_qtran_wgrad_rows as independent data (the kernel only multiplies them), integer bases for the
    gradients to accumulate into, and the float64 results.  The pad columns AE .. AEP of s1 / e2 / de2 hold 3.0: no product may
    reach a gradient from them.  exact: the gradient rows are nonzero on the seam rows and 64 more of a large batch."""
    rng = np.random.default_rng(case_seed("wg-%d-%d-%d-%s" % (S, AE, BT, kind)))
    AEP = (AE + 15) // 16 * 16
    grid = wg_plan(BT, S, AE)[2]
    seam = wg_seams(BT, grid)
    shapes = dict(s=(BT, S), s1=(BT, AEP), e2=(BT, AEP), y1=(BT, HD), y2=(BT, HD), d_out=(BT,), dy1=(BT, HD), dy2=(BT, HD), de2=(BT, AEP))
    i = NS(rows=seam)
    for k, shp in shapes.items():
        v = _ints(rng, shp, 3, 0.5) if kind == "exact" else rng.standard_normal(shp).astype(F32)
        if k in ("d_out", "dy1", "dy2", "de2") and (kind == "probe" or (kind == "exact" and BT > 129)):
            keep = seam if kind == "probe" else _pick(list(seam) + list(rng.integers(0, BT, size=64)), BT)
            z = np.zeros_like(v)
            z[keep] = v[keep]
            v = z
        if k in ("s1", "e2", "de2"):
            v[:, AE:] = 3.0
        setattr(i, k, v)
    i.base = NS()
    bshapes = dict(q0_w=(HD, S + AE), q0_b=(HD,), q2_w=(HD, HD), q2_b=(HD,), q4_w=(HD,), q4_b=(1,), enc2_w=(AE, AE))
    for k, shp in bshapes.items():
        setattr(i.base, k, rng.integers(-3, 4, size=shp).astype(F32) if kind == "exact" else
                (np.zeros(shp, F32) if kind == "probe" else rng.standard_normal(shp).astype(F32)))
    i.g = row_grads(i.s, i.s1, i.e2, i.y1, i.y2, i.d_out, i.dy1, i.dy2, i.de2, AE)
    return i


# ================================================================================================ the module seam and the reach table
SEAM_CASES = [NS(name="seam-q", head="q", A=5, N=3, BT=37, AE=HD + 5, S=20), NS(name="seam-v", head="v", A=0, N=2, BT=37, AE=HD, S=20)]

HEAD_INSTANCES = (("fwd", 5, True, False), ("fwd", 4, False, False), ("fwd2", 5, True, True), ("bwd", 5, True, False), ("bwd", 4, False, False))
WG_INSTANCES = ((4, 224), (5, 224), (4, 384), (5, 384))
