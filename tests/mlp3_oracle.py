"""Float64 statement of the fused 64-wide head kernels (csrc/mlp3_fused.hip: the fp32 pair; csrc/mlp3_x6.hip: the bf16 six-product
split pair; csrc/mlp3_common.h: what they share) and the table of cases that tests/test_gpu_mlp3.py runs and
tests/test_mlp3_oracle_cpu.py holds to the library's own plan query (marl_mlp3_plan).  Plain numpy: nothing here imports marl_amd.
The input rows are the sources of tests/dense_oracle.py (src / make_src / virtual_x: NaN pad columns, remaps, an episode map that
never names storage episode 0, idx = -1).

The operation, per head g:   Y_g = W3_g relu(W2_g relu(W1_g x + b1_g) + b2_g) + b3_g      (two-layer heads: no layer 2)
backward: all six gradients with the relu gate at h > 0, ACCUMULATED into the base contents of the gradient tensors; where the
element stride between the heads' layer-1 tensors is 0 (one wide head evaluated as column blocks) those gradients are summed over
the groups.

Three kinds of data
  exact   small integers with many zeros (x in -4 .. 4, weights and dY from a ladder of ranges / densities, the first rung at which
          the sum of ABSOLUTE values of the terms of every forward value, delta and gradient element - base contents and both
          accumulating runs included - stays below 2^24).  Every partial sum in any order is then an integer below 2^24: fp32, the
          split and float64 give THE SAME BITS, and the comparison is ==.  Pre-activations that are exactly 0 occur (counted in
          `zeros1` / `zeros2`): they tell a `>` gate from a `>=` one.
          The split pair: mlp3_x6.hip writes an fp32 operand as hi + mid + lo, three bf16 terms of 8 significand bits each, rounded
          to nearest one after the other; the sum is the operand exactly.  Of the nine term products it keeps six (mid.mid, hi.lo,
          lo.hi, hi.mid, mid.hi, hi.hi) and drops mid.lo, lo.mid, lo.lo.  An operand of at most 8 significant bits has mid = lo = 0,
          so every dropped product has a zero factor and the six kept ones are the product exactly (each is a product of two 8-bit
          integers scaled by a power of two: exact in fp32).  So a split case also needs ONE operand of every product to have at most
          8 significant bits: x (layer 1 and dW1), W2 (layer 2 and dh1), W3 (layer 3 and dh2), dY (dW3) and dh2 (dW2; the ones column
          of db1 and the bias sums are products with 1).  `x6_exact` checks it.
  probe   real-valued x and weights; dY zero but on a few named rows: first and last, either side of the first 16-row tile seam and
          of the first 64-row iteration seam, of the first and the last stripe seam of every planned launch of the case (forward,
          recomputing, kept and split backward) and of an episode seam of the remap
  real    dense Gaussian data

Error bound on probe and real data: the |W||x| analysis with unit roundoff u = 2^-24 per fp32 accumulation, carried through the
layers.  A sum of n products accumulated in fp32 in ANY order differs from the exact sum by at most k(n) u sum |terms|:
  fp32 pair    k(n) = n + 3          (gamma_n ~ n u; + 3: the bias, the final accumulate into the gradient tensor, the reference's
                                      rounding of fp32-sized values)
  split pair   k = 1.016 (32 + 6 ceil(depth / 32) + 3) + 2.02
               x6.h's mm6 issues, per 32 deep chunk of the sum, six v_mfma_f32_16x16x32_bf16 on one accumulator (mid.mid, hi.lo,
               lo.hi, hi.mid, mid.hi, hi.hi); an instruction is taken as a 32-term dot product summed in fp32 in any order (every
               term meets at most 32 additions there) and one addition to the accumulator: 6 ceil(depth / 32) additions at full size.
               bf16 rounds to nearest with 8 significand bits: |hi| <= (1 + 2^-8) |a|, |mid| <= 2^-8 (1 + 2^-8) |a|, |lo| <= 2^-16 |a|.
               The kept terms' absolute values sum to at most (1 + 2^-7 + 2^-15)^2 < 1.016 of |a||b|; the three dropped products
               to at most 2 . 2^-8 (1 + 2^-8) 2^-16 + 2^-32 < 2.02 u of |a||b|  (test_mlp3_oracle_cpu.py measures both).  depth is the length of the sum as the kernel runs it, zeros included (KV in layer 1; in a gradient an
               instruction whose 32 rows all have dY = 0 adds an exact zero, so 32 x min(rows with dY != 0, ceil(M / 32))).
n is the number of terms that can be nonzero: dense columns + one per one-hot block in layer 1, 64 in the others, the rows with a
nonzero dY (+ the slabs the reduce sums, + the groups of a shared layer) in the gradients.  With e the bound of a layer's input,
  e_out = |W| e_in + k(n) u (|W| (|in| + e_in) + |b|)          forward (relu is 1-Lipschitz)
  E(G^T H) = eG^T |H| + |G|^T eH + eG^T eH + k(n) u (|G| + eG)^T (|H| + eH)          a gradient, G the deltas and H the activations
It is computed from the data of each case - no fixed ceiling.
Kink rows: a row of a head with a pre-activation within its propagated bound of zero may gate differently in two correct evaluations;
its dY for that head is zero on both sides (its outputs are still compared).  At most KINK_CAP = 2 % of a case's (row, head) pairs may
be such rows (checked on the CPU from the reference alone); scales and seeds are chosen so that every case meets it: REAL_SCALE (W1
0.5 / sqrt(terms), W2 0.03, W3 0.2, hidden biases 4: the propagated bound of layer 2 is 64 |W2| times that of layer 1, and wide
biases spread the pre-activations away from zero) and the first of SALTS seeds whose kink rows stay under the cap.
"""
import functools

import numpy as np

from dense_oracle import F32, F64, NS, U, case_seed, make_src, src, terms, virtual_x, width

HD, FNW, NTW, BWD2_KC, XR = 64, 8, 10, 11, 64
CALLS = ("fwd", "bwd", "x6_fwd", "x6_bwd")
KINDS = ("exact", "probe", "real")
KINK_CAP = 0.02
LIMIT = 2.0 ** 24
LDS_MAX = 160 * 1024


# ================================================================================================ the host arithmetic, restated
def kc_bucket(KV):
    kc = (KV + 15) // 16
    return 11 if kc == 11 else (kc + 3) // 4 * 4 if kc <= 12 else 16 if kc <= 16 else (kc + 7) // 8 * 8


def stripes(units, groups, wgs=256):
    n = max(wgs // groups // 8 * 8, 8)
    return max(min(n, units), 1)


def fwd_lds(KC, CF, wide):
    return (4 * KC * 256 + 16 * 256 + (NTW if wide else 1) * 4 * 256 + (16 * NTW if wide else 0)) * 4 + (KC - CF) * 128


def bwd_shape(KC, kept, wide):
    """(two workgroups per CU, KH chunks of x^T per stage pass, passes)"""
    two = kept and not wide and KC <= BWD2_KC
    KH = 16 if KC > 24 else 6 if (two and KC > 8) else KC
    return two, KH, (KC + KH - 1) // KH


def bwd_lds(KC, CF, kept, wide, three):
    _, KH, _ = bwd_shape(KC, kept, wide)
    SF = max(16 * KH + HD, (192 if three else 64) + 16 * (NTW if wide else 1))
    return ((0 if kept else 4 * KC * 256 + 16 * 256) + (16 * 256 if three or not wide else 0) + (NTW * 4 * 256 if wide else 16 * 64) +
            SF * 68) * 4 + (KC - CF) * 128


def vec_rows(s):
    """dense segment 0 takes 16-byte loads: base on the grid, row stride a multiple of 4 floats"""
    return s.off0 % 4 == 0 and s.ld0 % 4 == 0


def supported(c):
    s = c.src
    wide = c.N3 > 16
    if not (1 <= c.N3 <= 16 * NTW) or (wide and (c.nl == 3 or c.N3 % 4)):
        return False
    if s.k0 < 4 or s.gate or s.nid or s.k1 % 4:
        return False
    kpad = -s.k0 % 4
    KC = kc_bucket(c.K1 + kpad)
    if KC > 32 or (wide and KC not in (8, 16, 24)):
        return False
    CF = s.k0 // 16 if vec_rows(s) else 0
    return bwd_lds(KC, CF, KC > 12 or wide, wide, c.nl == 3) <= LDS_MAX and fwd_lds(KC, CF, wide) <= LDS_MAX


def x6_supported(c):
    if not supported(c) or c.nl != 3 or c.N3 > 16:
        return False
    KV = c.K1 + -c.src.k0 % 4
    KC = (KV + 63) // 64 * 4
    return KC <= 12 and KV < 16 * KC          # (a free column for the ones that carry db1)


def needs_kept(c):
    return kc_bucket(c.K1 + -c.src.k0 % 4) > 12 or c.N3 > 16


def expected_plan(c, call, kept=True, lay=None):
    """what marl_mlp3_plan must report for the case (NS with the fields of ops.Mlp3Plan), None where the call is refused.
    kept: hsave given.  lay: the layout of Y / dY (default: the case's own)"""
    s, three, wide = c.src, c.nl == 3, c.N3 > 16
    x6, bwd = call.startswith("x6"), call.endswith("bwd")
    if not (x6_supported(c) if x6 else supported(c)):
        return None
    lay = lay or (dy_layout(c) if bwd else y_layout(c))
    kpad = -s.k0 % 4
    KV = c.K1 + kpad
    p = NS(kpad=kpad, KV=KV, three=three, wide=wide, n3t=(c.N3 + 15) // 16, kept=bool(kept), yvec=False, slabs=0)
    if x6:
        if bwd and not kept:
            return None
        p.KC = (KV + 63) // 64 * 4
        p.CF = s.k0 // 32 * 2 if vec_rows(s) else 0
        p.CFT = 6 if p.KC in (8, 12) and p.CF == 6 else -1
        p.wgpc = 2
    else:
        p.KC = kc_bucket(KV)
        p.CF = s.k0 // 16 if vec_rows(s) else 0
        p.CFT = 7 if not wide and p.KC in (8, 11) and p.CF == 7 else -1
    if bwd:
        if not x6:
            if (p.KC > 12 or wide) and not kept:
                return None
            if wide and (lay.ld % 4 or lay.gs % 4 or lay.off % 4):
                return None
            two, p.KH, p.passes = bwd_shape(p.KC, kept, wide)
            p.wgpc = 2 if two else 1
            p.lds = bwd_lds(p.KC, p.CF, kept, wide, three)
        else:
            two, p.KH, p.passes = True, 4, p.KC // 4
            p.lds = 8 * 768 * 4 + 4 * 3 * 128 * 4 + 3 * XR * 256 + (p.KC - p.CF) * 128
        units = (c.M + 63) // 64
        p.nst = stripes(units, c.G, 512 if two else 256)
        p.slabs = p.nst
    else:
        units = (c.M + 15) // 16
        p.nst = stripes((units + FNW - 1) // FNW, c.G)
        p.KH, p.passes = p.KC, 1
        if x6:
            p.lds = (4 * (p.KC // 2) + 8 + 2) * 768 * 4 + (p.KC - p.CF) * 128
        else:
            p.wgpc = 1 if (p.KC > 12 or wide) else 2
            p.lds = fwd_lds(p.KC, p.CF, wide)
            p.yvec = lay.ld % 4 == 0 and lay.gs % 4 == 0 and lay.off % 4 == 0 and c.N3 % 4 == 0
    p.per = (units + p.nst - 1) // p.nst
    p.grid = (p.nst + 7) // 8 * 8 * c.G
    return p


def instance(call, p):
    """the template instantiation a plan selects, as the MLP3_PICK* / X6_PICK macros name it"""
    if call.startswith("x6"):
        return (call, p.KC, p.CFT)
    return (call, p.KC, p.CFT, p.three, p.wide) + ((p.kept,) if call == "bwd" else ())


def all_instances():
    """every instantiation the dispatch macros of mlp3_fused.hip and mlp3_x6.hip can select"""
    small = [(4, -1), (8, -1), (8, 7), (11, -1), (11, 7), (12, -1)]
    out = []
    for three in (True, False):
        out += [("fwd", kc, cf, three, False) for kc, cf in small] + [("fwd", kc, -1, three, False) for kc in (16, 24, 32)]
        out += [("bwd", kc, cf, three, False, kept) for kc, cf in small for kept in (False, True)]
        out += [("bwd", kc, -1, three, False, True) for kc in (16, 24, 32)]
    out += [("fwd", kc, -1, False, True) for kc in (8, 16, 24)] + [("bwd", kc, -1, False, True, True) for kc in (8, 16, 24)]
    for call in ("x6_fwd", "x6_bwd"):
        out += [(call, 4, -1), (call, 8, -1), (call, 8, 6), (call, 12, -1), (call, 12, 6)]
    return out


# ================================================================================================ layouts
def y_layout(c):
    """Y: "cols" (M, G N3) with head g in columns [g N3, (g + 1) N3), rows ldy_pad floats longer; "blocks" (G, M, N3), each block
    gs_pad floats further; base yoff floats off the 16-byte grid"""
    if c.layout == "cols":
        return NS(ld=c.G * c.N3 + c.ldy_pad, gs=c.N3, off=c.yoff)
    ld = c.N3 + c.ldy_pad
    return NS(ld=ld, gs=c.M * ld + c.gs_pad, off=c.yoff)


def dy_layout(c):
    """dY: the layout of Y - but the WIDE backward takes 16-byte dY tiles only, so a wide case whose Y layout is there to switch
    yvec off has its dY in plain columns"""
    lay = y_layout(c)
    if c.N3 > 16 and (lay.ld % 4 or lay.gs % 4 or lay.off % 4):
        return NS(ld=c.G * c.N3, gs=c.N3, off=0)
    return lay


def lay_size(c, lay):
    return (c.G - 1) * lay.gs + (c.M - 1) * lay.ld + c.N3


def lay_index(c, lay):
    """[G, M, N3] flat positions of the heads' outputs in a buffer of lay_size floats"""
    g, m, n = np.meshgrid(np.arange(c.G), np.arange(c.M), np.arange(c.N3), indexing="ij")
    return g * lay.gs + m * lay.ld + n


W_NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")
GAP = 4          # sentinel floats between the tensors of the flat weight / gradient buffers


def w_layout(c):
    """one flat buffer: per head [W1 | b1 | W2 | b2 | W3 | b3], every tensor on the 16-byte grid and GAP floats apart.  Returns
    (offsets by name, floats per head, element strides by name: 0 for the layers a shared case shares)"""
    sizes = {"w1": HD * c.K1, "b1": HD, "w2": HD * HD, "b2": HD, "w3": c.N3 * HD, "b3": c.N3}
    off, o = {}, 0
    for n in W_NAMES:
        if c.nl == 2 and n in ("w2", "b2"):
            continue
        off[n] = o
        o += (sizes[n] + 3) // 4 * 4 + GAP
    gs = {n: (0 if (c.shared and n in ("w1", "b1")) else o) for n in off}
    return off, o, gs, sizes


# ================================================================================================ the operation and its bounds
def k_fp32(n, depth):
    """n: the terms that can be nonzero; depth: the length of the sum as the kernel runs it (zeros included)"""
    return n + 3.0


def k_x6(n, depth):
    return 1.016 * (32.0 + 6.0 * ((depth + 31) // 32) + 3.0) + 2.02


def relu(v):
    return np.maximum(v, 0.0)


def forward(c, X, w, k):
    """per head: pre-activations, activations, outputs and their running error bounds e1, e2, e3 (in units of 1, u included)"""
    A, n1, KV, out = np.abs, terms(c.src), c.K1 + -c.src.k0 % 4, []
    for g in range(c.G):
        g1 = 0 if c.shared else g
        p1 = X @ w.w1[g1].T + w.b1[g1]
        e1 = k(n1, KV) * U * (A(X) @ A(w.w1[g1]).T + A(w.b1[g1]))
        h1 = relu(p1)
        f = NS(p1=p1, e1=e1, h1=h1, p2=None)
        if c.nl == 3:
            f.p2 = h1 @ w.w2[g].T + w.b2[g]
            f.e2 = e1 @ A(w.w2[g]).T + k(HD, HD) * U * ((h1 + e1) @ A(w.w2[g]).T + A(w.b2[g]))
            f.h2 = relu(f.p2)
        else:
            f.e2, f.h2 = e1, h1
        f.Y = f.h2 @ w.w3[g].T + w.b3[g]
        f.eY = f.e2 @ A(w.w3[g]).T + k(HD, HD) * U * ((f.h2 + f.e2) @ A(w.w3[g]).T + A(w.b3[g]))
        f.kink = (A(p1) <= e1).any(1)
        if c.nl == 3:
            f.kink |= (A(f.p2) <= f.e2).any(1)
        out.append(f)
    return out


def _gh(G, eG, H, eH, kn):
    """(G^T H, its bound) - see the module docstring"""
    A = np.abs
    return G.T @ H, eG.T @ A(H) + A(G).T @ eH + eG.T @ eH + kn * U * ((A(G) + eG).T @ (A(H) + eH))


def backward(c, X, w, fs, dY, k, slabs):
    """per head g: {name: (gradient, bound)} for ONE backward run.  dY [G, M, N3]"""
    A, out = np.abs, []
    zx = np.zeros_like(X)
    for g, f in enumerate(fs):
        d3 = dY[g].astype(F64)
        nz = float((d3 != 0).any(1).sum())
        extra = slabs + (c.G if c.shared else 0)
        kn = k(nz + extra, 32 * (min(nz, (c.M + 31) // 32) + extra))
        z3 = np.zeros_like(d3)
        r = {}
        r["w3"] = _gh(d3, z3, f.h2, f.e2, kn)
        r["b3"] = (d3.sum(0), kn * U * A(d3).sum(0))
        t = d3 @ w.w3[g]
        et = k(c.N3, c.N3) * U * (A(d3) @ A(w.w3[g]))
        if c.nl == 3:
            d2, e2 = np.where(f.p2 > 0, t, 0.0), np.where(f.p2 > 0, et, 0.0)
            r["w2"] = _gh(d2, e2, f.h1, f.e1, kn)
            r["b2"] = (d2.sum(0), e2.sum(0) + kn * U * (A(d2) + e2).sum(0))
            t = d2 @ w.w2[g]
            et = e2 @ A(w.w2[g]) + k(HD, HD) * U * ((A(d2) + e2) @ A(w.w2[g]))
            f.d2 = d2
        d1, e1 = np.where(f.p1 > 0, t, 0.0), np.where(f.p1 > 0, et, 0.0)
        r["w1"] = _gh(d1, e1, X, zx, kn)
        r["b1"] = (d1.sum(0), e1.sum(0) + kn * U * (A(d1) + e1).sum(0))
        out.append(r)
    if c.shared:          # layer 1 is one tensor: its gradients are the sums over the groups (held by group 0)
        for n_ in ("w1", "b1"):
            tot = (sum(r[n_][0] for r in out), sum(r[n_][1] for r in out))
            for r in out:
                r[n_] = tot
    return out


# ================================================================================================ data
LADDER = ((2, 0.5, 2, 1.0), (1, 0.4, 2, 1.0), (1, 0.25, 1, 0.5), (1, 0.15, 1, 0.2), (1, 0.1, 1, 0.05), (1, 0.06, 1, 0.01))


REAL_SCALE = {"w1": lambda c: 0.5 / terms(c.src) ** 0.5, "w2": lambda c: 0.03, "w3": lambda c: 0.2, "b1": lambda c: 4.0,
              "b2": lambda c: 4.0, "b3": lambda c: 1.0}
SALTS = 8          # real / probe data: the first of this many seeds of a case that meets the kink cap


def _ints(rng, shape, r, density):
    v = rng.integers(-r, r + 1, size=shape).astype(F32)
    return np.where(rng.random(shape) < density, v, F32(0)).astype(F32)


def _weights(c, rng, kind, wr=1, dens=1.0):
    G = c.G
    shp = {"w1": (G, HD, c.K1), "b1": (G, HD), "w2": (G, HD, HD), "b2": (G, HD), "w3": (G, c.N3, HD), "b3": (G, c.N3)}
    w = NS()
    for n in W_NAMES:
        if kind == "exact":
            v = _ints(rng, shp[n], wr, dens if n[0] == "w" else 0.7)
        else:
            v = (rng.standard_normal(shp[n]) * REAL_SCALE[n](c)).astype(F32)
        setattr(w, n, v)
    if c.nl == 2:
        w.w2 = w.b2 = None
    return w


def sig_bits(v):
    """significant bits of integer-valued data (0 for 0)"""
    v = np.abs(np.asarray(v, F64)).astype(np.int64)
    low = v & -v
    return np.where(v == 0, 0, np.floor(np.log2(np.maximum(v // np.maximum(low, 1), 1))) + 1).astype(np.int64)


def abs_sums(c, X, w, dY, base):
    """exact data: the largest sum of absolute values of the terms of any forward value, delta or gradient element (both accumulating
    runs and the base contents included; a shared layer over its groups)"""
    A, worst = np.abs, 0.0
    X = A(X)
    sh1 = 0.0
    for g in range(c.G):
        g1 = 0 if c.shared else g
        a1 = X @ A(w.w1[g1]).T + A(w.b1[g1])
        a2 = a1 @ A(w.w2[g]).T + A(w.b2[g]) if c.nl == 3 else a1
        a3 = a2 @ A(w.w3[g]).T + A(w.b3[g])
        d3 = A(dY[g]).astype(F64)
        t = d3 @ A(w.w3[g])
        gr = [2 * (d3.T @ a2).max() + A(base.w3[g]).max(), 2 * d3.sum(0).max() + A(base.b3[g]).max()]
        if c.nl == 3:
            gr += [2 * (t.T @ a1).max() + A(base.w2[g]).max(), 2 * t.sum(0).max() + A(base.b2[g]).max()]
            t = t @ A(w.w2[g])
        g1w, g1b = 2 * (t.T @ X), 2 * t.sum(0)
        if c.shared:
            sh1 = sh1 + g1w.max() + g1b.max()
        gr += [g1w.max() + A(base.w1[g1]).max(), g1b.max() + A(base.b1[g1]).max(), sh1 + A(base.w1[0]).max()]
        worst = max([worst, a1.max(), a2.max(), a3.max(), t.max()] + gr)
    return worst


def probe_rows(c):
    """the rows on which a probe case's dY is nonzero (module docstring)"""
    at = [0, c.M - 1, 15, 16, 63, 64]
    for call, kept, unit in (("fwd", True, 16), ("bwd", False, 64), ("bwd", True, 64), ("x6_bwd", True, 64)):
        p = expected_plan(c, call, kept)
        if p is not None and p.per * unit < c.M:
            step = p.per * unit
            last = (c.M - 1) // step * step
            at += [step - 1, step, last - 1, last]
    ep = c.src.remap0[0] if c.src.remap0 else (c.src.remapi[0] if c.src.remapi else None)
    if ep:
        at += [ep - 1, ep]
    return np.array(sorted({r for r in at if 0 <= r < c.M}), dtype=np.int64)


def inputs(c, kind):
    return _inputs(c.name, kind)


@functools.lru_cache(maxsize=6)
def _inputs(name, kind):
    """every operand of a case and the float64 forward: NS(d, X, w, base, dY [G, M, N3], Y0, f (forward per head, fp32 bounds), fx
    (the same with the split pair's bounds, split cases only), kink [G, M], rung).  dY is zero on the kink rows of its head (by either
    pair's bound where the case runs both).  Shared between tests: read-only."""
    c = BY_NAME[name]
    rng = np.random.default_rng(case_seed(c.name + kind))
    d = make_src(c.src, c.M, rng, "exact" if kind == "exact" else "real")
    X = virtual_x(c.src, d, c.M)
    i = NS(c=c, kind=kind, d=d, X=X, rung=None, fx=None)
    shape = (c.G, c.M, c.N3)
    if kind == "exact":
        for rung, (wr, dens, dr, ddens) in enumerate(LADDER):
            r2 = np.random.default_rng(case_seed(c.name + kind) + rung)
            i.w = _weights(c, r2, kind, wr, dens)
            i.base = _weights(c, r2, kind, 3, 1.0)
            i.dY = np.where(r2.random((c.G, c.M, 1)) < ddens, _ints(r2, shape, dr, 0.8), F32(0)).astype(F32)
            i.dY[:, [0, c.M - 1]] = _ints(r2, (c.G, 2, c.N3), dr, 1.0)
            i.worst = abs_sums(c, X, i.w, i.dY, i.base)
            if i.worst < LIMIT:
                i.rung = rung
                break
        assert i.rung is not None, "no rung of the ladder keeps %s below 2^24" % c.name
        i.Y0 = _ints(rng, shape, 3, 1.0)
    else:
        return _real_inputs(c, kind, i, d, X)
    return _finish(c, kind, i)


def _real_inputs(c, kind, i, d, X):
    shape = (c.G, c.M, c.N3)
    for salt in range(SALTS):
        rng = np.random.default_rng(case_seed(c.name + kind) + 1000 + salt)
        i.salt = salt
        i.w = _weights(c, rng, kind)
        i.base = _weights(c, rng, kind)
        if kind == "probe":
            i.rows = probe_rows(c)
            i.dY = np.zeros(shape, F32)
            i.dY[:, i.rows] = rng.standard_normal((c.G, len(i.rows), c.N3)).astype(F32)
        else:
            i.dY = rng.standard_normal(shape).astype(F32)
        i.Y0 = rng.standard_normal(shape).astype(F32)
        _finish(c, kind, i)
        if i.kink.mean() <= KINK_CAP:
            break
    return i


def _finish(c, kind, i):
    X = i.X
    w64 = NS(**{n: (None if getattr(i.w, n) is None else getattr(i.w, n).astype(F64)) for n in W_NAMES})
    i.w64 = w64
    i.f = forward(c, X, w64, k_fp32)
    if c.x6:
        i.fx = forward(c, X, w64, k_x6)
    if kind == "exact":
        i.kink = np.zeros((c.G, c.M), bool)
        i.zeros1 = sum(int((f.p1 == 0).sum()) for f in i.f)
        i.zeros2 = sum(int((f.p2 == 0).sum()) for f in i.f) if c.nl == 3 else 0
    else:
        i.kink = np.stack([f.kink for f in i.f])
        if c.x6:          # (either pair's bound: the same dY serves both)
            i.kink |= np.stack([f.kink for f in i.fx])
        i.dY[i.kink] = 0
    i.Y = np.stack([f.Y for f in i.f])
    return i


def x6_exact(c, i):
    """exact data of a split case: one operand of every product has at most 8 significant bits (module docstring)"""
    backward(c, i.X, i.w64, i.f, i.dY, k_fp32, 1)          # (leaves the deltas dh2 in f.d2)
    worst = max(int(sig_bits(v).max()) for v in (i.X, i.w.w2, i.w.w3, i.dY))
    return max(worst, max(int(sig_bits(f.d2).max()) for f in i.f))


def grads(c, i, x6, slabs):
    """the float64 gradients of one backward run and their bounds: per head {name: (gradient, bound)}"""
    return backward(c, i.X, i.w64, i.fx if x6 else i.f, i.dY, k_x6 if x6 else k_fp32, slabs)


# ================================================================================================ cases
def case(name, M, G, N3, nl, s, x6=False, layout="cols", ldy_pad=0, gs_pad=0, yoff=0, shared=False, kinds=KINDS, want=None):
    """want: {(call, kept): {plan field: value}} - what the case is in the table for (asserted on top of the whole expected plan)"""
    c = NS(name=name, M=M, G=G, N3=N3, nl=nl, src=s, K1=width(s), x6=x6, layout=layout, ldy_pad=ldy_pad, gs_pad=gs_pad, yoff=yoff,
           shared=shared, kinds=kinds, want=want or {})
    if x6:
        assert x6_supported(c), name
    return c


FK, BR, BK, XF, XB = ("fwd", True), ("bwd", False), ("bwd", True), ("x6_fwd", True), ("x6_bwd", True)

# KV -> (k0, one-hot blocks, one-hot width): both sides of every step of the chunk buckets
BUCKETS = {64: (64, 0, 0), 65: (60, 1, 5), 128: (128, 0, 0), 129: (124, 1, 5), 160: (160, 0, 0), 161: (156, 1, 5), 176: (176, 0, 0),
           177: (172, 1, 5), 192: (192, 0, 0), 193: (188, 1, 5), 256: (256, 0, 0), 257: (252, 1, 5), 384: (384, 0, 0), 385: (380, 1, 5),
           512: (512, 0, 0)}
BUCKET_KC = {64: 4, 65: 8, 128: 8, 129: 12, 160: 12, 161: 11, 176: 11, 177: 12, 192: 12, 193: 16, 256: 16, 257: 24, 384: 24, 385: 32,
             512: 32}
# (k0, one-hot blocks, width) -> (KC, CF) of the fp32 pair and of the split pair: the compile-time CF variants and their neighbours
CF_SHAPES = {(96, 1, 20): ((8, 6), (8, 6)), (120, 0, 0): ((8, 7), (8, 6)), (128, 0, 0): ((8, 8), None), (64, 1, 20): ((8, 4), (8, 4)),
             (96, 5, 14): ((11, 6), (12, 6)), (120, 5, 11): ((11, 7), (12, 6)), (128, 3, 14): ((11, 8), (12, 8)),
             (64, 5, 20): ((11, 4), (12, 4))}
ROWS_M = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129)
REDUCE_SLABS = (1, 7, 8, 9, 15, 16, 17, 24, 256, 512)
N3_NARROW = (1, 3, 4, 15, 16)
N3_WIDE = (20, 32, 36, 144, 156, 160)


def _hot(k0, nh, hw, **kw):
    return src(k0=k0, nhot=nh, hot_w=hw, **kw)


def _cases():
    out = []
    # ---- chunk buckets, both sides of every step, two- and three-layer
    for KV, (k0, nh, hw) in BUCKETS.items():
        for nl in (3, 2):
            c = case("kv%d-l%d" % (KV, nl), 65, 2, 3, nl, _hot(k0, nh, hw))
            c.x6 = x6_supported(c)
            KC = BUCKET_KC[KV]
            c.want = {FK: dict(KC=KC, KV=KV)}
            if KC == 32:
                c.want[BK] = dict(KH=16, passes=2, wgpc=1)
            if KC == 12:
                c.want[BK] = dict(KH=12, passes=1, wgpc=1)
            out.append(c)
    # ---- kpad 1 .. 3 (0: everywhere else), vector rows
    for k0 in (29, 30, 31):
        c = case("kpad%d" % (-k0 % 4), 65, 2, 3, 3, _hot(k0, 2, 5), x6=True, want={FK: dict(kpad=-k0 % 4, KC=4, CF=1)})
        out.append(c)
    out.append(case("kpad2-kc24", 65, 2, 3, 3, src(k0=322), want={FK: dict(kpad=2, KC=24, CF=20)}))
    # ---- the compile-time CF variants beside their neighbours
    for (k0, nh, hw), (f32, x6p) in CF_SHAPES.items():
        for nl in (3, 2):
            c = case("cf-k%d+%dx%d-l%d" % (k0, nh, hw, nl), 65, 2, 3, nl, _hot(k0, nh, hw))
            c.x6 = x6_supported(c)
            c.want = {FK: dict(KC=f32[0], CF=f32[1], CFT=7 if f32[1] == 7 else -1)}
            if f32[0] == 11:
                c.want[BK] = dict(KH=6, passes=2, wgpc=2)
                c.want[BR] = dict(KH=11, passes=1, wgpc=1)
            if c.x6:
                assert x6p is not None
                c.want[XF] = dict(KC=x6p[0], CF=x6p[1], CFT=6 if x6p[1] == 6 else -1)
            out.append(c)
    # ---- input path: element loads (odd row stride; base off the grid), the narrowest dense segment
    out.append(case("elem-ld31", 65, 2, 3, 3, src(k0=30, ld0=31, nhot=2, hot_w=5), x6=True, want={FK: dict(CF=0), XF: dict(CF=0)}))
    out.append(case("elem-base+1", 65, 2, 3, 3, src(k0=32, off0=1, nhot=2, hot_w=5), x6=True, want={FK: dict(CF=0), XF: dict(CF=0)}))
    out.append(case("elem-ld121-kc8", 65, 2, 3, 2, src(k0=120, ld0=121), want={FK: dict(CF=0, KC=8, CFT=-1)}))
    out.append(case("k0=4", 65, 2, 3, 3, _hot(4, 2, 9), x6=True, want={FK: dict(CF=0, KC=4)}))
    # ---- input segments: dense1, a one-hot block across a 16-column chunk (columns 42 .. 48), rows that read as zero, episode map, remapi
    seg = dict(k0=20, k1=8, nhot=3, hot_w=7)
    out.append(case("seg-dense1-hot", 75, 2, 3, 3, src(**seg), x6=True))
    out.append(case("seg-remap", 129, 2, 3, 3, src(remap0=(15, 18, -2), emap=True, remapi=(15, 15, -3), **seg), x6=True))
    out.append(case("seg-remap-l2", 129, 2, 5, 2, src(remap0=(15, 18, -2), emap=True, remapi=(15, 15, -3), **seg)))
    out.append(case("seg-remap-kc16", 129, 2, 3, 3, src(k0=200, nhot=2, hot_w=9, remap0=(15, 18, -2), emap=True, remapi=(15, 15, -3))))
    # ---- head shapes
    for N3 in N3_NARROW:
        for nl in (3, 2):
            out.append(case("n3=%d-l%d" % (N3, nl), 33, 2, N3, nl, _hot(24, 1, 5), x6=nl == 3))
            out.append(case("n3=%d-l%d-blocks" % (N3, nl), 33, 2, N3, nl, _hot(24, 1, 5), x6=nl == 3, layout="blocks"))
    for N3 in N3_WIDE:
        out.append(case("wide%d" % N3, 65, 2, N3, 2, src(k0=72), want={FK: dict(wide=True, KC=8, n3t=(N3 + 15) // 16, yvec=True)}))
    out.append(case("wide36-kc16", 65, 2, 36, 2, src(k0=200), want={FK: dict(wide=True, KC=16, n3t=3)}))
    out.append(case("wide156-kc16-blocks", 65, 2, 156, 2, src(k0=200), layout="blocks", want={FK: dict(wide=True, KC=16, n3t=10)}))
    out.append(case("wide160-kc24", 65, 2, 160, 2, src(k0=322), want={FK: dict(wide=True, KC=24, CF=20, n3t=10, kpad=2)}))
    out.append(case("wide20-kc24", 65, 1, 20, 2, src(k0=384), want={FK: dict(wide=True, KC=24, CF=24, n3t=2)}))
    # ---- output stores: yvec on (wide32 above), and off by each cause in turn
    out.append(case("yvec-on-blocks", 65, 2, 32, 2, src(k0=72), layout="blocks", want={FK: dict(yvec=True)}))
    out.append(case("yvec-off-ldy", 65, 2, 32, 2, src(k0=72), ldy_pad=1, want={FK: dict(yvec=False)}))
    out.append(case("yvec-off-gs", 65, 2, 32, 2, src(k0=72), layout="blocks", gs_pad=2, want={FK: dict(yvec=False)}))
    out.append(case("yvec-off-base", 65, 2, 32, 2, src(k0=72), yoff=1, want={FK: dict(yvec=False)}))
    out.append(case("yvec-off-n3", 65, 2, 3, 2, src(k0=72), want={FK: dict(yvec=False)}))
    out.append(case("narrow-ldy-odd-base+1", 65, 3, 4, 3, _hot(24, 1, 5), x6=True, ldy_pad=1, yoff=1))
    # ---- rows
    for M in ROWS_M:
        out.append(case("rows%d" % M, M, 3, 2, 3, _hot(24, 1, 5), x6=True))
        out.append(case("rows%d-wide" % M, M, 2, 20, 2, src(k0=72)))
    # forward: 20 groups cap at 8 stripes; 65 tiles -> 9 per stripe: wave 0 of a workgroup walks a second tile, the others do not
    out.append(case("fwd-second-walk", 1037, 20, 2, 3, src(k0=8), x6=True, want={FK: dict(nst=8, per=9), XF: dict(nst=8, per=9)}))
    # 10 groups, 3073 rows: forward 193 tiles in 24 stripes of 9 (stripes 22, 23 empty); backward 49 iterations: recomputing 24 stripes
    # of 3 (17 .. 23 empty), kept and split 48 stripes of 2 (25 .. 47 empty)
    out.append(case("empty-stripes", 3073, 10, 2, 3, _hot(24, 1, 5), x6=True,
                    want={FK: dict(nst=24, per=9), BR: dict(nst=24, per=3, slabs=24), BK: dict(nst=48, per=2, slabs=48),
                          XB: dict(nst=48, per=2, slabs=48)}))
    out.append(case("empty-stripes-wide", 3073, 10, 20, 2, src(k0=72), want={FK: dict(nst=24, per=9), BK: dict(nst=24, per=3, wgpc=1)}))
    out.append(case("empty-stripes-kc12", 3073, 10, 2, 3, src(k0=180), kinds=("exact", "probe"),
                    want={FK: dict(nst=24, per=9), BK: dict(nst=24, per=3, wgpc=1, KC=12)}))
    # ---- the slab reduce: 1 .. 17 slabs around its 8-wide rounds and tail, 24 (empty-stripes), 256 and 512
    for sl in (1, 7, 8, 9, 15, 16, 17):
        out.append(case("slabs%d" % sl, 64 * sl - 5, 1, 2, 3, src(k0=8), x6=True, want={BR: dict(slabs=sl), BK: dict(slabs=sl), XB: dict(slabs=sl)}))
    out.append(case("slabs256", 16380, 1, 2, 3, src(k0=8), x6=True, kinds=("exact", "probe"),
                    want={BR: dict(slabs=256, per=1), BK: dict(slabs=256, per=1)}))
    out.append(case("slabs512", 32705, 1, 2, 3, src(k0=8), x6=True, kinds=("exact", "probe"),
                    want={BR: dict(slabs=256, per=2), BK: dict(slabs=512, per=1), XB: dict(slabs=512, per=1)}))
    # ---- layer 1 shared between the groups (one wide head in column blocks): its gradients are summed over the groups
    for G in (2, 3):
        out.append(case("shared-G%d" % G, 129, G, 20, 2, src(k0=72), shared=True))
    out.append(case("shared-G3-narrow", 129, 3, 5, 2, _hot(24, 1, 5), shared=True))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}

# shapes every entry point refuses
REFUSED = (
    case("refused-kv513", 65, 2, 3, 3, _hot(508, 1, 5)),
    case("refused-wide-kc24-unaligned", 65, 2, 160, 2, src(k0=322, ld0=323)),      # CF = 0: 165 888 bytes of LDS in the backward
    case("refused-wide-three", 65, 2, 32, 3, src(k0=72)),
    case("refused-wide-n3=22", 65, 2, 22, 2, src(k0=72)),
    case("refused-wide-kc12", 65, 2, 32, 2, src(k0=180)),
    case("refused-n3=164", 65, 2, 164, 2, src(k0=72)),
    case("refused-k0=3", 65, 2, 3, 3, _hot(3, 2, 5)),
    case("refused-k1=6", 65, 2, 3, 3, src(k0=24, k1=6)),
)
