"""marl_ppo_loss_bwd (csrc/policy.hip) and marl_masked_standardize (csrc/ppo.hip) on the MI355X against tests/ppo_oracle.py
(float64).  Bounds: tests/parity.close at 1e-4 * max|ref| for log pi, H, the gradient on the logits, the numerator and the
standardised values; the counts (N sum m, the clipped rows, M) exact; the bitwise contracts of include/marl_hip.h (without logp_old
the pass is marl_policy_loss_bwd_ex's; dead rows are never looked at; misalignment and a second call change no bit)."""
import functools

import numpy as np
import pytest
import torch

import parity
import ppo_oracle as pp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GRID_PASS_ROWS = 1024 * 4 * 64
# tests/test_gpu_policy.py's SHAPES (B, T, N, A): (2, 3, 2, 30) takes the row-per-lane form, (87500, 1, 3, 3) a second grid trip
SHAPES = [(3, 1, 2, 3), (4, 6, 5, 11), (2, 7, 8, 14), (37, 3, 10, 18), (2, 3, 2, 30), (87500, 1, 3, 3)]
assert tuple(SHAPES) == pp.KERNEL_SHAPES and SHAPES[-1][0] * SHAPES[-1][1] * SHAPES[-1][2] > GRID_PASS_ROWS
C, BETA = pp.KERNEL_CLIP, pp.KERNEL_BETA
assert (C, BETA) == (0.2, 0.01)
sid = lambda s: "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def content(shape, eps):
    return pp.kernel_case(shape, eps, pp.kernel_seed(shape), C)


@functools.lru_cache(maxsize=None)
def reference(shape, eps, beta, with_old=True):
    rows = content(shape, eps)
    return pp.kernel_reference(rows, shape[2], eps, beta, C, rows["logp_old"] if with_old else None, rows["adv"])


def dev(x, off=0):
    """device copy; off: floats of misalignment against the 16-byte boundary the staged copies want"""
    t = torch.as_tensor(x)
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    buf[off:].copy_(t.reshape(-1))
    return buf[off:].view(t.shape)


def run_ppo(rows, N, eps, beta, clip=C, with_old=True, with_ent=True, off=0, ex=False):
    """(dlogits, logp, ent or None, statistics) of one call; ex: marl_policy_loss_bwd_ex with G = adv and no v instead.  NaN
    canaries behind every output are checked to be untouched"""
    from marl_amd import ops
    R, A = rows["logits"].shape
    tail = 32
    logits = dev(rows["logits"], off)
    dl = torch.full((R * A + tail + off,), float("nan"), device=DEV)[off:]
    logp = torch.full((R + tail,), float("nan"), device=DEV)
    ent = torch.full((R + tail,), float("nan"), device=DEV) if with_ent else None
    stats = torch.full((6,), float("nan"), device=DEV)
    common = (logits, dev(rows["avail"], off), dev(rows["u"]), dev(rows["adv"]))
    if ex:
        ops.policy_loss_bwd_ex(*common, None, dev(rows["padded"]), eps, beta, dl, logp, ent, stats, R, N, A)
    else:
        ops.ppo_loss_bwd(*common, dev(rows["logp_old"]) if with_old else None, dev(rows["padded"]), eps, beta, clip, dl, logp, ent,
                         stats, R, N, A)
    torch.cuda.synchronize()
    ns = 3 if ex else 4
    assert bool(torch.isnan(dl[R * A:]).all()) and bool(torch.isnan(logp[R:]).all()) and bool(torch.isnan(stats[ns:]).all()) \
        and (ent is None or bool(torch.isnan(ent[R:]).all())), "the kernel wrote behind its outputs"
    return (dl[:R * A].view(R, A).cpu().numpy(), logp[:R].cpu().numpy(), None if ent is None else ent[:R].cpu().numpy(),
            stats[:ns].cpu().numpy())


def same_bits(x, y):
    return all((a is None and b is None) or a.tobytes() == b.tobytes() for a, b in zip(x, y))


@pytest.mark.parametrize("eps,beta", [(0.0, BETA), (0.02, BETA), (0.5, BETA), (0.02, 0.0)], ids=lambda v: "%g" % v)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_ppo_loss_bwd_vs_float64(shape, eps, beta):
    rows, ref = content(shape, eps), reference(shape, eps, beta)
    N = shape[2]
    c = "ppo:%s eps=%g beta=%g" % (sid(shape), eps, beta)
    dl, logp, ent, stats = got = run_ppo(rows, N, eps, beta)
    for name, x in zip(("dlogits", "logp", "ent", "stats"), got):
        assert np.isfinite(x).all(), name
    parity.close(c, "dlogits", dl, ref["dlogits"])
    parity.close(c, "logp", logp, ref["logp"])
    parity.close(c, "ent", ent, ref["ent"])
    parity.close(c, "numerator", stats[0], ref["stats"][0])
    parity.close(c, "sum m H", stats[2], ref["stats"][2])
    assert float(stats[1]) == ref["stats"][1]                                  # N * M: a count
    assert float(stats[3]) == ref["stats"][3] == float(ref["clipped"].sum())   # the clipped rows: a count
    # the mask itself, row by row: with beta = 0 a clipped row's gradient is exactly zero and no other spread row's is
    if beta == 0.0:
        spread = (rows["avail"].sum(-1) > 1) & ~rows["pad_rows"]
        assert not dl[ref["clipped"]].any() and bool(dl[spread & ~ref["clipped"]].any(axis=1).all())
    pad, one = rows["pad_rows"], rows["one_rows"]
    assert not dl[pad].any() and not logp[pad].any() and not ent[pad].any()      # whatever their 1e6 logits and NaN logp_old hold
    assert np.isnan(rows["logp_old"][pad]).all() and (np.abs(rows["logits"][pad]) == 1e6).all()
    assert not dl[one].any() and not logp[one].any() and not ent[one].any()      # n = 1: rho = 1, H = 0, no gradient, exactly
    assert same_bits(got, run_ppo(rows, N, eps, beta))                           # two calls, the same bits
    assert same_bits(got, run_ppo(rows, N, eps, beta, off=1))                    # operands one float off 16 bytes
    assert same_bits(got[:2] + got[3:], (lambda o: o[:2] + o[3:])(run_ppo(rows, N, eps, beta, with_ent=False)))


@pytest.mark.parametrize("eps,beta", [(0.0, BETA), (0.5, BETA), (0.02, 0.0)], ids=lambda v: "%g" % v)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_without_logp_old_it_is_policy_loss_bwd_ex_bit_for_bit(shape, eps, beta):
    rows = content(shape, eps)
    N = shape[2]
    dl, logp, ent, stats = run_ppo(rows, N, eps, beta, with_old=False)
    dl0, logp0, ent0, stats0 = run_ppo(rows, N, eps, beta, ex=True)
    assert dl.tobytes() == dl0.tobytes() and logp.tobytes() == logp0.tobytes() and ent.tobytes() == ent0.tobytes()
    assert stats[3] == 0 and stats[1] == stats0[1] and stats[2] == stats0[2]
    ref = reference(shape, eps, beta, False)
    parity.close("ppo:%s eps=%g first pass" % (sid(shape), eps), "numerator", stats[0], ref["stats"][0])      # - sum m adv - beta sum m H


def test_dead_rows_are_never_looked_at():
    """NaN logits, every action "available", NaN adv and logp_old on the padded steps change no bit"""
    shape, eps = (4, 6, 5, 11), 0.02
    rows = content(shape, eps)
    got = run_ppo(rows, shape[2], eps, BETA)
    junk = {k: np.array(x, copy=True) for k, x in rows.items() if isinstance(x, np.ndarray)}
    pad = rows["pad_rows"]
    junk["logits"][pad] = np.nan
    junk["avail"][pad] = 1.0
    junk["adv"][rows["padded"] == 1] = np.nan
    assert same_bits(got, run_ppo(junk, shape[2], eps, BETA))


def test_no_rows_launch_nothing_and_bad_arguments_are_refused():
    from marl_amd import _lib
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    n = None
    f = lib.marl_ppo_loss_bwd
    assert f(n, n, n, n, n, n, 0.1, 0.01, 0.2, n, n, n, n, n, 0, 2, 5, s) == 0
    keep = torch.ones(64, device=DEV), torch.ones(64, device=DEV)
    p, q = keep[0].data_ptr(), keep[1].data_ptr()
    assert p != q
    good = lambda **kw: f(*[kw.get(k, v) for k, v in (("logits", p), ("avail", q), ("u", p), ("adv", p), ("old", n), ("padded", p),
                                                      ("eps", 0.1), ("beta", 0.01), ("clip", 0.2), ("dl", p), ("logp", p), ("ent", n),
                                                      ("out4", p), ("ws", p), ("rows", 4), ("N", 2), ("A", 5))], s)
    torch.cuda.synchronize()
    for bad in (dict(logits=n), dict(avail=n), dict(u=n), dict(adv=n), dict(padded=n), dict(dl=n), dict(logp=n), dict(out4=n),
                dict(ws=n), dict(rows=5), dict(clip=0.0), dict(clip=1.0), dict(clip=-0.2), dict(clip=float("nan")), dict(beta=-0.5),
                dict(dl=q), dict(N=0)):
        assert good(**bad) != 0, bad
    assert good(rows=0, clip=7.0, beta=-1.0) == 0                          # (no rows: no check, no launch)
    assert lib.marl_masked_standardize(n, n, n, n, n, 0, s) == 0
    assert lib.marl_masked_standardize(p, p, p, n, p, 4, s) != 0 and lib.marl_masked_standardize(p, q, q, p, p, 4, s) != 0


# ---------------------------------------------------------------------------------------------------- masked_standardize
def run_std(x, padded, in_place=False):
    from marl_amd import ops
    rows, tail = len(x), 32
    xd = torch.full((rows + tail,), float("nan"), device=DEV)
    xd[:rows].copy_(torch.as_tensor(x))
    out = xd if in_place else torch.full((rows + tail,), float("nan"), device=DEV)
    stats = torch.full((5,), float("nan"), device=DEV)
    ops.masked_standardize(xd, dev(padded), out, stats, rows)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[rows:]).all()) and bool(torch.isnan(stats[3:]).all()), "the kernel wrote behind its outputs"
    return out[:rows].cpu().numpy(), stats[:3].cpu().numpy()


STD_CASES = [(r, "rand") for r in (1, 2, 63, 64, 65, 4097, 300000)] + [(4097, "allpad"), (4097, "one"), (300000, "far"), (65, "far")]


@pytest.mark.parametrize("rows,how", STD_CASES, ids=lambda v: str(v))
def test_masked_standardize_vs_float64(rows, how):
    x, padded = pp.standardize_case(rows, how)
    ref, mean, var, M = pp.standardize(torch.tensor(x.astype(np.float64)), torch.tensor(padded.astype(np.float64)))
    c = "standardize:%d %s" % (rows, how)
    out, stats = got = run_std(x, padded)
    assert np.isfinite(out).all() and not out[padded == 1].any()              # padded rows: exact zeros, whatever NaN x holds there
    assert float(stats[2]) == M == float((padded == 0).sum())
    parity.close(c, "out", out, ref.numpy())
    parity.close(c, "mean", stats[0], mean)
    parity.close(c, "var", stats[1], var)
    if M == 0:
        assert not out.any() and not stats.any()
    if how == "one":
        assert not out.any() and stats[1] == 0 and stats[0] == x[padded == 0][0]
    assert same_bits(got, run_std(x, padded))                                   # two calls, the same bits
    assert same_bits(got, run_std(x, padded, in_place=True))                    # out may be x
