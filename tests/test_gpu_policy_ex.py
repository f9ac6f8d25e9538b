"""marl_policy_loss_bwd_ex (csrc/policy.hip) on the MI355X against tests/pg_oracle.py (float64): the actor loss without a baseline
and with the entropy bonus.  Bounds: tests/parity.close at 1e-4 * max|ref| for log pi, H, the gradient on the logits and the
statistics; the count N sum m exact; the bitwise contracts of include/marl_hip.h (beta = 0 with v is marl_policy_loss_bwd; dead rows
are never looked at; aliasing, misalignment, a NULL ent and a second call change no bit)."""
import functools

import numpy as np
import pytest
import torch

import parity
import pg_oracle as pg
import policy_oracle as po

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GRID_PASS_ROWS = 1024 * 4 * 64
# (B*T, N, A, eps, beta, v given): rows = B*T*N at the edges of the 64-row wave tile and of the 256-row workgroup, and one past a
# full grid pass; A = 11 (odd), 14 / 18 (two-way LDS walks), 28 / 29 (the last tiled, the first row-per-lane), 3 (the matrix game)
CASES = [(1, 1, 11, 0.0, 0.01, False), (63, 1, 14, 0.3, 1.0, True), (64, 1, 18, 0.0, 1.0, False), (13, 5, 11, 0.3, 0.01, True),
         (51, 5, 28, 0.0, 0.01, False), (256, 1, 29, 0.3, 1.0, True), (257, 1, 3, 0.0, 0.0, True), (26, 10, 11, 0.3, 0.01, False),
         (26, 10, 29, 0.0, 0.01, False), (26, 10, 14, 0.0, 0.0, False), (52429, 5, 3, 0.3, 0.01, True)]
assert sorted(c[0] * c[1] for c in CASES[:7]) == [1, 63, 64, 65, 255, 256, 257] and CASES[-1][0] * CASES[-1][1] == GRID_PASS_ROWS + 1
ids = lambda c: "%dx%dx%d-eps%g-beta%g-%s" % (c[0] * c[1], c[1], c[2], c[3], c[4], "v" if c[5] else "nov")


@functools.lru_cache(maxsize=None)
def content(BT, N, A, special=False):
    rows = po.kernel_rows(BT, 1, N, A, seed=BT + N + A)
    where = pg.special_rows(rows, N) if special else None
    return rows, where


@functools.lru_cache(maxsize=None)
def reference(BT, N, A, eps, beta, with_v, special=False):
    return pg.kernel_reference(content(BT, N, A, special)[0], N, eps, beta, with_v)


def dev(x, off=0):
    """device copy; off: floats of misalignment against the 16-byte boundary the staged copies want"""
    t = torch.as_tensor(x)
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    buf[off:].copy_(t.reshape(-1))
    return buf[off:].view(t.shape)


def run_ex(rows, N, eps, beta, with_v=True, with_ent=True, off=0, alias=False, plain=False):
    """(dlogits, logp, ent or None, statistics) of one call; plain: marl_policy_loss_bwd instead.  The tails behind the outputs
    are checked to be untouched"""
    from marl_amd import ops
    R, A = rows["logits"].shape
    tail = 32
    logits = torch.full((R * A + tail + off,), float("nan"), device=DEV)[off:]
    logits[:R * A].copy_(torch.as_tensor(rows["logits"]).reshape(-1))
    dl = logits if alias else torch.full((R * A + tail + off,), float("nan"), device=DEV)[off:]
    logp = torch.full((R + tail,), float("nan"), device=DEV)
    ent = torch.full((R + tail,), float("nan"), device=DEV) if with_ent and not plain else None
    stats = torch.full((5,), float("nan"), device=DEV)
    common = (logits, dev(rows["avail"], off), dev(rows["u"]), dev(rows["G"]))
    if plain:
        ops.policy_loss_bwd(*common, dev(rows["v"]), dev(rows["padded"]), eps, dl, logp, stats, R, N, A)
    else:
        ops.policy_loss_bwd_ex(*common, dev(rows["v"]) if with_v else None, dev(rows["padded"]), eps, beta, dl, logp, ent, stats,
                               R, N, A)
    torch.cuda.synchronize()
    ns = 2 if plain else 3
    assert bool(torch.isnan(dl[R * A:]).all()) and bool(torch.isnan(logp[R:]).all()) and bool(torch.isnan(stats[ns:]).all()) \
        and (ent is None or bool(torch.isnan(ent[R:]).all())), "the kernel wrote behind its outputs"
    return (dl[:R * A].view(R, A).cpu().numpy(), logp[:R].cpu().numpy(), None if ent is None else ent[:R].cpu().numpy(),
            stats[:ns].cpu().numpy())


def same_bits(x, y):
    return all((a is None and b is None) or a.tobytes() == b.tobytes() for a, b in zip(x, y))


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_ex_vs_float64(case):
    BT, N, A, eps, beta, with_v = case
    rows, ref = content(BT, N, A)[0], reference(*case)
    c = "policy_ex:" + ids(case)
    dl, logp, ent, stats = got = run_ex(rows, N, eps, beta, with_v)
    for name, x in zip(("dlogits", "logp", "ent", "stats"), got):
        assert np.isfinite(x).all(), name
    parity.close(c, "logp", logp, ref["logp"])
    parity.close(c, "ent", ent, ref["ent"])
    parity.close(c, "dlogits", dl, ref["dlogits"])
    parity.close(c, "numerator", stats[0], ref["stats"][0])
    parity.close(c, "sum m H", stats[2], ref["stats"][2])
    assert float(stats[1]) == ref["stats"][1]                       # N * M: a count
    m = 1.0 - np.repeat(rows["padded"], N).astype(np.float64)
    parity.close(c, "sum m H of ent", stats[2], float(np.sum(ent.astype(np.float64) * m)))
    pad, one = rows["pad_rows"], rows["one_rows"]
    assert not dl[pad].any() and not logp[pad].any() and not ent[pad].any()
    assert not dl[one].any() and not logp[one].any() and not ent[one].any()      # n = 1: H = 0 and no gradient, exactly
    assert same_bits(got, run_ex(rows, N, eps, beta, with_v))                    # two calls, the same bits
    assert same_bits(got[:2] + got[3:], (lambda o: o[:2] + o[3:])(run_ex(rows, N, eps, beta, with_v, with_ent=False)))


@pytest.mark.parametrize("eps", [0.0, 0.3])
@pytest.mark.parametrize("BT,N,A", [(52, 5, 11), (26, 10, 28), (26, 10, 29), (52429, 5, 3)], ids=lambda v: str(v))
def test_beta_zero_with_v_is_the_plain_loss_kernel_bit_for_bit(BT, N, A, eps):
    rows = content(BT, N, A)[0]
    dl, logp, ent, stats = run_ex(rows, N, eps, 0.0)
    dl0, logp0, _, stats0 = run_ex(rows, N, eps, 0.0, plain=True)
    assert dl.tobytes() == dl0.tobytes() and logp.tobytes() == logp0.tobytes() and stats[:2].tobytes() == stats0.tobytes()


@pytest.mark.parametrize("eps", [0.0, 0.3])
@pytest.mark.parametrize("A", [11, 29])
def test_special_rows_and_bitwise_contracts(A, eps):
    BT, N, beta = 52, 5, 0.01
    rows, where = content(BT, N, A, True)
    ref = reference(BT, N, A, eps, beta, False, True)
    c = "policy_ex:special A=%d eps=%g" % (A, eps)
    dl, logp, ent, stats = got = run_ex(rows, N, eps, beta, with_v=False)
    for name, x in zip(("dlogits", "logp", "ent", "stats"), got):
        assert np.isfinite(x).all(), name                            # the row with a logit 200 below included
    parity.close(c, "logp", logp, ref["logp"])
    parity.close(c, "ent", ent, ref["ent"])
    parity.close(c, "dlogits", dl, ref["dlogits"])
    parity.close(c, "numerator", stats[0], ref["stats"][0])
    parity.close(c, "sum m H", stats[2], ref["stats"][2])
    assert float(stats[1]) == ref["stats"][1]
    bad = where["bad_u"]
    assert not dl[bad].any() and logp[bad] == 0 and ent[bad] == 0                # a taken action that is not available: no policy
    assert ent[where["deep"]] > 0
    # dlogits written over the logits, operands one float off the 16-byte boundary: the same bits
    assert same_bits(got, run_ex(rows, N, eps, beta, with_v=False, alias=True))
    assert same_bits(got, run_ex(rows, N, eps, beta, with_v=False, off=1))
    assert same_bits(got, run_ex(rows, N, eps, beta, with_v=False, off=1, alias=True))
    # dead rows are never looked at: NaN logits, every action "available" and 1e6 in G on the padded steps change nothing
    junk = {k: np.array(x, copy=True) for k, x in rows.items()}
    pad = rows["pad_rows"]
    junk["logits"][pad] = np.nan
    junk["avail"][pad] = 1.0
    junk["G"][rows["padded"] == 1] = 1.0e6
    junk["v"][rows["padded"] == 1] = 1.0e6
    assert same_bits(got, run_ex(junk, N, eps, beta, with_v=False))
    with_v = run_ex(rows, N, eps, beta, with_v=True)
    assert same_bits(with_v, run_ex(junk, N, eps, beta, with_v=True))
    assert not dl[pad].any() and not logp[pad].any() and not ent[pad].any()


def test_no_rows_launch_nothing_and_bad_arguments_are_refused():
    from marl_amd import _lib
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    n = None
    assert lib.marl_policy_loss_bwd_ex(n, n, n, n, n, n, 0.1, 0.01, n, n, n, n, n, 0, 2, 5, s) == 0
    x = torch.ones(64, device=DEV)
    p = x.data_ptr()
    assert lib.marl_policy_loss_bwd_ex(p, p, n, n, n, n, 0.1, 0.01, n, n, n, n, n, 4, 2, 5, s) != 0
    q = torch.ones(64, device=DEV).data_ptr()
    assert lib.marl_policy_loss_bwd_ex(p, q, p, p, n, p, 0.1, -0.5, p, p, n, p, p, 0, 2, 5, s) == 0      # (no rows: no check)
    assert lib.marl_policy_loss_bwd_ex(p, q, p, p, n, p, 0.1, -0.5, p, p, n, p, p, 4, 2, 5, s) != 0      # beta < 0
