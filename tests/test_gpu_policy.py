"""csrc/policy.hip on the MI355X against tests/policy_oracle.py (float64): marl_policy_probs, marl_policy_loss_bwd and
marl_policy_sample.  Bounds: tests/parity.close at 1e-4 * max|ref| for pi, log pi, the gradient on the logits and both statistics;
exact zeros on padded rows; bitwise equality of two calls; the sampler action for action wherever the draw is farther than 1e-5
from every float64 CDF boundary (under 0.5 % of the draws are not), and its frequencies within five standard deviations."""
import functools

import numpy as np
import pytest
import torch

import parity
import policy_oracle as po

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
EPSS = (0.0, 0.02, 0.5)
# one grid pass of the tiled kernels covers 1024 workgroups x 4 waves x 64 rows = 262 144 rows: 87 500 x 1 x 3 = 262 500 rows take a
# second trip of the grid-stride loop.  30 actions: past the 28 the staged tiles hold, the row-per-lane kernel
GRID_PASS_ROWS = 1024 * 4 * 64
SHAPES = [(3, 1, 2, 3), (4, 6, 5, 11), (2, 7, 8, 14), (37, 3, 10, 18), (2, 3, 2, 30), (87500, 1, 3, 3)]
assert SHAPES[-1][0] * SHAPES[-1][1] * SHAPES[-1][2] > GRID_PASS_ROWS


@functools.lru_cache(maxsize=None)
def case(shape, eps):
    B, T, N, A = shape
    rows = po.kernel_rows(B, T, N, A, seed=sum(shape))
    return rows, po.kernel_reference(rows, N, eps)


def dev(x, off=0):
    """device copy; off: floats of misalignment against the 16-byte boundary the staged copies want"""
    t = torch.as_tensor(x)
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    buf[off:].copy_(t.reshape(-1))
    return buf[off:].view(t.shape)


def run_loss(rows, N, eps, off=0):
    from marl_amd import ops
    R, A = rows["logits"].shape
    tail = 32
    dl = torch.full((R * A + tail + off,), float("nan"), device=DEV)[off:]
    logp = torch.full((R + tail,), float("nan"), device=DEV)
    stats = torch.full((4,), float("nan"), device=DEV)
    ops.policy_loss_bwd(dev(rows["logits"], off), dev(rows["avail"], off), dev(rows["u"]), dev(rows["G"]), dev(rows["v"]),
                        dev(rows["padded"]), eps, dl, logp, stats, R, N, A)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dl[R * A:]).all()) and bool(torch.isnan(logp[R:]).all()) and bool(torch.isnan(stats[2:]).all()), \
        "the kernel wrote behind its outputs"
    return dl[:R * A].view(R, A).cpu().numpy(), logp[:R].cpu().numpy(), stats[:2].cpu().numpy()


def run_probs(rows, eps, off=0):
    from marl_amd import ops
    R, A = rows["logits"].shape
    pi = torch.full((R * A + 32 + off,), float("nan"), device=DEV)[off:]
    ops.policy_probs(dev(rows["logits"], off), dev(rows["avail"], off), eps, pi, R, A)
    torch.cuda.synchronize()
    assert bool(torch.isnan(pi[R * A:]).all())
    return pi[:R * A].view(R, A).cpu().numpy()


@pytest.mark.parametrize("eps", EPSS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_vs_float64(shape, eps):
    rows, ref = case(shape, eps)
    N = shape[2]
    c = "policy:%s eps=%g" % ("x".join(map(str, shape)), eps)
    pi = run_probs(rows, eps)
    dl, logp, stats = run_loss(rows, N, eps)
    for name, got in (("pi", pi), ("dlogits", dl), ("logp", logp), ("stats", stats)):
        assert np.isfinite(got).all(), name
    parity.close(c, "pi", pi, ref["pi"])
    parity.close(c, "logp", logp, ref["logp"])
    parity.close(c, "dlogits", dl, ref["dlogits"])
    parity.close(c, "actor numerator", stats[0], ref["stats"][0])
    assert float(stats[1]) == ref["stats"][1]                       # N * M: a count
    pad, one = rows["pad_rows"], rows["one_rows"]
    assert pad.any() and len(one)
    assert not dl[pad].any() and not logp[pad].any() and not pi[pad].any()      # exact zeros, whatever the 1e6 logits hold
    assert not logp[one].any()                                      # one available action: log pi = 0 ...
    assert np.abs(dl[one]).max() <= 1e-4 * np.abs(ref["dlogits"]).max()         # ... and no gradient
    assert not pi[rows["avail"] == 0].any()
    # two calls, the same bits
    dl2, logp2, stats2 = run_loss(rows, N, eps)
    assert dl.tobytes() == dl2.tobytes() and logp.tobytes() == logp2.tobytes() and stats.tobytes() == stats2.tobytes()
    assert pi.tobytes() == run_probs(rows, eps).tobytes()


@pytest.mark.parametrize("shape", [(4, 6, 5, 11), (2, 7, 8, 14)], ids=lambda s: "x".join(map(str, s)))
def test_misaligned_operands_give_the_same_bits(shape):
    """operands one float off the 16-byte boundary take the element-wise staging copy: the same arithmetic"""
    rows, _ = case(shape, 0.02)
    a, b = run_loss(rows, shape[2], 0.02), run_loss(rows, shape[2], 0.02, off=1)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert run_probs(rows, 0.02).tobytes() == run_probs(rows, 0.02, off=1).tobytes()


def test_no_rows_launch_nothing():
    from marl_amd import _lib
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    assert lib.marl_policy_probs(None, None, 0.1, None, 0, 5, s) == 0
    assert lib.marl_policy_loss_bwd(None, None, None, None, None, None, 0.1, None, None, None, None, 0, 2, 5, s) == 0
    assert lib.marl_policy_sample(None, None, 0, None, 0.1, 1, 0, None, 0, None, 0, 0, 5, 11, s) == 0
    x = torch.ones(64, device=DEV)
    assert lib.marl_policy_loss_bwd(x.data_ptr(), x.data_ptr(), None, None, None, None, 0.1, None, None, None, None, 4, 2, 5, s) != 0


# ---------------------------------------------------------------------------------------------------- the sampler
def run_sample(z, a, alive, eps, rseed, env0, tg):
    from marl_amd import ops
    E, N, A = z.shape
    act = torch.full((E, N), -7, dtype=torch.int32, device=DEV)
    ops.policy_sample(dev(z), dev(a), N * A, None if alive is None else dev(alive), eps, rseed, env0, None, tg, act, N, E, N, A)
    torch.cuda.synchronize()
    return act.cpu().numpy()


@pytest.mark.parametrize("tg,eps,seed", po.SAMPLER_SEEDS)
def test_sampler_vs_restatement(tg, eps, seed):
    z, a, alive = po.sampler_case(4096, 5, 11, seed)
    got = run_sample(z, a, alive, eps, 5, 100, tg)
    want, margin, _ = po.sample(z, a, alive, eps, 5, 100, tg)
    live = alive != 0
    assert (got[~live] == -1).all()
    assert (got[live] >= 0).all() and (np.take_along_axis(a[live], got[live][..., None].astype(np.int64), -1) == 1).all()
    far = live[:, None] & (margin >= po.SAMPLER_EXCLUDE)
    assert float((~far[live]).mean()) < po.SAMPLER_CAP
    assert (got[far] == want[far]).all(), int((got[far] != want[far]).sum())
    assert run_sample(z, a, alive, eps, 5, 100, tg).tobytes() == got.tobytes()


@pytest.mark.parametrize("eps", [0.0, 0.5])
def test_sampler_frequencies(eps):
    """65 536 environments share one logit / availability row per agent: every available action's frequency within five standard
    deviations sqrt(pi (1 - pi) / n) of pi, and an unavailable action is never drawn"""
    E, N, A = 65536, 5, 11
    z1, a1, _ = po.sampler_case(1, N, A, 31)
    z, a = np.repeat(z1, E, 0), np.repeat(a1, E, 0)
    got = run_sample(z, a, None, eps, 9, 0, 3)
    pi = po.policy(torch.tensor(z1[0].astype(np.float64)), torch.tensor(a1[0].astype(np.float64)), eps).numpy()
    for n in range(N):
        freq = np.bincount(got[:, n], minlength=A) / E
        assert not freq[a1[0, n] == 0].any()
        sd = np.sqrt(pi[n] * (1 - pi[n]) / E)
        assert (np.abs(freq - pi[n]) <= 5 * sd + 1e-12).all(), (n, freq, pi[n])
