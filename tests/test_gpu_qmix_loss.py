"""The loss-folded QMIX backward kernels - marl_qmix_fused_loss_bwd / _x6 (csrc/qmix_fused.hip, LOSS = true) and
marl_qmix_wide_loss_bwd (csrc/qmix_wide.hip) - against the float64 statement of the operation (tests/qmix_loss_oracle.py), at
the row counts where their launch code changes behaviour, and on the contract include/marl_hip.h gives them.  Every QMIX update
goes through one of them (algorithm/q_learner.py, network/mixer.py: hip_loss_backward); the learner-level half of the pair is
tests/test_gpu_edges.py::test_qmix_loss_folded_into_the_mixer_backward.  Needs a real MI355X: ``pytest -m gpu``.

Bounds (none of them new): those the unfolded kernels of the same family and mode hold against torch-CPU in
tests/test_gpu_kernels.py (test_qmix_fused, test_qmix_wide), scaled by max(1, max|want|): q_tot and dq 1e-4; gradients 1e-4
(fused: 2e-4 max(1, sqrt(R / 64))); weight matrices of the wide kernel with bf16 weight-gradient operands 2e-2.  sum(mask) is a
sum of fewer than 2^24 zeros and ones: exact.  sum td^2 gets what the q_tot bound implies: 2 tol sum(mask |td|) + tol^2 sum(mask).
Kinks: an output column of |w1|, |w2|, relu(h) with a float64 value within 2e-6 of 0 is left out of that segment's weight and
bias gradient comparison only; at most 2 such columns per case (4 for the 32775-row case in the bf16 modes), by choice of seed
(counted on the CPU: tests/test_qmix_loss_oracle_cpu.py)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import qmix_loss_oracle as qo

pytestmark = pytest.mark.gpu

E = qo.E
SENTINEL = -77.25
# kernel modes: fused f32 / bf16x6 split; wide C-ABI flags 0 (fp32), 3 (bf16 operands in both GEMMs), 1 (bf16 forward GEMM only)
WIDE_MODE = {0: dict(bf16=False, wgrad_bf16=None), 3: dict(bf16=True, wgrad_bf16=True), 1: dict(bf16=True, wgrad_bf16=False)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from marl_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def cu(x, dev, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x)).to(dtype).to(dev).contiguous()


def close(a, b, atol=1e-4, rtol=1e-4, msg=""):
    np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(), atol=atol, rtol=rtol, err_msg=msg)


def _upload(dev, family, c, remap=False):
    """the inputs of a case on the device.  State rows carry the padded stride of the existing tests with zeros in the pad columns
    (the wide kernel reads them); remap: the learner's view - (T+1)-slot storage of more episodes than the batch, read in place
    through an episode map and a slot offset, every other slot and episode filled with different data"""
    from marl_amd import ops
    R, S = c.R, c.S
    ld = (S + 3) // 4 * 4 + (4 if family == "fused" else 0)
    if remap:
        T = qo.REMAP_T
        Eb, Es = R // T, R // T + 7
        assert Eb * T == R
        g = torch.Generator().manual_seed(R)
        perm = torch.randperm(Es, generator=g)[:Eb]
        store = torch.zeros(Es, T + 1, ld)
        store[:, :, :S] = torch.randn(Es, T + 1, S, generator=g)
        store[perm, 1:, :S] = c.s.view(Eb, T, S)
        sd = cu(store.view(Es * (T + 1), ld), dev)
        xs = ops.src(ops.Rows(sd[:, :S], (T, T + 1, 1), cu(perm, dev, torch.int32)))
    else:
        sd = torch.zeros(R, ld, device=dev)
        sd[:, :S] = cu(c.s, dev)
        xs = ops.src(sd[:, :S])
    return types.SimpleNamespace(W={k: cu(v, dev) for k, v in c.P.items()}, xs=xs, sd=sd, q=cu(c.q, dev), tgt=cu(c.q_tot_tgt, dev),
                                 r=cu(c.r, dev), term=cu(c.term, dev), padded=cu(c.padded, dev))


def _call(dev, family, mode, c, d, gamma=0.99, base=None, fill=(3.0, 5.0), with_q_tot=True, into=None, **over):
    """ONE call of the loss-folded entry point.  q_tot and dq are views of buffers 16 rows longer, pre-filled with a sentinel;
    gradients start from `base` (zeros when None), loss2 from `fill`; `into`: accumulate into the buffers of an earlier call.
    over: device tensors that replace r / tgt / term / padded."""
    from marl_amd import ops
    R, N, S = c.R, c.N, c.S
    if into is None:
        G = {k: (cu(base[k], dev) if base is not None else torch.zeros(v.shape, device=dev)) for k, v in c.P.items()}
        loss2 = torch.tensor(fill, device=dev, dtype=torch.float32)
    else:
        G, loss2 = into.G, into.loss2
    qt_buf = torch.full((R + 16,), SENTINEL, device=dev)
    dq_buf = torch.full((R + 16, N), SENTINEL, device=dev)
    assert qt_buf.data_ptr() % 16 == 0
    q_tot = qt_buf[:R] if with_q_tot else None
    a = [ops.qmix_weights(d.W), d.xs, d.q, over.get("tgt", d.tgt), over.get("r", d.r), over.get("term", d.term),
         over.get("padded", d.padded), gamma, q_tot, dq_buf[:R], ops.qmix_weights(G), loss2, R, N, S, E]
    if family == "fused":
        assert ops.qmix_fused_supported(N, S, E)
        ops.qmix_fused_loss_bwd(*a, x6=(mode == "bf16x6"))
    else:
        assert ops.qmix_wide_supported(N, S, E)
        ops.qmix_wide_loss_bwd(*a, **WIDE_MODE[mode])
    torch.cuda.synchronize()
    return types.SimpleNamespace(q_tot=q_tot, dq=dq_buf[:R], G=G, loss2=loss2, qt_buf=qt_buf, dq_buf=dq_buf)


def _tails_untouched(out, R):
    assert bool((out.qt_buf[R:] == SENTINEL).all()), "q_tot written past the last row"
    assert bool((out.dq_buf[R:] == SENTINEL).all()), "dq written past the last row"
    if out.q_tot is None:
        assert bool((out.qt_buf == SENTINEL).all())


def _oracle(family, mode, c, gamma=0.99):
    bf16 = family == "wide" and mode in (1, 3)
    return qo.loss_backward(c.P, c.s, c.q, c.q_tot_tgt, c.r, c.term, c.padded, gamma, bf16=bf16, wgrad_fp32=(family == "wide" and mode == 1))


def _check_against_oracle(family, mode, c, out, o, fill=(3.0, 5.0)):
    R = c.R
    maxabs = lambda t: max(1.0, float(t.abs().max()))
    # ---- q_tot, dq: 1e-4 of scale
    tol_q = 1e-4 * maxabs(o.q_tot)
    got_q, got_dq = out.q_tot.cpu().double(), out.dq.cpu().double()
    print("\n%s %s R=%d: q_tot err %.3g / %.3g, dq err %.3g / %.3g" % (
        family, mode, R, float((got_q - o.q_tot).abs().max()), tol_q, float((got_dq - o.dq).abs().max()), 1e-4 * maxabs(o.dq)))
    close(got_q, o.q_tot, tol_q, 1e-4, msg="q_tot")
    close(got_dq, o.dq, 1e-4 * maxabs(o.dq), 1e-4, msg="dq")
    pad = c.padded.bool()
    assert bool((got_dq[pad] == 0).all()), "dq of a padded row"
    # ---- loss2
    l2 = out.loss2.cpu().double() - torch.tensor(fill, dtype=torch.float64)
    bound = qo.loss0_bound(o, tol_q)
    print("   loss2[0] %.9g want %.9g (bound %.3g), sum(mask) %g" % (float(l2[0]), float(o.loss2[0]), bound, float(l2[1])))
    assert float(l2[1]) == float(o.loss2[1]), "sum(mask)"
    # loss2[0] comes back as fp32(fill + value): one more rounding of the stored sum, 2^-24 relative
    assert abs(float(l2[0]) - float(o.loss2[0])) <= bound + 2.0 ** -24 * (fill[0] + float(o.loss2[0])), "sum td^2"
    # ---- gradients, kinked columns left out of their own segment's weight and bias gradient
    kink = qo.kink_columns(o.hyper)
    nk = sum(int(v.sum()) for v in kink.values())
    bf = family == "wide" and mode in (1, 3)
    assert nk <= (qo.KINK_CAP_32775_BF16 if (bf and R == 32775) else qo.KINK_CAP), nk
    loose = family == "wide" and mode == 3
    for k in qo.NAMES:
        want = o.grads[k]
        got = out.G[k].cpu().double() - c.base[k].double()
        seg = k[:-2] if k.endswith("_b") else k
        if seg in kink and bool(kink[seg].any()):
            keep = ~kink[seg]
            want, got = want[keep], got[keep]
        sc = maxabs(want)
        if family == "fused":
            atol, rtol = 2e-4 * max(1.0, (R / 64.0) ** 0.5) * sc, 1e-4
        else:
            atol, rtol = (2e-2 if loose and k in qo.SEGMENTS else 1e-4) * sc, (2e-2 if loose else 1e-4)
        print("   %-5s err %.3g / %.3g (scale %.3g)" % (k, float((got - want).abs().max()), atol, sc))
        close(got, want, atol, rtol, msg=k)


def _run_case(dev, family, mode, shape, seed, remap=False, gamma=0.99):
    c = qo.make_case(*shape, seed)
    d = _upload(dev, family, c, remap=remap)
    out = _call(dev, family, mode, c, d, gamma=gamma, base=c.base)
    _tails_untouched(out, c.R)
    _check_against_oracle(family, mode, c, out, _oracle(family, mode, c, gamma))


# ------------------------------------------------------------------------------------------------ against the float64 oracle
@pytest.mark.parametrize("mode", ["f32", "bf16x6"])
@pytest.mark.parametrize("R,N,S,seed", qo.FUSED_CASES, ids=lambda v: str(v))
def test_fused_loss_bwd(dev, R, N, S, seed, mode):
    """registers-resident kernel (2s3z / 3s5z-sized states): one 16-row tile per workgroup up to 256 workgroups - single rows,
    tile tails, a second and third tile in a workgroup, 7.5 passes of the grid; both arithmetic modes (the split one keeps
    KR = 2 instead of 3 k chunks in registers in this variant only)"""
    _run_case(dev, "fused", mode, (R, N, S), seed)


def _wide_params():
    out = []
    for R, N, S, seed, seed_bf in qo.WIDE_CASES:
        out.append(pytest.param(R, N, S, seed, 0, id="%d-%d-%d-flags0" % (R, N, S)))
        if seed_bf is not None:
            out += [pytest.param(R, N, S, seed_bf, f, id="%d-%d-%d-flags%d" % (R, N, S, f)) for f in (3, 1)]
    return out


@pytest.mark.parametrize("R,N,S,seed,flags", _wide_params())
def test_wide_loss_bwd(dev, R, N, S, seed, flags):
    """streamed-weights kernel (MMM2-sized states): 128 rows per block up to 256 blocks - block tails, narrower hypernets, a
    second pass of the grid with a 7-row tail; fp32, bf16 operands in both GEMMs (flags 3: reference with both operands rounded to
    bf16, weight gradient on the rounded states at 2e-2) and in the forward GEMM only (flags 1: weight gradient in fp32 on the
    unrounded states, 1e-4)"""
    _run_case(dev, "wide", flags, (R, N, S), seed)


@pytest.mark.parametrize("family,mode", [("fused", "f32"), ("fused", "bf16x6"), ("wide", 0), ("wide", 3), ("wide", 1)])
def test_loss_bwd_reads_states_in_place_like_the_learner(dev, family, mode):
    """the states as a replay sample has them: (T + 1)-slot storage of 43 episodes, 36 of them read through an episode map with
    a slot offset of 1 (ops.Rows), T = 120 -> 4320 rows"""
    R, N, S, seed = qo.REMAP_CASES[family]
    _run_case(dev, family, mode, (R, N, S), seed, remap=True)


@pytest.mark.parametrize("family,mode,shape,seed", [("fused", "f32", (333, 5, 120), 458), ("wide", 0, (333, 10, 322), 665)])
def test_loss_bwd_gamma_zero(dev, family, mode, shape, seed):
    """gamma = 0: the target is the reward alone"""
    _run_case(dev, family, mode, shape, seed, gamma=0.0)


# ------------------------------------------------------------------------------------------------ contract (include/marl_hip.h)
# two row counts per family: one a multiple of 16 (the last q_tot tile of the fused kernel goes out as 16-byte stores), one not
CONTRACT = [("fused", "f32", (320, 5, 120)), ("fused", "bf16x6", (320, 5, 120)), ("fused", "f32", (4099, 3, 48)),
            ("fused", "bf16x6", (4099, 3, 48)), ("wide", 0, (333, 10, 322)), ("wide", 3, (333, 10, 322)),
            ("wide", 0, (4096, 10, 322)), ("wide", 3, (4096, 10, 322))]
contract = pytest.mark.parametrize("family,mode,shape", CONTRACT, ids=lambda v: str(v).replace(" ", ""))


def _setup(dev, family, shape):
    c = qo.make_case(*shape, seed=sum(shape))
    assert c.padded.sum() > 0 and (c.term * (1 - c.padded)).sum() > 0
    return c, _upload(dev, family, c)


def _same_bits(a, b, what, q_tot=True):
    assert torch.equal(a.dq, b.dq), what + ": dq"
    assert torch.equal(a.loss2, b.loss2), what + ": loss2"
    if q_tot:
        assert torch.equal(a.q_tot, b.q_tot), what + ": q_tot"
    for k in qo.NAMES:
        assert torch.equal(a.G[k], b.G[k]), what + ": " + k


@contract
def test_padded_rows_contribute_nothing(dev, family, mode, shape):
    """r and q_tot_tgt of padded rows at +-1e6 (finite): dq there is exactly 0; loss2 and every gradient equal the run with zeros
    there, bit for bit"""
    c, d = _setup(dev, family, shape)
    pad = d.padded.bool()
    zero = torch.zeros_like(d.r)
    a = _call(dev, family, mode, c, d, base=c.base, r=torch.where(pad, zero, d.r), tgt=torch.where(pad, zero, d.tgt))
    b = _call(dev, family, mode, c, d, base=c.base, r=torch.where(pad, zero + 1e6, d.r), tgt=torch.where(pad, zero - 1e6, d.tgt))
    assert bool((b.dq[pad] == 0).all()) and bool((a.dq[pad] == 0).all())
    assert bool((b.dq[~pad].abs().sum(1) > 0).all())
    _same_bits(a, b, "padded rows", q_tot=True)


@contract
def test_terminated_rows_ignore_the_target_network(dev, family, mode, shape):
    """changing q_tot_tgt on rows with term = 1 changes nothing, bit for bit"""
    c, d = _setup(dev, family, shape)
    a = _call(dev, family, mode, c, d, base=c.base)
    b = _call(dev, family, mode, c, d, base=c.base, tgt=torch.where(d.term.bool(), d.tgt * -3.0 + 11.0, d.tgt))
    _same_bits(a, b, "terminated rows")
    z = _call(dev, family, mode, c, d, base=c.base, tgt=d.tgt + 1.0)                  # ... while rows that go on do read it
    assert not torch.equal(z.dq, a.dq)


@contract
def test_outputs_accumulate(dev, family, mode, shape):
    """loss2 pre-filled with (3, 5) and gradients with a random base come back as base + value; a second call adds the value
    again (to fp32 rounding of the sums: 2^-23 of the largest term, two roundings)"""
    c, d = _setup(dev, family, shape)
    v = _call(dev, family, mode, c, d, base=None, fill=(0.0, 0.0))                      # the value alone
    a = _call(dev, family, mode, c, d, base=c.base, fill=(3.0, 5.0))
    once = {k: a.G[k].clone() for k in qo.NAMES}
    once_l = a.loss2.clone()
    b = _call(dev, family, mode, c, d, into=a)
    rnd = 2.0 ** -23
    for k in qo.NAMES:
        base = cu(c.base[k], dev)
        big = float(torch.maximum(base.abs(), v.G[k].abs()).max()) * 2.0 + 1.0
        close(once[k], base + v.G[k], rnd * big, 0, msg=k + " once")
        close(b.G[k], base + 2.0 * v.G[k], 2 * rnd * big, 0, msg=k + " twice")
    fill = torch.tensor([3.0, 5.0], device=dev)
    big = float(v.loss2.max()) * 2.0 + 5.0
    close(once_l, fill + v.loss2, rnd * big, 0, msg="loss2 once")
    close(b.loss2, fill + 2.0 * v.loss2, 2 * rnd * big, 0, msg="loss2 twice")
    assert float(b.loss2[1]) == 5.0 + 2.0 * float((1 - c.padded).sum())
    assert torch.equal(a.dq, v.dq) and torch.equal(a.q_tot, v.q_tot)                 # ... which are written, not accumulated


@contract
def test_q_tot_is_optional(dev, family, mode, shape):
    """q_tot = NULL gives bitwise the same dq, gradients and loss2"""
    c, d = _setup(dev, family, shape)
    a = _call(dev, family, mode, c, d, base=c.base)
    b = _call(dev, family, mode, c, d, base=c.base, with_q_tot=False)
    _tails_untouched(b, c.R)
    _same_bits(a, b, "q_tot = None", q_tot=False)


@contract
def test_no_stray_writes_and_fixed_summation_order(dev, family, mode, shape):
    """nothing is written past the last row of q_tot and dq (the 16-byte q_tot stores of the fused kernel and its scalar tail),
    every row is written, and two calls on the same inputs give bitwise equal outputs (the header promises a fixed order)"""
    c, d = _setup(dev, family, shape)
    a = _call(dev, family, mode, c, d, base=c.base)
    _tails_untouched(a, c.R)
    assert bool((a.q_tot != SENTINEL).all()) and bool((a.dq != SENTINEL).all())
    b = _call(dev, family, mode, c, d, base=c.base)
    _same_bits(a, b, "second call")


@pytest.mark.parametrize("x6", [False, True], ids=["f32", "bf16x6"])
@pytest.mark.parametrize("shape", [(320, 5, 120), (4099, 3, 48)], ids=lambda v: str(v).replace(" ", ""))
def test_fused_entry_refuses_a_misaligned_q_tot(dev, shape, x6):
    """the fused kernel stores q_tot 16 bytes per lane: a q_tot that is offset by 4 bytes is refused with a non-zero return before
    anything is launched - every output buffer keeps its contents"""
    from marl_amd import _lib, ops
    c, d = _setup(dev, "fused", shape)
    R, N, S = shape
    lib = _lib.load()
    G = {k: cu(c.base[k], dev) for k in qo.NAMES}
    loss2 = torch.tensor([3.0, 5.0], device=dev)
    qt_buf = torch.full((R + 16,), SENTINEL, device=dev)
    dq = torch.full((R, N), SENTINEL, device=dev)
    ws = ops.WS.get("qmix_fused", lib.marl_qmix_fused_workspace(R, N, S), dev)
    w, gw = ops.qmix_weights(d.W), ops.qmix_weights(G)
    fn = lib.marl_qmix_fused_loss_bwd_x6 if x6 else lib.marl_qmix_fused_loss_bwd
    q_tot = qt_buf[1:R + 1]
    assert q_tot.data_ptr() % 16 == 4
    rc = fn(C.byref(w), C.byref(d.xs), ops._p(d.q), ops._p(d.tgt), ops._p(d.r), ops._p(d.term), ops._p(d.padded), 0.99,
            ops._p(q_tot), ops._p(dq), C.byref(gw), ops._p(loss2), ops._p(ws), ws.numel() * 4, R, N, S, E, ops._stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert bool((qt_buf == SENTINEL).all()) and bool((dq == SENTINEL).all())
    assert loss2.tolist() == [3.0, 5.0]
    for k in qo.NAMES:
        assert torch.equal(G[k], cu(c.base[k], dev)), k


@contract
def test_agrees_with_the_unfolded_kernels(dev, family, mode, shape):
    """*_fwd + ops.td_loss + *_bwd on the same inputs: q_tot, dq, gradients and sum td^2 within 2e-6 of scale (the bound
    test_qmix_loss_folded_into_the_mixer_backward holds the two paths to: they differ in the summation order of q_tot between the
    forward and the backward kernel and of the partial sums of the loss; scale = the largest entry of q_tot, of dq, and of
    the ten gradient tensors together, as that test scales by the whole gradient vector), sum(mask) exactly"""
    from marl_amd import ops
    c, d = _setup(dev, family, shape)
    R, N, S = shape
    a = _call(dev, family, mode, c, d, base=None, fill=(0.0, 0.0))
    G = {k: torch.zeros(v.shape, device=dev) for k, v in c.P.items()}
    q_tot = torch.full((R,), SENTINEL, device=dev)
    dq_tot = torch.full((R,), SENTINEL, device=dev)
    dq = torch.full((R, N), SENTINEL, device=dev)
    loss2 = torch.zeros(2, device=dev)
    w, gw = ops.qmix_weights(d.W), ops.qmix_weights(G)
    if family == "fused":
        x6 = mode == "bf16x6"
        ops.qmix_fused_fwd(w, d.xs, d.q, q_tot, R, N, S, E, x6=x6)
        ops.td_loss(q_tot, d.tgt, d.r, d.term, d.padded, 0.99, dq_tot, loss2, R)
        ops.qmix_fused_bwd(w, d.xs, d.q, dq_tot, dq, gw, R, N, S, E, x6=x6)
    else:
        kw = WIDE_MODE[mode]
        ops.qmix_wide_fwd(w, d.xs, d.q, q_tot, R, N, S, E, bf16=kw["bf16"])
        ops.td_loss(q_tot, d.tgt, d.r, d.term, d.padded, 0.99, dq_tot, loss2, R)
        ops.qmix_wide_bwd(w, d.xs, d.q, dq_tot, dq, gw, R, N, S, E, **kw)
    torch.cuda.synchronize()
    assert float(a.loss2[1]) == float(loss2[1]) == float((1 - c.padded).sum())
    np.testing.assert_allclose(float(a.loss2[0]), float(loss2[0]), rtol=2e-6)
    close(a.q_tot, q_tot, 2e-6 * float(q_tot.abs().max()), 0, msg="q_tot")
    close(a.dq, dq, 2e-6 * float(dq.abs().max()), 0, msg="dq")
    scale = max(float(G[k].abs().max()) for k in qo.NAMES)
    for k in qo.NAMES:
        close(a.G[k], G[k], 2e-6 * scale, 0, msg=k)
