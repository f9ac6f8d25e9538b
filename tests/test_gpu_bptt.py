"""Backward-through-time of the agent unroll - the fp32 kernels of csrc/agent.hip (agent_bwd_pipe_kernel: sparse dq, up to four row
tiles per workgroup, T >= 2; agent_bwd_kernel: everything else) and the bf16x6 split kernel of csrc/agent_bwd_x6.hip - against the
float64 statement of the operation (tests/bptt_oracle.py), at every launch plan.  Needs a real MI355X: ``pytest -m gpu``.

Cases (bptt_oracle.CASES) are the smallest row counts that reach each branch of the launch code: the split kernel's one-tile plan at
its upper edge (256 tiles), all two-tile workgroups with a last one that has no second tile (257, 769 tiles), the mixed plan - a
second launch of one-tile workgroups at tile_base = 2 n2, slab_base = n2 - with 1, 2, 8 and 256 workgroups in it (one of them
holding ONE row); the fp32 kernels at 1 to 6 row tiles per workgroup (6 is the most LDS allows), with a last workgroup that holds
fewer tiles than the others; two action tiles (MMM2); T = 2 (the pipelined kernel's minimum), T = 40.  Every test first ASKS THE
LIBRARY which plan it will run (workspace bytes / bytes of one slab) and fails with "the plan moved" when that is not the plan the
row count was picked for.

Per case and kernel: one sparse pair per row ("s1"), two pairs + an external gradient on hs ("s2h", the QTRAN form), a dense dq +
that gradient ("dense", fp32 kernels only: selects the two-phase kernel), and the seam probe.  The forward (ops.agent_unroll_fwd)
starts from a non-zero h0; dxp and dh0 start as NaN in allocations 16 rows longer whose tail holds a sentinel; the gradients start
from a non-zero base; the fc1 gradient is built from dxp with ops.linear_wgrad as the learner builds it.

Seam probe: dq is exactly 0 except on ~10-20 rows - the first and the last row and the two rows either side of the first tile seam,
of the first and the last workgroup seam of either kernel and of the split kernel's launch seam.  Each gradient is then a sum over
those rows only, so a dropped, doubled or misplaced row moves it by order 1 however the bounds are set; dxp and dh0 of every other
row must be bitwise zero (no leakage across rows), the 16 rows past the end untouched.

Bounds (none of them new): gradients, after dividing by max(1, max|want|): atol 2e-4, rtol 1e-3 (test_agent_unroll_bwd,
test_agent_unroll_bwd_x6_split); q, dxp, dh0: 1e-4 of max(1, max|want|), rtol 1e-4 (what q holds in test_agent_unroll_fwd).  dxp
leaves out the elements bptt_oracle.kink_mask names (<= 1e-4 of them: tests/test_bptt_oracle_cpu.py).  Both arithmetic modes hold
the same bounds.  Every test prints, per tensor, the kernel's scaled error next to the scaled error of fp32 torch-CPU autograd on
the same inputs (DESIGN.md has the table).  One thing that yardstick shows: a forward that gates a kinked element the other way
moves fc1's two gradients by that element's dxp times its input row - fp32 torch-CPU does so once at 16385 rows (2.5e-3 of scale
on fc1.bias, 5.3e-3 on fc1.weight, every other tensor of that case at 4e-7); the kernels' forward gates every kinked element of these
seeds as float64 does.  A change of the forward's summation order that flips one is no defect: such a case gets another seed."""
import numpy as np
import pytest
import torch

import bptt_oracle as bo
from oracle import seeded

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
GRAD_TOL = (2e-4, 1e-3)
VALUE_TOL = (1e-4, 1e-4)
ORACLE = bo.Oracle()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from marl_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def cu(x, dev, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x)).to(dtype).to(dev).contiguous()


def _runs():
    """(case, form, kernel): case by case, so that the oracle keeps one case at a time"""
    out = []
    for c in bo.CASES:
        for form in c.forms:
            for kernel in ("x6", "f32"):
                if kernel == "x6" and (c.x6 is None or form == "dense"):
                    continue
                out.append(pytest.param(c, form, kernel, id="%s-%s-%s" % (bo.case_id(c), form, bo.plan_id(c, kernel))))
            if form == "probe":     # the same probe as a dense tensor: the two-phase fp32 kernel at every RT
                out.append(pytest.param(c, "probe", "f32-dense", id="%s-probe-dense-%s" % (bo.case_id(c), bo.plan_id(c, "f32"))))
    return out


def _assert_plan(c, kernel):
    """the library's own account of the plan: slabs of partial sums, one per workgroup"""
    from marl_amd import _lib
    lib = _lib.load()
    if kernel == "x6":
        from marl_amd import ops
        assert ops.agent_unroll_bwd_x6_supported(c.B, c.T, c.N, c.A)
        slabs, want = lib.marl_agent_bwd_x6_workspace(c.B, c.N, c.A) / lib.marl_agent_bwd_x6_workspace(1, 1, c.A), sum(c.x6)
        assert bo.bx6_plan(c.R) == c.x6, "the plan mirror moved: bptt_oracle.bx6_plan(%d) = %r, case picked for %r" % (c.R, bo.bx6_plan(c.R), c.x6)
    else:
        slabs, want = lib.marl_agent_bwd_workspace(c.B, c.N, c.A) / lib.marl_agent_bwd_workspace(1, 1, c.A), c.f32[1]
        assert bo.f32_plan(c.R, c.A) == c.f32, "the plan mirror moved: bptt_oracle.f32_plan(%d, %d) = %r, case picked for %r" % (c.R, c.A, bo.f32_plan(c.R, c.A), c.f32)
    assert slabs == want, ("the plan moved, re-pick the row count: %s runs %g workgroups on %d rows (A = %d), this case was picked for %d (%s)"
                           % (kernel, slabs, c.R, c.A, want, bo.plan_id(c, kernel)))


def _fc1_input(args, obs_d, u_d, M):
    """the fc1 weight gradient's input rows as the learner builds them (tests/test_gpu_kernels.py:_fc1_input)"""
    from marl_amd import ops
    N, O, A = args.n_agents, args.obs_shape, args.n_actions
    kw = dict(idx=u_d.view(M, 1), nhot=1, hot_w=A) if args.last_action else {}
    I = O + (A if args.last_action else 0) + (N if args.reuse_network else 0)
    assert I == seeded.agent_param_shapes(args)[0][1][1]
    return ops.src(obs_d.view(M, O), nid=N if args.reuse_network else 0, **kw), I


def _launch(dev, c, o, kernel):
    """forward from h0, then ONE backward call + the fc1 weight gradient.  -> q, grads - base (float64), dxp and dh0 buffers"""
    from marl_amd import ops
    k, d = o.k, o.d
    args = k.args
    B, T, N, A, O, R = c.B, c.T, c.N, c.A, k.args.obs_shape, c.R
    M = B * T * N
    pd = {n: cu(v, dev) for n, v in k.p.items()}
    w = ops.agent_weights(pd)
    q, hs = torch.empty(B, T, N, A, device=dev), torch.empty(B, T, N, 64, device=dev)
    saved = torch.empty(ops.saved_shape(T, B, N), device=dev)
    obs_d, u_d = cu(k.obs, dev), cu(k.ufed, dev, torch.int32)
    ops.agent_unroll_fwd(w, obs_d, T * N, 0, u_d, T * N, 0, cu(k.h0, dev), q, hs, None, saved, B, T, N, O, A,
                         last_action=args.last_action, reuse_network=args.reuse_network)
    g = torch.Generator().manual_seed(9)
    base = {n: torch.randn(v.shape, generator=g) * 0.25 for n, v in k.p.items()}
    grads = {n: cu(v, dev) for n, v in base.items()}
    dxp = torch.full((M + 16, 64), float("nan"), device=dev)
    dh0 = torch.full((R + 16, 64), float("nan"), device=dev)
    dxp[M:] = SENTINEL
    dh0[R:] = SENTINEL
    i32 = lambda t: cu(t, dev, torch.int32) if t is not None else None
    f32 = lambda t: cu(t, dev) if t is not None else None
    sparse = {} if (d.form == "dense" or kernel == "f32-dense") else dict(dq_idx=i32(d.idx), dq_val=f32(d.val), dq_idx2=i32(d.idx2),
                                                                        dq_val2=f32(d.val2), dq_gdiv=d.gdiv)
    ops.agent_unroll_bwd(w, None if sparse else f32(d.full), f32(d.dhs), saved, hs, dxp[:M], dh0[:R], {n: grads[n] for n in bo.BWD_PARAMS},
                         B, T, N, A, x6=(kernel == "x6"), **sparse)
    fc1_in, I = _fc1_input(args, obs_d, u_d, M)
    ops.linear_wgrad(dxp[:M], fc1_in, grads["fc1.weight"], grads["fc1.bias"], M, 64, I)
    torch.cuda.synchronize()
    got = {n: grads[n].cpu().double() - base[n].double() for n in bo.PARAMS}
    return q.cpu(), got, dxp.cpu(), dh0.cpu()


def _compare(label, name, got, want, tol, ref_err, fails, keep=None):
    """got vs want at |got - want| <= atol s + rtol |want|, s = max(1, max|want|); prints the scaled error beside fp32 torch-CPU's"""
    atol, rtol = tol
    assert not torch.isnan(got).any(), "%s: NaN in %s" % (label, name)
    want = want.double()
    s = max(1.0, float(want.abs().max()))
    diff = (got.double() - want).abs()
    use = diff / (atol * s + rtol * want.abs())
    if keep is not None:
        diff, use = diff[keep], use[keep]
    err, worst = float(diff.max()) / s, float(use.max())
    print("BPTT %-58s %-14s kernel %.2e  fp32-cpu %.2e  bound %.0e  (%.1f %% of it)" % (label, name, err, ref_err, atol, 100 * worst))
    if not worst <= 1.0:
        fails.append("%s: scaled error %.3e (fp32 torch-CPU: %.3e), %.2f x the bound %g + %g |want|" % (name, err, ref_err, worst, atol, rtol))


@pytest.mark.parametrize("c,form,kernel", _runs())
def test_bptt_against_float64(dev, c, form, kernel):
    _assert_plan(c, "x6" if kernel == "x6" else "f32")
    o = ORACLE.get(c, form)
    q, got, dxp_buf, dh0_buf = _launch(dev, c, o, kernel)
    B, T, N, R = c.B, c.T, c.N, c.R
    M = B * T * N
    label = "%s %s %s" % (bo.case_id(c), form + ("-dense" if kernel == "f32-dense" else ""), bo.plan_id(c, "x6" if kernel == "x6" else "f32"))
    fails = []
    _compare(label, "q", q, o.want["q"], VALUE_TOL, o.ref_err["q"], fails)
    for n in bo.PARAMS:
        _compare(label, n, got[n], o.want[n], GRAD_TOL, o.ref_err[n], fails)
    dxp, dh0 = dxp_buf[:M].view(B, T, N, 64), dh0_buf[:R]
    _compare(label, "dxp", dxp, o.want["dxp"], VALUE_TOL, o.ref_err["dxp"], fails, keep=o.keep)
    _compare(label, "dh0", dh0, o.want["dh0"], VALUE_TOL, o.ref_err["dh0"], fails)
    assert not fails, label + ": " + "; ".join(fails)
    # nothing is written past the last row
    assert bool((dxp_buf[M:] == SENTINEL).all()) and bool((dh0_buf[R:] == SENTINEL).all()), label + ": rows past the end were written"
    if form == "probe":
        quiet = torch.ones(R, dtype=torch.bool)
        quiet[o.d.rows] = False
        assert bool((o.want["dxp"].permute(0, 2, 1, 3).reshape(R, T * 64)[quiet] == 0).all())
        leak = (dxp.permute(0, 2, 1, 3).reshape(R, T * 64)[quiet] != 0).any(1) | (dh0[quiet] != 0).any(1)
        assert not bool(leak.any()), "%s: rows with zero dq and zero carry got a gradient: %r (probe rows %r)" % (
            label, quiet.nonzero().flatten()[leak][:20].tolist(), o.d.rows)
        live = (dxp.permute(0, 2, 1, 3).reshape(R, T * 64)[o.d.rows] != 0).any(1) & (dh0[o.d.rows] != 0).any(1)
        assert bool(live.all()), "%s: probe rows without a gradient: %r" % (label, [r for r, l in zip(o.d.rows, live.tolist()) if not l])
