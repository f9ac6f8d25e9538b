"""The forward agent unroll - marl_agent_unroll_fwd (csrc/agent.hip: the software-pipelined and the multi-tile kernel) and
marl_agent_unroll_fwd_x6 (csrc/agent_x6.hip, csrc/agent_x6p.hip) - against the float64 statement of the operation
(tests/unroll_oracle.py), at every launch plan and at the input widths where the instantiations change.  Needs a real MI355X:
``pytest -m gpu``.

Cases (unroll_oracle.CASES) are the smallest row counts that reach each branch of the launch code (unroll_oracle.FAMILIES names them);
every test first ASKS THE LIBRARY which plan it will run (marl_agent_unroll_fwd_plan: the host function the launch itself calls) and
fails with "the plan moved" when that is not the plan the row count was picked for.

Per case: (T+1)-slot storage holding more episodes than the batch, read through a permuting ep_map; ragged ep_len that includes 1 and
T and differs between rows of one tile; fed actions with -1 entries, u_t0 = -1 for eval passes and 0 for continuations; a non-zero
h0.  Outputs start as NaN in allocations 16 rows longer whose tails hold a sentinel: the tails must be untouched and nothing inside
left NaN.  q, hs, h_last - and for saving launches the six saved planes and the three gate sums (the fp32 kernels' pre-scaled ones
divided by the factors unroll_oracle.gate_sum_scale reads from csrc/common.h) - are held to float64.  A continuation that reads
gi_in equals the same launch computing everything bit for bit, and its q is held to float64 too.  The same launch without hs /
without h_last gives the same q bit for bit wherever the plan query says the plan is the same; without ufed (and without gi_in: the stored sums hold the fed
actions' columns) it is held to the oracle without fed actions.  h_last aliasing h0 gives the same h_last and q, once per kernel family, entry and launch kind.

Bound (not new): |got - want| <= 1e-4 s + 1e-4 |want|, s = max(1, max|want|) - VALUE_TOL of tests/test_gpu_bptt.py, what
test_agent_unroll_fwd holds q to - for every tensor, in both arithmetic modes; nothing is left out of a comparison.  Every test
prints, per tensor, the kernel's scaled error beside the scaled error of fp32 torch-CPU on the same inputs (DESIGN.md has the table)."""
import numpy as np
import pytest
import torch

import unroll_oracle as uo

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
VALUE_TOL = (1e-4, 1e-4)
PLANES = ("hprev", "x", "r", "z", "n", "hn")
GATES = ("gi_r", "gi_z", "gi_n")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from marl_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def cu(x, dev, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x)).to(dtype).to(dev).contiguous()


def _off_buffer(n, off, dev, fill=float("nan")):
    """n floats that start `off` floats past a 16-byte boundary"""
    raw = torch.full((n + 8,), fill, device=dev)
    lead = (-(raw.data_ptr() // 4)) % 4          # floats up to the next 16-byte boundary
    t = raw[lead + off:lead + off + n]
    assert t.data_ptr() % 16 == 4 * off
    return t


def _out(rows, cols, off, dev):
    """(rows + 16, cols): NaN inside, the sentinel in the 16 rows past the end"""
    t = _off_buffer((rows + 16) * cols, off, dev).view(rows + 16, cols)
    t[rows:] = SENTINEL
    return t


class Inputs:
    """the inputs of one case key on the host and on the device, and the float64 / fp32 CPU unrolls asked for so far"""

    def __init__(self):
        self.key = None

    def get(self, c, dev):
        if self.key != (c.key, c.obs_off):
            self.key, self.memo = (c.key, c.obs_off), {}
            self.inp = i = uo.make_inputs(c)
            self.store = _off_buffer(i.store.size, 1 if c.obs_off else 0, dev)
            self.store.copy_(cu(i.store.reshape(-1), dev))
            self.u, self.emap, self.lens = cu(i.u, dev, torch.int32), cu(i.emap, dev, torch.int32), cu(i.lens, dev, torch.int32)
            self.p = {n: cu(v, dev) for n, v in i.p.items()}
        return self

    def want(self, T, t0, u_t0, h0, with_u=True):
        """(float64 unroll, fp32 torch-CPU unroll) of one launch"""
        k = (t0, u_t0, with_u, h0.tobytes() if h0 is not self.inp.h0 else "h0")
        if k not in self.memo:
            self.memo[k] = (uo.forward(self.inp, T, t0, u_t0, h0, with_u=with_u), uo.forward(self.inp, T, t0, u_t0, h0, torch.float32, with_u=with_u))
        return self.memo[k]


INPUTS = Inputs()


def _launch(dev, c, d, kind, t0, u_t0, h0_np, gi_in=None, hs=True, h_last=True, with_u=True, alias=False):
    """one launch of the case's entry point -> the outputs on the host (with their 16 extra rows) and, for saving launches, the
    decoded planes and the gate-sum buffer"""
    from marl_amd import ops
    B, T, N, O, A, R = c.B, c.T, c.N, c.O, c.A, c.R
    M = B * T * N
    off = 1 if c.h_off else 0
    w = ops.agent_weights(d.p)
    q = _out(M, A, 0, dev)
    hs_b = _out(M, 64, 0, dev) if hs else None
    h0_b = _out(R, 64, off, dev)
    h0_b[:R] = cu(h0_np, dev)
    hl_b = h0_b if alias else (_out(R, 64, off, dev) if h_last else None)
    saved = gi = None
    if kind == "save":
        shp, gshp = ops.saved_shape(T, B, N), ops.saved_shape(T, B, N, planes=3)
        saved, gi = _out(int(np.prod(shp)) // 64, 64, 0, dev), _out(int(np.prod(gshp)) // 64, 64, 0, dev)
    fn = ops.agent_unroll_fwd_x6 if c.entry == "x6" else ops.agent_unroll_fwd
    fn(w, d.store, (T + 1) * N, t0, d.u if with_u else None, T * N, u_t0, h0_b[:R], q[:M], hs_b[:M] if hs else None,
       hl_b[:R] if hl_b is not None else None, saved[:-16].view(shp) if saved is not None else None, B, T, N, O, A,
       last_action=bool(c.la), reuse_network=bool(c.rn), ep_len=d.lens, ep_map=d.emap, cu_budget=c.cus,
       gi_out=gi[:-16].view(gshp) if gi is not None else None, gi_in=gi_in)
    torch.cuda.synchronize()
    out = {"q": (q.cpu(), M)}
    if hs:
        out["hs"] = (hs_b.cpu(), M)
    if hl_b is not None:
        out["h_last"] = (hl_b.cpu(), R)
    res = {}
    for n, (t, rows) in out.items():
        # nothing is written past the last row, nothing inside is left unwritten
        assert bool((t[rows:] == SENTINEL).all()), "%s: rows past the end of %s were written" % (uo.case_id(c), n)
        assert not torch.isnan(t[:rows]).any(), "%s: NaN in %s" % (uo.case_id(c), n)
        res[n] = t[:rows]
    res["q"], res["hs"] = res["q"].view(B, T, N, A), res["hs"].view(B, T, N, 64) if hs else None
    if saved is not None:
        assert bool((saved[-16:] == SENTINEL).all()) and bool((gi[-16:] == SENTINEL).all()), uo.case_id(c) + ": written past the end of saved / gi_out"
        sv, g = saved[:-16].view(shp), gi[:-16].view(gshp)
        res["planes"] = [ops.saved_plane(sv, k, R).cpu()[:T + (1 if k == 0 else 0)] for k in range(6)]
        res["gi"] = [ops.saved_plane(g, k, R).cpu() for k in range(3)]
        res["gi_dev"] = g
    return res


def _compare(label, name, got, want, ref, fails, tol=VALUE_TOL):
    """got vs want at |got - want| <= atol s + rtol |want|, s = max(1, max|want|); prints the scaled error beside fp32 torch-CPU's"""
    atol, rtol = tol
    assert got.shape == want.shape, (label, name, got.shape, want.shape)
    assert not torch.isnan(got).any(), "%s: NaN in %s" % (label, name)
    want = want.double()
    s = max(1.0, float(want.abs().max()))
    diff = (got.double() - want).abs()
    err, worst = float(diff.max()) / s, float((diff / (atol * s + rtol * want.abs())).max())
    ref_err = uo.scaled_err(ref, want)
    print("UNROLL %-62s %-8s kernel %.2e  fp32-cpu %.2e  bound %.0e  (%.1f %% of it)" % (label, name, err, ref_err, atol, 100 * worst))
    if not worst <= 1.0:
        fails.append("%s %s: scaled error %.3e (fp32 torch-CPU: %.3e), %.2f x the bound %g + %g |want|" % (label.split("] ")[-1] if "] " in label else "", name, err, ref_err, worst, atol, rtol))


def _compare_all(label, c, got, w64, w32, fails):
    _compare(label, "q", got["q"], w64.q, w32.q, fails)
    if got.get("hs") is not None:
        _compare(label, "hs", got["hs"], w64.hs, w32.hs, fails)
    if "h_last" in got:
        _compare(label, "h_last", got["h_last"], w64.h_last, w32.h_last, fails)
    if "planes" in got:
        for k, n in enumerate(PLANES):
            _compare(label, n, got["planes"][k], w64.planes[k], w32.planes[k], fails)
        scale = uo.gate_sum_scale(c.A, c.entry)
        for k, n in enumerate(GATES):
            _compare(label, n, got["gi"][k].double() / scale[k], w64.gi[k], w32.gi[k], fails)


def _alias_cases():
    """the cases that also run with h_last aliasing h0: the ones the table marks, and the first of every (entry, family, input path,
    launch kind)"""
    seen, out = set(), set()
    for c in uo.CASES:
        k = (c.entry, c.plan[0], c.plan[6], c.kind)
        if c.alias or k not in seen:
            out.add(uo.case_id(c))
        seen.add(k)
    return out


ALIAS = _alias_cases()


@pytest.mark.parametrize("c", [pytest.param(c, id=uo.case_id(c)) for c in uo.CASES])
def test_unroll_against_float64(dev, c):
    plan = uo.query(c)
    assert plan == c.plan, "the plan moved, re-pick the row count: %s runs %s, this case was picked for %s" % (
        uo.case_id(c), uo.plan_id(plan) if plan else plan, uo.plan_id(c.plan))
    d = INPUTS.get(c, dev)
    T = c.T
    label = uo.case_id(c) + " " + uo.plan_id(plan)
    fails = []
    if c.kind == "cont":
        # eval pass over slots 0..T-1 (u_t0 = -1) that stores the gate sums, then slots 1..T (u_t0 = 0) from its h_last
        ev = _launch(dev, c, d, "save", 0, -1, d.inp.h0)
        h0 = ev["h_last"].numpy().copy()
        t0, u_t0, extra = 1, 0, dict(gi_in=ev["gi_dev"])
        main = _launch(dev, c, d, "cont", t0, u_t0, h0, **extra)
        full = _launch(dev, c, d, "plain", t0, u_t0, h0)
        for n in ("q", "hs", "h_last"):
            assert torch.equal(main[n], full[n]), "%s: %s of the launch reading gi_in differs from the launch computing everything" % (label, n)
    else:
        h0, t0, u_t0, extra = d.inp.h0, 0, -1, {}
        main = _launch(dev, c, d, c.kind, t0, u_t0, h0, hs=c.kind != "nohs")
    w64, w32 = d.want(T, t0, u_t0, h0)
    _compare_all(label, c, main, w64, w32, fails)
    # optional outputs: same q bit for bit where the plan is the same; in any case held to float64
    for name, kw in (("no-hs", dict(hs=False)), ("no-h_last", dict(h_last=False))):
        if c.kind == "nohs" and name == "no-hs":
            continue
        v = _launch(dev, c, d, c.kind, t0, u_t0, h0, **dict(dict(extra, hs=c.kind != "nohs"), **kw))
        if uo.query(c, hs=kw.get("hs", c.kind != "nohs")) == plan:
            assert torch.equal(v["q"], main["q"]), "%s: q changes when the launch gets %s" % (label, name)
        _compare_all(label + " " + name, c, v, w64, w32, fails)
    # (without gi_in: the stored sums hold the fed actions' columns)
    v = _launch(dev, c, d, "plain" if c.kind == "cont" else c.kind, t0, u_t0, h0, with_u=False, hs=c.kind != "nohs")
    n64, n32 = d.want(T, t0, u_t0, h0, with_u=False)
    _compare_all(label + " no-ufed", c, v, n64, n32, fails)
    if uo.case_id(c) in ALIAS:
        v = _launch(dev, c, d, c.kind, t0, u_t0, h0, alias=True, **dict(extra, hs=c.kind != "nohs"))
        assert torch.equal(v["h_last"], main["h_last"]) and torch.equal(v["q"], main["q"]), label + ": h_last aliasing h0 changes the result"
    assert not fails, label + ": " + "; ".join(fails)


def test_refusals_return_before_any_launch(dev):
    """host-side argument checks of the two entry points: the split entry with a misaligned obs, A = 33, A = 17 at 160 columns"""
    from marl_amd import ops, _lib
    from oracle import seeded
    c = uo._c("2s3z", 4, 4, 0, "plain", "x6", (0,) * 8, obs_off=1)
    d = INPUTS.get(c, dev)
    R = c.B * 7
    h0 = torch.zeros(R, 64, device=dev)
    big = torch.zeros(8 * 5 * 8 * 136, device=dev)

    def refused(fn, x6, obs, N, O, A, **flags):
        """weights of the shape asked for; the plan query refuses, the entry point raises, nothing is written"""
        assert ops.agent_unroll_fwd_plan(x6, c.B, c.T, N, O, A, **flags) is None
        args = seeded.make_args("2s3z", "qmix", episode_limit=c.T, n_agents=N, obs_shape=O, n_actions=A)
        w = ops.agent_weights({n: cu(v, dev) for n, v in seeded.seeded_state(seeded.agent_param_shapes(args), seed=1).items()})
        M = c.B * c.T * N
        q, hl = _out(M, A, 0, dev), _out(c.B * N, 64, 0, dev)
        with pytest.raises(_lib.MarlHipError):
            fn(w, obs, (c.T + 1) * N, 0, None, c.T * N, -1, h0[:c.B * N], q[:M], None, hl[:c.B * N], None, c.B, c.T, N, O, A, ep_len=d.lens, ep_map=d.emap)
        torch.cuda.synchronize()
        assert torch.isnan(q[:M]).all() and torch.isnan(hl[:c.B * N]).all() and bool((q[M:] == SENTINEL).all()), "a refused call wrote its outputs"

    assert uo.query(c) is None
    refused(ops.agent_unroll_fwd_x6, True, d.store, c.N, c.O, c.A, obs_aligned=False)      # obs one float past a 16-byte boundary
    refused(ops.agent_unroll_fwd_x6, True, big, 5, 80, 33)                                 # A = 33
    refused(ops.agent_unroll_fwd, False, big, 5, 80, 33)
    assert 136 + 17 + 7 == 160
    refused(ops.agent_unroll_fwd_x6, True, big, 7, 136, 17)                                # A = 17 at 160 input columns: one action tile only
