"""tests/unroll_oracle.py on the CPU: its case table is held to the library's own plan query (marl_agent_unroll_fwd_plan: a host
function, no GPU), reaches every launch plan the forward unroll has, and its float64 statement agrees with oracle/nets.agent_unroll."""
import numpy as np
import pytest
import torch

import unroll_oracle as uo
from oracle import nets

NEW_SHAPES = [s for s in uo.SHAPES if s not in uo.SCENARIOS]


def test_every_case_runs_the_plan_it_was_picked_for():
    from marl_amd import ops
    ids = [uo.case_id(c) for c in uo.CASES]
    assert len(set(ids)) == len(ids)
    for c in uo.CASES:
        got = uo.query(c)
        assert got == c.plan, "the plan moved, re-pick the row count: %s runs %s, picked for %s" % (
            uo.case_id(c), uo.plan_id(got) if got else got, uo.plan_id(c.plan))
        sup = ops.agent_unroll_x6_supported(c.B, max(c.T, 4), c.N, c.O, c.A, bool(c.la), bool(c.rn))
        assert sup == (c.shape not in uo.F32_ONLY), uo.case_id(c)
        assert c.entry == "f32" or sup
        assert c.entry == "f32" or not c.obs_off
        if c.kind == "nohs":
            assert got[0] == uo.R6, uo.case_id(c)
    for shape, (_, N, O, A) in uo.SHAPES.items():           # the widths the table names
        assert uo.width(shape) == O + A + N
    assert [uo.width(s) for s in ("i13", "i60", "i41n20", "2s3z", "i97", "i160", "i165a16", "i161a32", "o192", "i224", "i304")] == \
        [13, 60, 41, 96, 97, 160, 165, 161, 208, 224, 304]
    assert uo.width("i165a16", rn=0) == 160 and uo.width("i97", rn=0) == 91


def test_the_table_reaches_every_plan_family():
    missing = []
    for fam, pred in uo.FAMILIES.items():
        shapes = {c.shape for c in uo.CASES if pred(c, c.plan)}
        new = sorted(s for s in shapes if s in NEW_SHAPES)
        if not any(s in uo.SCENARIOS for s in shapes) or len(new) < 2:
            missing.append("%s: scenario %r, new %r" % (fam, sorted(s for s in shapes if s in uo.SCENARIOS), new))
    for fam, pred in uo.FAMILIES_ONCE.items():
        if not any(pred(c, c.plan) for c in uo.CASES):
            missing.append(fam)
    assert not missing, "plan families without their cases: " + "; ".join(missing)
    # every shape of the table runs on every entry point that takes it, flags off where the table says so
    for s in uo.SHAPES:
        assert any(c.shape == s and c.entry == "f32" for c in uo.CASES), s
        assert s in uo.F32_ONLY or any(c.shape == s and c.entry == "x6" for c in uo.CASES), s
    assert any(c.shape == "i165a16" and not c.rn and c.entry == "x6" and c.plan[5] == 5 and c.plan[4] == 1 for c in uo.CASES)
    assert any(c.shape == "i97" and not c.rn and c.entry == "x6" and c.plan[5] == 3 for c in uo.CASES)
    assert any(c.shape == "2s3z" and c.obs_off and c.plan[6] == uo.ELEMENT for c in uo.CASES)
    assert all(uo.query(c, kind=k) is not None for c in uo.CASES for k in ("plain", "save") if c.kind != "nohs")


def test_plan_query_refusals():
    """what the entry points refuse, the query refuses (host-side argument checks)"""
    from marl_amd import ops
    q = ops.agent_unroll_fwd_plan
    assert q(True, 8, 4, 5, 80, 11) is not None and q(True, 8, 4, 5, 80, 11, obs_aligned=False) is None
    assert q(False, 8, 4, 5, 80, 33) is None and q(True, 8, 4, 5, 80, 33) is None and q(False, 8, 4, 5, 80, 32) is not None
    assert q(True, 8, 4, 7, 136, 17) is None and ops.agent_unroll_x6_supported(8, 4, 7, 136, 17) is False      # A = 17 at 160 columns
    assert q(True, 8, 4, 8, 136, 17) is not None                                                             # ... 161 columns take it
    assert q(True, 8, 3, 5, 80, 11) is None and q(True, 8, 4, 5, 80, 11, saved=True, gi_in=True) is None
    assert q(False, 0, 4, 5, 80, 11) is None and q(False, 8, 4, 5, 80, 11, cu_budget=257) is None


@pytest.mark.parametrize("shape,la,rn", [("2s3z", 1, 1), ("MMM2", 1, 1), ("i41n20", 1, 0), ("o55", 0, 1)])
def test_float64_oracle_agrees_with_nets_agent_unroll(shape, la, rn):
    """the oracle's addressing + bptt_oracle.unroll against oracle/nets.agent_unroll in fp32 on inputs resolved by hand, at 1e-4;
    the saved vectors and gate sums against the definitions of include/marl_hip.h"""
    B, T = 7, 5
    c = uo._c(shape, B, T, 0, "plain", "f32", (0,) * 8, la=la, rn=rn)
    inp = uo.make_inputs(c)
    assert inp.lens[0] == T and inp.lens[-1] == 1 and len(set(inp.emap.tolist())) == B and inp.emap.max() >= B - 1
    assert (inp.u == -1).any() and (inp.u >= 0).any()
    N, O, A = c.N, c.O, c.A
    for t0, u_t0 in ((0, -1), (1, 0)):
        want = uo.forward(inp, T, t0, u_t0, inp.h0)
        # by hand: storage episode ep_map[b], slot t + t0, zeros from ep_len on; the action of slot t + u_t0
        obs = np.zeros((B, T, N, O), np.float32)
        oh = np.zeros((B, T, N, A), np.float32)
        for b in range(B):
            for t in range(T):
                if t < inp.lens[b]:
                    obs[b, t] = inp.store[inp.emap[b], t + t0]
                for n in range(N):
                    if t + u_t0 >= 0 and inp.u[b, t + u_t0, n] >= 0:
                        oh[b, t, n, inp.u[b, t + u_t0, n]] = 1
        p = {k: torch.tensor(v) for k, v in inp.p.items()}
        with torch.no_grad():
            q, hs, hl = nets.agent_unroll(p, torch.tensor(obs), torch.tensor(oh), torch.tensor(inp.h0), bool(la), bool(rn))
        for name, got, ref in (("q", q, want.q), ("hs", hs, want.hs), ("h_last", hl, want.h_last)):
            assert got.shape == ref.shape
            assert uo.scaled_err(got, ref) <= 1e-4, (name, uo.scaled_err(got, ref))
        f32 = uo.forward(inp, T, t0, u_t0, inp.h0, dtype=torch.float32)
        assert f32.q.dtype == torch.float32 and uo.scaled_err(f32.q, want.q) <= 1e-4
        # the saved vectors: hprev(t + 1) = hs(t) = (1 - z) n + z hprev; the sums rebuild r, z, n with the hidden side
        R = B * N
        hp, x, r, z, n, hn = want.planes
        assert hp.shape == (T + 1, R, 64) and all(v.shape == (T, R, 64) for v in (x, r, z, n, hn) + tuple(want.gi))
        hs_t = want.hs.permute(1, 0, 2, 3).reshape(T, R, 64)
        assert torch.equal(hp[0], torch.tensor(inp.h0, dtype=torch.float64)) and torch.equal(hp[1:], hs_t)
        assert torch.allclose((1 - z) * n + z * hp[:-1], hs_t, rtol=0, atol=1e-14)
        p64 = {k: torch.tensor(v, dtype=torch.float64) for k, v in inp.p.items()}
        whh, bhh = p64["rnn.weight_hh"], p64["rnn.bias_hh"]
        gh = hp[:-1] @ whh.T
        assert torch.allclose(torch.sigmoid(want.gi[0] + gh[..., :64]), r, rtol=0, atol=1e-14)
        assert torch.allclose(torch.sigmoid(want.gi[1] + gh[..., 64:128]), z, rtol=0, atol=1e-14)
        assert torch.allclose(hn, gh[..., 128:] + bhh[128:], rtol=0, atol=1e-13)
        assert torch.allclose(torch.tanh(want.gi[2] + r * hn), n, rtol=0, atol=1e-14)
        assert (x >= 0).all() and (x == 0).any()
    no_u = uo.forward(inp, T, 0, -1, inp.h0, with_u=False)
    assert (uo.scaled_err(no_u.q, uo.forward(inp, T, 0, -1, inp.h0).q) > 1e-3) == bool(la)


def test_gate_sum_scale_is_read_from_the_kernel_source():
    assert uo.gate_sum_scale(16, "f32") == (1.0, 1.0, 1.0) and uo.gate_sum_scale(18, "x6") == (1.0, 1.0, 1.0)
    s = uo.gate_sum_scale(17, "f32")
    assert s[0] == s[1] and abs(s[0] + 1 / np.log(2)) < 1e-7 and abs(s[2] - 2 / np.log(2)) < 1e-7
