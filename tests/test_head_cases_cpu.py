"""The head-kernel edge cases (tests/head_cases.py) on the CPU: the seed conditions every case was chosen for, the float32
yardstick of every tensor tests/test_gpu_head_edges.py compares, the weight-gradient plans the world cases reach, and the two
properties of the dtype-generic RTW oracle (float32 bits unchanged; u = -1 reads as action 0)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_cases as hc
import rtw_oracle

RTW_IDS = [hc.shape_id(*c[:3]) for c in hc.RTW_CASES]
WORLD_IDS = [hc.world_id(c) for c in hc.WORLD_CASES]
F32_WORST = {}            # head -> (share of 1e-4 max|ref|, case, tensor), printed by the last test of each head


def yardstick(head, case_id, name, f32, ref):
    """the float32 oracle against the float64 one: under a quarter of 1e-4 * max|ref| (+ the 1e-7 floor), or as F32_EXCEPTIONS says"""
    ref = np.asarray(ref, dtype=np.float64)
    err = float(np.abs(np.asarray(f32, dtype=np.float64) - ref).max())
    scale = float(np.abs(ref).max())
    share = err / (1e-4 * scale + 1e-30)
    if scale > 0 and share > F32_WORST.get(head, (0.0,))[0]:
        F32_WORST[head] = (share, case_id, name)
    print("%-6s %-28s %-34s f32 err %.3e  max|ref| %.3e  share of 1e-4 max|ref| %.4f" % (head, case_id, name, err, scale, share))
    exc = hc.F32_EXCEPTIONS.get((head, case_id, name))
    if exc is not None:
        assert err <= 1.5 * exc, (case_id, name, err, exc)
    else:
        assert err <= 0.25 * 1e-4 * scale + 1e-7, (case_id, name, err, scale)


@pytest.mark.parametrize("case", hc.RTW_CASES, ids=RTW_IDS)
def test_rtw_act_margins_and_availability(case):
    """every top-two margin >= 1e-4 in float64 at every row count and both not_self_model values: no row is ambiguous; and the
    availability edges the cases promise are present (an agent without any action picks 0, as argmax of an all -1e9 row does)"""
    N, O, A, seed = case
    for not_self in (True, False):
        for G in hc.rtw_row_counts(N):
            c, o = hc.rtw_act_oracle(N, O, A, G, seed, not_self)
            assert o.margin.min() >= hc.MARGIN, (G, not_self, o.margin.min())
            assert c.av[0, 0].sum() == 0 and (o.a.reshape(G, N, N)[0, :, 0] == 0).all()
            only0 = (c.av.sum(-1) == 1) & (c.av[..., 0] == 1)
            assert only0.any() or G * N < 2
            assert (o.a.reshape(G, N, N)[np.broadcast_to(only0[:, None, :], (G, N, N))] == 0).all()
            assert np.isnan(c.obs[:, [0, 1, 3]]).all() and np.isnan(c.avail[:, [0, 1, 3]]).all()
            assert np.isfinite(o.qr).all() and np.isfinite(o.ohat).all()


@pytest.mark.parametrize("case", hc.RTW_CASES, ids=RTW_IDS)
def test_rtw_float32_oracle_stays_under_a_quarter_of_the_bound(case):
    N, O, A, seed = case
    for not_self in (True, False):
        tag = "ns" if not_self else "self"
        for G in hc.rtw_row_counts(N):
            _, o64 = hc.rtw_act_oracle(N, O, A, G, seed, not_self)
            _, o32 = hc.rtw_act_oracle(N, O, A, G, seed, not_self, torch.float32)
            np.testing.assert_array_equal(o32.a, o64.a)
            cid = "%s_G%d_%s" % (hc.shape_id(N, O, A), G, tag)
            yardstick("rtw", cid, "act/q_r", o32.qr, o64.qr)
            yardstick("rtw", cid, "act/o_hat", o32.ohat, o64.ohat)
        for B, T in hc.rtw_given_bt(N):
            c, q64 = hc.rtw_given_oracle(N, O, A, B, T, seed, not_self)
            _, q32 = hc.rtw_given_oracle(N, O, A, B, T, seed, not_self, torch.float32)
            ept = 16 // N
            assert B >= 3 and (ept == 1 or T % ept) and (c.u == -1).any() and (c.plane[:, [0, T + 1]] == hc.POISON_U).all()
            yardstick("rtw", "%s_B%d_T%d_%s" % (hc.shape_id(N, O, A), B, T, tag), "given/q_r", q32, q64)
    if case == hc.RTW_CASES[-1]:
        print("largest float32-oracle share, RTW head: %.4f of 1e-4 max|ref| (%s %s)" % F32_WORST["rtw"])


@pytest.mark.parametrize("case", hc.WORLD_CASES, ids=WORLD_IDS)
def test_world_no_preactivation_near_the_kink(case):
    """no z or e pre-activation within 1e-5 of 0 in float64 (so no weight row is left out of a gradient comparison: the cap of
    KINK_CAP rows per case is not drawn on), and the addressing data is what the cases promise"""
    kinks = hc.world_kinks(case)
    assert sum(int(v.sum()) for v in kinks.values()) <= hc.KINK_CAP
    assert all(int(v.sum()) == 0 for v in kinks.values()), "the seed scan found a clean seed for every case"
    c = hc.world_case(case)
    assert c.R == c.B * c.T * c.N and c.ep_len[0] == c.T and len(set(c.emap.tolist())) == c.B and c.emap.max() < c.E
    assert not np.array_equal(c.emap, np.arange(c.B))
    st, seen = hc.world_storage(c, "map")
    assert np.isnan(st[:, 0]).all() and np.isnan(st[[e for e in range(c.E) if e not in c.emap]]).all()
    for b in range(c.B):
        assert np.isnan(st[c.emap[b], 1 + c.ep_len[b]:]).all() and np.isfinite(st[c.emap[b], 1:1 + c.ep_len[b]]).all()
        assert (seen[b, c.ep_len[b]:] == 0).all()


def test_world_row_counts_cross_the_loss_and_plan_seams():
    """per shape: a one-tile case, 256 and 257 loss partials; the 4096-row cases get multi-slab weight-gradient plans and the
    small ones a single slab, so marl_linear_wgrad is asked for a second plan without an extra case"""
    for shape in hc.SHAPES:
        tiles = sorted((c[3] * c[4] * c[0] + 15) // 16 for c in hc.WORLD_CASES if c[:3] == shape)
        assert tiles[0] == 1 and 256 in tiles and 257 in tiles, (shape, tiles)
    rows = {c[3] * c[4] * c[0] for c in hc.WORLD_CASES}
    assert {1, 15, 16, 17, 4096, 4097} <= rows
    assert any(c[1] % 4 for c in hc.WORLD_CASES)
    seen = set()
    for case in hc.WORLD_CASES:
        plans = hc.world_wgrad_plans(case)
        assert all(p is not None for p in plans), case
        R = case[3] * case[4] * case[0]
        if R <= 512:
            assert all(p.slabs == 1 for p in plans), (case, plans)
        if R >= 4090:
            assert all(p.slabs > 1 for p in plans), (case, plans)
        seen |= {(p.family, p.slabs > 1) for p in plans}
    assert ("generic", False) in seen and ("full", True) in seen and ("generic", True) in seen and ("thin", True) in seen


@pytest.mark.parametrize("case", hc.WORLD_CASES, ids=WORLD_IDS)
def test_world_float32_oracle_stays_under_a_quarter_of_the_bound(case):
    cid = hc.world_id(case)
    for name, a, b in zip(("r", "o_hat", "tau"), hc.world_forward_oracle(case, torch.float32), hc.world_forward_oracle(case)):
        yardstick("world", cid, name, a, b)
    for mode in hc.WORLD_MODES:
        o64, o32 = hc.world_backward_oracle(case, mode), hc.world_backward_oracle(case, mode, torch.float32)
        yardstick("world", cid, mode + "/loss", o32.loss, o64.loss)
        yardstick("world", cid, mode + "/dhs", o32.dhs, o64.dhs)
        for k in hc.WORLD_GRADS:
            yardstick("world", cid, mode + "/grad " + k, o32.grads[k], o64.grads[k])
        assert np.abs(o64.grads["world.terminate_out.weight"]).max() == 0.0
    if case in hc.WORLD_OPTIONAL_CASES:
        for tag, kw in (("no dq", dict(dq=False)), ("no den", dict(den=False))):
            o64, o32 = hc.world_backward_oracle(case, "map", **kw), hc.world_backward_oracle(case, "map", torch.float32, **kw)
            yardstick("world", cid, tag + "/dhs", o32.dhs, o64.dhs)
            for k in hc.WORLD_GRADS:
                yardstick("world", cid, tag + " grad " + k, o32.grads[k], o64.grads[k])
    if case == hc.WORLD_CASES[-1]:
        print("largest float32-oracle share, world head: %.4f of 1e-4 max|ref| (%s %s)" % F32_WORST["world"])


# ---- the dtype-generic RTW oracle
def _float32_only_act_head(p, h, o, avail, N, not_self=True):
    """act_head as it stood while the oracle was float32-only (torch.eye(N), one_hot(...).float()), kept to pin the bits"""
    G = h.shape[0] // N
    H, O, A = h.shape[1], o.shape[1], avail.shape[-1]
    hr = h.view(G, N, 1, H).expand(G, N, N, H)
    x = torch.cat([hr, torch.eye(N).view(1, 1, N, N).expand(G, N, N, N)], -1).clone()
    idx = torch.arange(N)
    if not_self:
        x[:, idx, idx] = 0.0
    t = rtw_oracle._mlp(p, "teammate_net", x)
    tm = torch.where(avail.view(G, 1, N, A).expand(G, N, N, A) == 0.0, torch.full_like(t, -1e9), t)
    a = tm.argmax(-1)
    m = F.one_hot(a, A).float()
    if not_self:
        m[:, idx, idx] = 0.0
    og = o.view(G, N, O)
    ohat = rtw_oracle._mlp(p, "world_net", torch.cat([og, m.reshape(G, N, N * A)], -1))
    qr = rtw_oracle._reflect(p, hr, og, ohat, m, N, not_self)
    return qr.reshape(G * N, A), ohat.reshape(G * N, O), a.reshape(G * N, N)


def _float32_only_given_head(p, hs, o, on, u, N, not_self=True):
    G = hs.shape[0] // N
    H, O, A = hs.shape[1], o.shape[1], p["w_k.weight"].shape[1]
    hr = hs.view(G, 1, N, H).expand(G, N, N, H)
    m = F.one_hot(u.view(G, 1, N).expand(G, N, N).clamp(min=0).long(), A).float()
    if not_self:
        idx = torch.arange(N)
        m[:, idx, idx] = 0.0
    return rtw_oracle._reflect(p, hr, o.view(G, N, O), on.view(G, N, O), m, N, not_self).reshape(G * N, A)


@pytest.mark.parametrize("not_self", [True, False])
def test_rtw_oracle_float32_bits_unchanged(golden_dir, not_self):
    """the MMM2 fixture's act inputs (tests/test_rtw_cpu.py::test_oracle_matches_reference_mmm2_seeded) and a given-mode batch:
    the dtype-generic oracle in float32 gives the bits of the float32-only statements; params_t still defaults to float32"""
    fx = np.load(os.path.join(golden_dir, "rtw_MMM2.npz"))
    N, O, A = 10, 176, 18
    sd = {k[3:]: fx[k] for k in fx.files if k.startswith("sd/")}
    p = rtw_oracle.params_t(sd)
    assert all(v.dtype == torch.float32 for v in p.values())
    G = fx["act/obs"].shape[0]
    h = torch.tensor(fx["act/h"]).reshape(G * N, 64)
    o, av = torch.tensor(fx["act/obs"]).reshape(G * N, O), torch.tensor(fx["act/avail"])
    with torch.no_grad():
        new, old = rtw_oracle.act_head(p, h, o, av, N, not_self), _float32_only_act_head(p, h, o, av, N, not_self)
        for a, b in zip(new[:3], old):
            assert a.dtype == b.dtype and torch.equal(a, b)
        c = hc.make_rtw_given(N, O, A, 3, 2, 5)
        args = (torch.tensor(c.hs).reshape(-1, 64), torch.tensor(c.obs[:, :2]).reshape(-1, O), torch.tensor(c.obs[:, 1:]).reshape(-1, O),
                torch.tensor(c.u).reshape(-1), N, not_self)
        a, b = rtw_oracle.given_head(p, *args), _float32_only_given_head(p, *args)
        assert a.dtype == torch.float32 and torch.equal(a, b)
        # and float64 in, float64 out
        p64 = rtw_oracle.params_t(sd, torch.float64)
        assert all(x.dtype == torch.float64 for x in rtw_oracle.act_head(p64, h.double(), o.double(), av.double(), N, not_self)[:2])


@pytest.mark.parametrize("not_self", [True, False])
def test_rtw_given_head_reads_padded_actions_as_zero(not_self):
    N, O, A, seed = hc.RTW_CASES[4]
    B, T = hc.rtw_given_bt(N)[0]
    c = hc.make_rtw_given(N, O, A, B, T, seed)
    assert (c.u == -1).sum() > 1
    p = rtw_oracle.params_t(hc.rtw_params(N, O, A, seed), torch.float64)
    args = [torch.tensor(x, dtype=torch.float64).reshape(-1, x.shape[-1]) for x in (c.hs, c.obs[:, :T], c.obs[:, 1:])]
    u = torch.tensor(c.u).reshape(-1)
    with torch.no_grad():
        assert torch.equal(rtw_oracle.given_head(p, *args, u, N, not_self), rtw_oracle.given_head(p, *args, u.clamp(min=0), N, not_self))
