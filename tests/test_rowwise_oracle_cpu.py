"""tests/rowwise_oracle.py against torch in float64 (autograd, torch.optim, plain indexing), and every condition the GPU cases of
tests/test_gpu_rowwise.py rely on, checked where no GPU is needed: the ties tie, the all-unavailable rows exist, the gradient norms
sit on the intended side of the clip threshold, the derived bounds stay under the ceilings the older kernel tests hold."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rowwise_oracle as ro

t64 = lambda x, grad=False: torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=grad)


# ------------------------------------------------------------------------------------------ gather and select rules
@pytest.mark.parametrize("T,N,A", ro.REPLAY_SHAPES)
def test_replay_sample_is_plain_indexing(T, N, A):
    ring, idx = ro.replay_case(T, N, A)
    s = ro.replay_sample(ring, idx)
    for b, e in enumerate(idx):
        assert s.o_map[b] == e and s.length[b] == ring.length[e] and s.won[b] == ring.won[e]
        assert (s.u[b] == ring.u[e]).all() and (s.u_act[b] == np.where(ring.u[e] < 0, 0, ring.u[e])).all()
        assert (s.r[b] == ring.r[e]).all() and (s.term[b] == ring.term[e]).all() and (s.padded[b] == ring.padded[e]).all()
        for t in range(T):
            assert (s.avail_next[b, t] == ring.avail[e, t + 1]).all()
            assert (s.avail_cur[b, t] == (ring.avail[e, t] if t < ring.length[e] else 0)).all()
    # what the GPU cases rely on
    assert len(set(idx.tolist())) < len(idx) and 0 in idx and ro.REPLAY_RING - 1 in idx and list(idx) != sorted(idx)
    assert ro.REPLAY_RING > len(idx)
    L = ring.length[idx]
    assert L.min() == 1 and L.max() == T and (T < 3 or ((L > 1) & (L < T)).any())
    for e in range(ro.REPLAY_RING):
        assert (ring.u[e, ring.length[e]:] == -1).all() and (ring.u[e, :ring.length[e]] >= 0).all()
    assert (ring.avail > 0).all()          # a zeroed entry of avail_cur is never a copied one: an off-by-one end shows
    for a in range(ro.REPLAY_RING):        # no two episodes and no two slots hold the same availability
        for b in range(a + 1, ro.REPLAY_RING):
            assert not np.array_equal(ring.avail[a], ring.avail[b]) and not np.array_equal(ring.r[a], ring.r[b])
    assert all(not np.array_equal(ring.avail[:, t], ring.avail[:, t + 1]) for t in range(T))


def test_replay_chunking_arithmetic():
    """the sizes the cases are named for: 1024 floats per chunk of avail"""
    sizes = [T * N * A for T, N, A in ro.REPLAY_SHAPES]
    assert sizes == [1, 105, 1024, 1025, 6720, 600]
    assert -(-6720 // 1024) == 7 and 60 * 8 > 256 and 300 > 256


@pytest.mark.parametrize("rows,A", [(1, 1), (257, 11), (65, 32), (4096, 33)])
def test_select_rules_are_plain_indexing(rows, A):
    c = ro.select_case(rows, A)
    masked = torch.where(t64(c.avail) == 0, torch.tensor(ro.MASK_VAL, dtype=torch.float64), t64(c.q_sel))
    mx, arg = ro.q_masked_max(c.q_sel, c.avail, ro.MASK_VAL)
    for r in range(min(rows, 300)):
        row = masked[r].tolist()
        assert mx[r] == max(row) and arg[r] == row.index(max(row))
    assert (mx == masked.max(dim=1)[0].numpy()).all()
    val, arg2 = ro.q_double_select(c.q_sel, c.q_val, c.avail, ro.MASK_VAL)
    assert (arg2 == arg).all()
    mv = np.where(c.avail == 0, ro.MASK_VAL, c.q_val.astype(np.float64))
    assert (val == mv[np.arange(rows), arg]).all()
    g = ro.q_gather(c.q_sel, c.idx, c.avail, ro.MASK_VAL)
    g0 = ro.q_gather(c.q_sel, c.idx)
    for r in range(min(rows, 300)):
        a = c.idx[r]
        assert g0[r] == (0.0 if a < 0 else c.q_sel[r, a])
        assert g[r] == (0.0 if a < 0 else (ro.MASK_VAL if c.avail[r, a] == 0 else c.q_sel[r, a]))
    mx0, arg0 = ro.q_masked_max(c.q_sel, None, ro.MASK_VAL)
    assert (mx0 == c.q_sel.max(axis=1)).all() and (arg0 == torch.tensor(c.q_sel).argmax(dim=1).numpy()).all() or A == 1
    # the edges the GPU cases rely on
    r = np.arange(rows)
    if rows >= 5 and A >= 3:
        t0, t1, t2 = r % 5 == 0, r % 5 == 1, r % 5 == 2
        assert (masked.numpy()[t0, 0] == masked.numpy()[t0, A - 1]).all() and (arg[t0] == 0).all()
        assert (mx[t0] == 7.5).all() and (mx[t1] == 8.25).all() and (arg[t1] == A - 2).all()
        assert (c.avail[t2] == 0).all() and (mx[t2] == ro.MASK_VAL).all() and (arg[t2] == 0).all() and (val[t2] == ro.MASK_VAL).all()
        assert (c.idx < 0).any() and ((c.idx >= 0) & (c.avail[r, np.maximum(c.idx, 0)] == 0)).any()
    assert float(np.float32(ro.MASK_VAL)) == ro.MASK_VAL


def test_scatter_sum_bcast_add_rules():
    g = np.random.default_rng(3)
    rows, A, N = 40, 6, 5
    i1, i2 = g.integers(-1, A, rows), g.integers(-1, A, rows)
    i2[:10] = i1[:10]
    g1, g2 = g.standard_normal(rows // N), g.standard_normal(rows // N)
    dq = ro.q_scatter(i1, g1, i2, g2, rows, A, gdiv=N)
    want = np.zeros((rows, A))
    for r in range(rows):
        if i1[r] >= 0:
            want[r, i1[r]] += g1[r // N]
        if i2[r] >= 0:
            want[r, i2[r]] += g2[r // N]
    assert (dq == want).all() and (i1[:10] >= 0).any()
    one = ro.q_scatter(i1, g.standard_normal(rows), None, None, rows, A)
    assert ((one != 0).sum(axis=1) <= 1).all()
    x = g.standard_normal((7, N, 3))
    s, mag = ro.agent_sum(x)
    assert np.allclose(s, t64(x).sum(1).numpy(), rtol=1e-15) and (mag >= np.abs(s)).all()
    b = ro.agent_bcast(s, N, base=x)
    assert (b == s[:, None, :] + x).all() and (ro.agent_bcast(s, N)[:, 3] == s).all()
    assert (ro.vec_add(x, 2 * x) == x + 2 * x).all()


def test_double_select_lds_arithmetic():
    """what motivates the row-per-thread form of marl_q_double_select: four waves x three operands x 64 rows x A floats"""
    lds = lambda A, operands: 4 * operands * ((64 * A + 3) & ~3) * 4
    assert lds(21, 3) == 64512 <= 65536 < lds(22, 3) == 67584
    assert all(lds(A, 3) > 65536 for A in range(22, 33))
    assert lds(32, 2) == 65536 < lds(33, 2)            # marl_q_masked_max: 32 actions request exactly 64 KiB, 33 fall back
    assert 2048 * 4 * 64 == 524288 and 1024 * 256 == 262144 and 8192 * 256 // 64 * 2 == 65536 and 4096 * 256 == 1048576


# ------------------------------------------------------------------------------------------ QMIX mixing against autograd
def _torch_qmix(c, bias_form):
    N, E = c.N, c.E
    hy, q, b2, w22, b22 = t64(c.hy, True), t64(c.q, True), t64(c.b2, True), t64(c.w22), t64(c.b22)
    w1 = hy[:, :N * E].abs().view(-1, N, E)
    hid = F.elu(torch.bmm(q.view(-1, 1, N), w1).squeeze(1) + hy[:, N * E:N * E + E])
    bias = b2 if bias_form == "b2" else F.relu(hy[:, N * E + 2 * E:]) @ w22 + b22
    qt = (hid * hy[:, N * E + E:N * E + 2 * E].abs()).sum(1) + bias
    (qt * t64(c.dq_tot)).sum().backward()
    return qt.detach().numpy(), hy.grad.numpy(), q.grad.numpy(), (b2.grad.numpy() if bias_form == "b2" else None)


@pytest.mark.parametrize("N,E", [(1, 16), (5, 32), (10, 32), (16, 64)])
@pytest.mark.parametrize("bias_form", ["b2", "w22"])
def test_qmix_mixing_matches_autograd(N, E, bias_form):
    c = ro.qmix_case(131, N, E, seed=N)
    qt, dhy, dq, db2 = _torch_qmix(c, bias_form)
    kw = dict(b2=c.b2) if bias_form == "b2" else dict(w22=c.w22, b22=c.b22)
    f = ro.qmix_mix(c.hy, c.q, N, E, **kw)
    np.testing.assert_allclose(f.q_tot, qt, rtol=1e-12, atol=1e-13)
    assert (f.mag >= np.abs(f.q_tot) * (1 - 1e-12)).all()
    g = ro.qmix_mix_grad(c.hy, c.q, c.dq_tot, N, E, w22=None if bias_form == "b2" else c.w22)
    np.testing.assert_allclose(g.d_w1.reshape(c.R, -1), dhy[:, :N * E], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(g.d_b1, dhy[:, N * E:N * E + E], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(g.d_w2, dhy[:, N * E + E:N * E + 2 * E], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(g.dq, dq, rtol=1e-12, atol=1e-14)
    if bias_form == "b2":
        assert (g.db2 == db2).all() and g.d_hb is None and (dhy[:, N * E + 2 * E:] == 0).all()
    else:
        np.testing.assert_allclose(g.d_hb, dhy[:, N * E + 2 * E:], rtol=1e-12, atol=0)
    for got, mag in ((g.d_w1, g.mag_w1), (g.d_b1, g.mag_b1), (g.d_w2, g.mag_w2), (g.dq, g.mag_q)):
        assert (mag >= np.abs(got) * (1 - 1e-12)).all()
    # planted zeros: the gradient there is exactly 0 (torch's abs and relu)
    w1z, w2z, hbz = c.hy[:, :N * E] == 0, c.hy[:, N * E + E:N * E + 2 * E] == 0, c.hy[:, N * E + 2 * E:] == 0
    assert w1z.any() and w2z.any() and hbz.any()
    assert (g.d_w1.reshape(c.R, -1)[w1z] == 0).all() and (dhy[:, :N * E][w1z] == 0).all()
    assert (g.d_w2[w2z] == 0).all() and (dhy[:, N * E + E:N * E + 2 * E][w2z] == 0).all()
    if g.d_hb is not None:
        assert (g.d_hb[hbz] == 0).all()
    # large negative and near-zero pre-activations exist
    assert (f.pre < -20).any() and (np.abs(f.pre) < 1e-6).any() and (f.pre > 0.5).any()


@pytest.mark.parametrize("N,E", [(1, 16), (5, 32), (10, 32), (16, 64)])
def test_qmix_bounds_stay_under_the_ceiling(N, E):
    """the ceiling of the mixing kernels: 1e-4 of the tensor's scale max|ref| (tests/parity.py's reading of a tolerance)"""
    c = ro.qmix_case(131, N, E, seed=N)
    f = ro.qmix_mix(c.hy, c.q, N, E, w22=c.w22, b22=c.b22)
    g = ro.qmix_mix_grad(c.hy, c.q, c.dq_tot, N, E, w22=c.w22)
    ceil = lambda ref: 1e-4 * np.abs(ref).max()
    assert (ro.k_qmix_fwd(N, E) * ro.U * f.mag <= ceil(f.q_tot)).all()
    assert (ro.k_qmix_dw1(N) * ro.U * g.mag_w1 <= ceil(g.d_w1)).all()
    assert (ro.k_qmix_dpre(N) * ro.U * g.mag_b1 <= ceil(g.d_b1)).all()
    assert (ro.k_qmix_dw2(N) * ro.U * g.mag_w2 <= ceil(g.d_w2)).all()
    assert (ro.k_qmix_dq(N, E) * ro.U * g.mag_q <= ceil(g.dq)).all()


# ------------------------------------------------------------------------------------------ losses against autograd
@pytest.mark.parametrize("kind", ro.LOSS_KINDS)
def test_losses_match_autograd(kind):
    c = ro.loss_case(257, kind)
    mask = 1 - t64(c.padded)
    q_tot = t64(c.q_tot, True)
    td = mask * (t64(c.r) + ro.GAMMA * t64(c.q_tgt) * (1 - t64(c.term)) - q_tot)
    (td ** 2).sum().backward()
    o = ro.td_loss(c.q_tot, c.q_tgt, c.r, c.term, c.padded, ro.GAMMA)
    np.testing.assert_allclose(o.dq_tot, q_tot.grad.numpy(), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(o.out2, [float((td ** 2).sum().detach()), float(mask.sum())], rtol=1e-13)
    assert o.mag_num >= o.out2[0] and (o.mag_dq >= np.abs(o.dq_tot)).all()

    jq, v, so, sn = t64(c.jq, True), t64(c.v, True), t64(c.qs_opt, True), t64(c.qs_nopt, True)
    y = t64(c.r) + ro.GAMMA * t64(c.jq_tgt) * (1 - t64(c.term))
    l_td = (((jq - y) * mask) ** 2).sum()
    l_opt = (((so - t64(c.jq_hat) + v) * mask) ** 2).sum()
    l_nopt = (((sn - jq.detach() + v).clamp(max=0) * mask) ** 2).sum()
    (l_td + ro.LAM_OPT * l_opt + ro.LAM_NOPT * l_nopt).backward()
    assert ro.LAM_OPT != ro.LAM_NOPT and 1.0 not in (ro.LAM_OPT, ro.LAM_NOPT)
    o = ro.qtran_loss(c.jq, c.jq_tgt, c.v, c.jq_hat, c.qs_opt, c.qs_nopt, c.r, c.term, c.padded, ro.GAMMA, ro.LAM_OPT, ro.LAM_NOPT)
    for got, ref in ((o.d_jq, jq), (o.d_v, v), (o.d_qs_opt, so), (o.d_qs_nopt, sn)):
        np.testing.assert_allclose(got, ref.grad.numpy(), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(o.out4, [float(l_td.detach()), float(l_opt.detach()), float(l_nopt.detach()), float(mask.sum())], rtol=1e-13)
    # swapped lambdas are another function
    sw = ro.qtran_loss(c.jq, c.jq_tgt, c.v, c.jq_hat, c.qs_opt, c.qs_nopt, c.r, c.term, c.padded, ro.GAMMA, ro.LAM_NOPT, ro.LAM_OPT)
    if kind != "all_padded":
        assert np.abs(sw.d_qs_opt - o.d_qs_opt).max() > 0.1 and np.abs(sw.d_v - o.d_v).max() > 0.1
        assert (o.nraw == 0).any() and (o.nraw > 0).any() and (o.nraw < 0).any()
        assert (o.d_qs_nopt[o.nraw >= 0] == 0).all() and (o.d_qs_nopt[(o.nraw < 0) & (c.padded == 0)] != 0).all()
    else:
        assert (o.out4 == 0).all() and all((x == 0).all() for x in (o.d_jq, o.d_v, o.d_qs_opt, o.d_qs_nopt))
    if kind == "all_terminated":
        assert (c.term == 1).all()
    if kind == "none_padded":
        assert o.out4[3] == c.R
    # fp32 evaluation of the exactly-zero rows is exactly zero as well
    z = np.arange(c.R) % 3 == 0
    assert ((c.qs_nopt[z] - c.jq[z]) + c.v[z] == 0).all()
    # ceilings of the older test (test_losses_and_optimizer): 1e-5 of scale
    assert ro.K_TD * ro.U <= 1e-5 and ro.K_QTRAN_G * ro.U <= 1e-5 and ro.K_TD_NUM * ro.U <= 1e-5 and ro.K_QTRAN_NUM * ro.U <= 1e-5


# ------------------------------------------------------------------------------------------ optimizer against torch.optim
@pytest.mark.parametrize("kind", ["RMS", "Adam"])
@pytest.mark.parametrize("den", [None, 37.0])
def test_optimizer_matches_torch_over_three_steps(kind, den):
    g = np.random.default_rng(11)
    n = 1001
    p = g.standard_normal(n)
    pt = torch.nn.Parameter(t64(p))
    opt = (torch.optim.RMSprop([pt], lr=ro.LR, alpha=ro.ALPHA, eps=ro.EPS) if kind == "RMS"
           else torch.optim.Adam([pt], lr=ro.LR, betas=(ro.BETA1, ro.BETA2), eps=ro.EPS))
    s1, s2 = np.zeros(n), np.zeros(n)
    coefs = []
    for step, size in ((1, 50.0), (2, 0.05), (3, 3.0)):
        graw = g.standard_normal(n) * size * (den or 1.0)
        pt.grad = t64(graw / (den or 1.0))
        torch.nn.utils.clip_grad_norm_([pt], ro.CLIP)
        opt.step()
        if kind == "RMS":
            o = ro.rmsprop_step(p, graw, s1, ro.LR, ro.ALPHA, ro.EPS, ro.CLIP, den)
            p, s1 = o.p, o.sq
            np.testing.assert_allclose(s1, opt.state[pt]["square_avg"].numpy(), rtol=1e-12, atol=0)
        else:
            o = ro.adam_step(p, graw, s1, s2, ro.LR, ro.BETA1, ro.BETA2, ro.EPS, 1 - ro.BETA1 ** step,
                             np.sqrt(1 - ro.BETA2 ** step), ro.CLIP, den)
            p, s1, s2 = o.p, o.m, o.v
            np.testing.assert_allclose(s1, opt.state[pt]["exp_avg"].numpy(), rtol=1e-12, atol=1e-18)
            np.testing.assert_allclose(s2, opt.state[pt]["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(p, pt.detach().numpy(), rtol=1e-12, atol=1e-14)
        coefs.append(o.coef)
    assert coefs[0] < 1 and coefs[1] > 1 and coefs[2] < 1          # the clip is active in some steps and inactive in others


@pytest.mark.parametrize("den", [None, 37.0, 9000.0])
@pytest.mark.parametrize("n", [1, 257, 262145])
def test_clip_regimes_sit_where_intended(n, den):
    """the GPU cases just under the threshold really have an fp64 coefficient >= 1, their twins < 1, both within 1e-3"""
    want = {"under": (9.9, 10.1), "over": (0.199, 0.201), "just_under": (1.0, 1.001), "just_over": (0.999, 1.0)}
    for regime, (lo, hi) in want.items():
        c = ro.optim_case(n, regime, den)
        _, coef = ro.grad_scale(ro.sumsq(c.g), den, ro.CLIP)
        assert lo <= coef <= hi and (coef >= 1) == (regime in ("under", "just_under")), (regime, coef)
        assert abs(coef - 1) > 2 * ro.K_SCALE * ro.U or regime in ("under", "over")     # not within the kernel's own error of 1
        if n > 7:
            z = np.arange(n) % 7 == 0
            assert (c.g[z] == 0).all() and (c.sq[z] == 0).all() and (c.m[z] == 0).all() and (c.v[z] == 0).all()
            assert (c.sq[~z] > 0).all() and (c.v[~z] > 0).all() and (c.m[~z] != 0).any()
            o = ro.rmsprop_step(c.p, c.g, c.sq, ro.LR, ro.ALPHA, ro.EPS, ro.CLIP, den)
            assert (o.dp[z] == 0).all() and (o.sq[z] == 0).all()
            # without the clamp the step is another one by far more than the bound
            if regime == "just_under":
                sc, _ = ro.grad_scale(ro.sumsq(c.g), den, ro.CLIP)
                gi = c.g.astype(np.float64) * sc * coef
                s = ro.ALPHA * c.sq + (1 - ro.ALPHA) * gi * gi
                dp = ro.LR * gi / (np.sqrt(s) + ro.EPS)
                assert (np.abs(dp - o.dp) > ro.K_RMS_DP * ro.U * o.mag_dp + ro.U * np.abs(o.p)).any()


def test_optimizer_bounds_stay_under_the_ceiling():
    """the older test (test_losses_and_optimizer) holds 2e-6 + 1e-5 |ref|"""
    for regime in ro.OPT_REGIMES:
        c = ro.optim_case(65537, regime, 37.0)
        o = ro.rmsprop_step(c.p, c.g, c.sq, ro.LR, ro.ALPHA, ro.EPS, ro.CLIP, c.den)
        assert (ro.U * np.abs(o.p) + ro.K_RMS_DP * ro.U * o.mag_dp <= 2e-6 + 1e-5 * np.abs(o.p)).all()
        for step in (1, 1000):
            bc1, bc2s = ro.bias_corrections(step)
            a = ro.adam_step(c.p, c.g, c.m, c.v, ro.LR, ro.BETA1, ro.BETA2, ro.EPS, bc1, bc2s, ro.CLIP, c.den)
            assert (ro.U * np.abs(a.p) + ro.K_ADAM_DP * ro.U * a.mag_dp <= 2e-6 + 1e-5 * np.abs(a.p)).all()
            assert (a.mag_dp >= np.abs(a.dp) * (1 - 1e-12)).all() and (a.mag_m >= np.abs(a.m) * (1 - 1e-12)).all()
    assert max(ro.K_SQ, ro.K_ADAM_V, ro.K_ADAM_M, ro.K_SUMSQ) * ro.U <= 1e-5
    assert 1 - ro.ALPHA == float(np.float32(1) - np.float32(ro.ALPHA))      # the kernel's 1.f - alpha is exact (Sterbenz)
    assert 1 - ro.BETA1 == float(np.float32(1) - np.float32(ro.BETA1)) and 1 - ro.BETA2 == float(np.float32(1) - np.float32(ro.BETA2))


def test_sumsq_is_the_float64_sum():
    g = np.random.default_rng(5).standard_normal(70001).astype(np.float32)
    assert ro.sumsq(g) == pytest.approx(float((t64(g) ** 2).sum()), rel=1e-13)
