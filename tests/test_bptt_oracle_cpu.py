"""tests/bptt_oracle.py itself, without a GPU: the float64 unroll against oracle/nets.agent_unroll and its autograd, the dxp / dh0
path against central differences, the share of dxp the kink mask removes in every kernel case, the launch-plan mirror against the
table the cases were picked from, and the probe rows."""
import numpy as np
import pytest
import torch

import bptt_oracle as bo
from oracle import nets

TINY = [bo._c("2s3z", 2, 3, (0, 1), (1, 1)), bo._c("matrix", 2, 3, (0, 1), (1, 1)),
        bo._c("2s3z", 3, 2, None, (1, 1), la=0, rn=1), bo._c("MMM2", 2, 3, (0, 2), (1, 2), la=1, rn=0)]


def _nets_unroll(k):
    a = k.args
    p = {n: torch.tensor(v, dtype=torch.float64, requires_grad=True) for n, v in k.p.items()}
    h0 = torch.tensor(k.h0, dtype=torch.float64)
    q, hs, hl = nets.agent_unroll(p, torch.tensor(k.obs, dtype=torch.float64), bo.onehot(k.ufed, a.n_actions, torch.float64), h0,
                                  a.last_action, a.reuse_network)
    return p, q, hs, hl


@pytest.mark.parametrize("c", TINY, ids=bo.case_id)
@pytest.mark.parametrize("form", bo.FORMS)
def test_unroll_and_parameter_gradients_equal_nets_agent_unroll(c, form):
    k = bo.make_case(c)
    u = bo.unroll(k)
    p, q, hs, hl = _nets_unroll(k)
    for got, want in ((u.q, q), (u.hs, hs), (u.h_last, hl)):
        assert got.dtype == torch.float64 and float((got - want).detach().abs().max()) <= 1e-12
    d = bo.make_dq(c, form)
    got = bo.backward(u, d.full, d.dhs)
    loss = (q * d.full.double()).sum()
    if d.dhs is not None:
        loss = loss + (hs * d.dhs.double()).sum()
    loss.backward()
    for n in bo.PARAMS:
        assert got[n].dtype == torch.float64
        assert float((got[n] - p[n].grad).abs().max()) <= 1e-12 * max(1.0, float(p[n].grad.abs().max())), n
    # a second backward on the same unroll starts from zero
    again = bo.backward(u, d.full, d.dhs)
    for n in got:
        assert torch.equal(again[n], got[n]), n


def test_sparse_forms_stand_for_their_dense_tensor():
    c = TINY[0]
    d = bo.make_dq(c, "s1")
    b, t, n = 1, 2, 3
    assert d.full[b, t, n, d.idx[b, t, n]] == d.val[b, t, n] and int((d.full[b, t, n] != 0).sum()) == 1
    d = bo.make_dq(c, "s2h")
    assert d.gdiv == c.N and d.val.shape == (c.B, c.T)
    assert torch.equal(d.idx[0, 0], d.idx2[0, 0]) and torch.equal(d.full[0, 0].sum(-1), (d.val[0, 0] + d.val2[0, 0]).expand(c.N))
    want = torch.zeros(c.A)
    want[d.idx[b, t, n]] += d.val[b, t]
    want[d.idx2[b, t, n]] += d.val2[b, t]
    assert torch.equal(d.full[b, t, n], want)


@pytest.mark.parametrize("c", TINY[:2], ids=bo.case_id)
def test_dxp_and_dh0_against_central_differences(c):
    k = bo.make_case(c)
    d = bo.make_dq(c, "s2h")

    def loss(pre_delta=None, h0_delta=None):
        kk = k
        if h0_delta is not None:
            kk = bo.types.SimpleNamespace(**vars(k))
            kk.h0 = k.h0.astype(np.float64) + h0_delta
        u = bo.unroll(kk, pre_delta=pre_delta)
        return float(((u.q * d.full.double()).sum() + (u.hs * d.dhs.double()).sum()).detach())

    u = bo.unroll(k)
    g = bo.backward(u, d.full, d.dhs)
    pre = bo.pre_of(u)
    eps = 1e-4
    R = c.R
    # h0: the largest entry and a few fixed ones
    picks = [divmod(int(g["dh0"].abs().argmax()), bo.H), (0, 0), (R - 1, 63), (R // 2, 17)]
    for r, j in picks:
        dl = np.zeros((R, bo.H))
        dl[r, j] = eps
        fd = (loss(h0_delta=dl) - loss(h0_delta=-dl)) / (2 * eps)
        an = float(g["dh0"][r, j])
        assert abs(fd - an) <= 1e-6 * abs(an), ("dh0", r, j, fd, an)
    # pre-activations: per step the largest gated-on entry; one gated-off entry (exactly zero either way)
    dxp = g["dxp"]                                                # (B,T,N,H); row r = b N + n
    for t in range(c.T):
        flat = dxp[:, t].reshape(R, bo.H)
        r, j = divmod(int(flat.abs().argmax()), bo.H)
        dl = torch.zeros(c.T, R, bo.H, dtype=torch.float64)
        dl[t, r, j] = eps
        fd = (loss(pre_delta=dl) - loss(pre_delta=-dl)) / (2 * eps)
        an = float(flat[r, j])
        assert float(pre[:, t].reshape(R, bo.H)[r, j]) > 100 * eps      # gated on, away from the kink
        assert an != 0 and abs(fd - an) <= 1e-6 * abs(an), ("dxp", t, r, j, fd, an)
    off = (pre < -0.1).nonzero()[0]
    b, t, n, j = (int(x) for x in off)
    dl = torch.zeros(c.T, R, bo.H, dtype=torch.float64)
    dl[t, b * c.N + n, j] = eps
    assert float(dxp[b, t, n, j]) == 0.0 and loss(pre_delta=dl) == loss(pre_delta=-dl)


@pytest.mark.parametrize("c", bo.CASES, ids=bo.case_id)
def test_kink_mask_removes_at_most_1e_4_of_dxp(c):
    """a condition on the seeded cases (a case that exceeds it gets another seed), not a measurement of the kernels"""
    with torch.no_grad():
        k = bo.make_case(c)
        a = k.args
        p = {n: torch.tensor(v, dtype=torch.float64) for n, v in k.p.items()}
        obs, oh = torch.tensor(k.obs, dtype=torch.float64), bo.onehot(k.ufed, a.n_actions, torch.float64)
        pre = torch.stack([nets.lin(p, "fc1", nets.build_inputs(obs[:, t], oh[:, t], c.N, a.last_action, a.reuse_network))
                           for t in range(c.T)])
    share = float(bo.kink_mask(pre).double().mean())
    print("%s: kink share %.2e" % (bo.case_id(c), share))
    assert share <= 1e-4


# tiles -> (n2, n1) of the split kernel; the 4096-env headline (1280 tiles) runs the mixed plan
X6_TABLE = {1: (0, 1), 256: (0, 256), 257: (129, 0), 512: (256, 0), 513: (256, 1), 514: (256, 2), 768: (256, 256), 769: (385, 0),
            1024: (512, 0), 1025: (512, 1), 1280: (512, 256), 1281: (641, 0), 1282: (641, 0)}
# (rows, A) -> (RT, workgroups) of the fp32 kernels
F32_TABLE = {(4090, 11): (1, 256), (4110, 11): (2, 129), (8205, 11): (3, 171), (8315, 11): (3, 174), (12285, 11): (3, 256),
             (12300, 11): (4, 193), (16385, 11): (5, 205), (16500, 11): (5, 207), (20500, 11): (6, 214), (40000, 11): (6, 417),
             (8210, 18): (3, 172), (8320, 18): (3, 174), (20500, 18): (4, 321)}


def test_plan_mirror_reproduces_the_table():
    for tiles, want in X6_TABLE.items():
        assert bo.bx6_plan(tiles * 16) == want and bo.bx6_plan(tiles * 16 - 15) == want, tiles
    for (R, A), want in F32_TABLE.items():
        assert bo.f32_plan(R, A) == want, (R, A)
    for c in bo.CASES:
        assert bo.f32_plan(c.R, c.A) == c.f32, bo.case_id(c)
        if c.x6 is not None:
            assert bo.bx6_plan(c.R) == c.x6 and c.T >= 3, bo.case_id(c)
        else:
            assert c.T < 3
    # the branches the cases are there for
    by = {(c.shape, c.R, c.T): c for c in bo.CASES if c.la and c.rn}
    assert by[("2s3z", 4110, 3)].x6[0] * 2 == bo.tiles_of(4110) + 1                  # no second tile in the last workgroup
    assert by[("2s3z", 16385, 3)].R - 32 * 512 == 1                                  # the second launch holds one row
    assert by[("2s3z", 12300, 3)].R - 192 * 64 == 12                                 # the last RT-4 workgroup: one 12-row tile
    assert {c.f32[0] for c in bo.CASES} == {1, 2, 3, 4, 5, 6}


@pytest.mark.parametrize("c", bo.CASES, ids=bo.case_id)
def test_probe_rows_lie_inside_the_batch_and_on_every_seam(c):
    s = bo.seams(c.R, c.A)
    rows = bo.probe_rows(c.R, s)
    assert all(0 <= r < c.R for r in rows) and rows == sorted(set(rows))
    assert {0, c.R - 1, 15, 16} <= set(rows)
    rt, nwg = c.f32
    want = {rt * 16, (nwg - 1) * rt * 16}
    n2, n1 = bo.bx6_plan(c.R)
    want |= {32 if n2 else 16, 32 * n2 + 16 * (n1 - 1) if n1 else 32 * (n2 - 1)}
    if n2 and n1:
        want.add(32 * n2)
    for w in want:
        assert w - 1 in rows and w in rows, (w, rows)
    d = bo.make_dq(c, "probe")
    val = d.val.permute(0, 2, 1).reshape(c.R, c.T)                # row = b N + n
    hit = (val != 0).all(1)
    assert hit.nonzero().flatten().tolist() == rows and bool((val[~hit] == 0).all())
    assert len(rows) <= 20
