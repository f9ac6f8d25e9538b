"""LICA's kernels on the MI355X: the mixing-critic row kernels of csrc/lica.hip against tests/lica_oracle.rows (float64, the analytic
contract, itself held to autograd by tests/test_lica_oracle_cpu.py) and marl_policy_probs_bwd of csrc/policy.hip against float64
autograd through the pi definition.

Bound: tests/parity.close at 1e-4 * max|ref| on every tensor (the sequential float32 twin stays under a quarter of it on every case
here - tests/test_lica_oracle_cpu.py - so there is no exception), plus the exact checks the header states."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import lica_oracle as lo
import parity

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENT = 7.0
SEED = 11


def dev(x, dt=None):
    return torch.tensor(np.ascontiguousarray(x), device=DEV, dtype=dt)


def _sent(*shape):
    return torch.full(shape, SENT, device=DEV)


def _inputs(c, N, A, inp):
    """(x, u, oracle keywords) of an input kind: the pi-like dense x, an exact one-hot as dense x, or the taken actions"""
    if inp == "x":
        return dev(c["x"]), None, dict(x=c["x"])
    if inp == "onehot":
        return dev(lo.onehot_rows(c["u"], N, A, np.float32)), None, dict(u=c["u"])
    return None, dev(c["u"]).reshape(-1), dict(u=c["u"])


def run_mix(c, N, A, E, inp, pad=0):
    """mix_fwd, then mix_bwd with both outputs; hy and dhy live in buffers ``pad`` floats wider than needed, sentinel in the gap"""
    from marl_amd import ops
    R, K = len(c["hy"]), N * A
    W = K * E + 2 * E + 1
    hyb, dhyb = _sent(R, W + pad), _sent(R, W - 1 + pad)
    hyb[:, :W] = dev(c["hy"])
    hy, dhy = hyb[:, :W], dhyb[:, :W - 1]
    x, u, _ = _inputs(c, N, A, inp)
    q, dx = _sent(R), _sent(R, K)
    ops.lica_mix_fwd(hy, x, u, q, R, N, A, E)
    ops.lica_mix_bwd(hy, x, u, dev(c["dq"]), dhy, dx, R, N, A, E)
    return dict(q=q, dhy=dhy, dx=dx, hy_buf=hyb, dhy_buf=dhyb)


def check_mix(case, c, N, A, E, inp, pad=0):
    R, K = len(c["hy"]), N * A
    KE = K * E
    _, _, kw = _inputs(c, N, A, inp)
    ref = lo.rows(c["hy"], N, A, E, dq=c["dq"], **kw)
    got = run_mix(c, N, A, E, inp, pad)
    for k in ("q", "dhy", "dx"):
        parity.close(case, k, got[k].cpu().numpy(), ref[k])
    if pad:
        assert bool((got["hy_buf"][:, KE + 2 * E + 1:] == SENT).all()) and bool((got["dhy_buf"][:, KE + 2 * E:] == SENT).all())
    dhy = got["dhy"].cpu().numpy()
    if inp != "x":                                   # exact: dpre in the blocks of the taken actions, zeros in the others
        dW = dhy[:, :KE].reshape(R, N, A, E)
        db1 = dhy[:, KE:KE + E]
        taken = lo.onehot_rows(c["u"], N, A).reshape(R, N, A) > 0
        assert not dW[~taken].any()
        for i in range(N):
            r = np.nonzero(taken[:, i].any(-1))[0]
            assert np.array_equal(dW[r, i, c["u"].reshape(R, N)[r, i]], db1[r]), i
    again = run_mix(c, N, A, E, inp, pad)
    for k in ("q", "dhy", "dx"):
        assert torch.equal(got[k], again[k]), k
    return got


# ---------------------------------------------------------------------------------------------------- mix_fwd / mix_bwd
@pytest.mark.parametrize("inp", ["x", "onehot", "u"])
@pytest.mark.parametrize("case", lo.CASES)
def test_mix_vs_rows(case, inp):
    """one row; a full tile and one row over; MMM2; the support corner K = 512, E = 64; an odd E without a 16-byte row pitch"""
    R, N, A, E = case
    c = lo.kernel_case(R, N, A, E, SEED)
    check_mix("lica_mix:%s %s" % ("x".join(map(str, case)), inp), c, N, A, E, inp)


@pytest.mark.parametrize("inp", ["x", "u"])
def test_mix_when_a_workgroup_walks_more_than_one_tile(inp):
    from marl_amd import ops
    R, N, A, E = lo.TILES_CASE
    tr, grid, lds, walks = ops.lica_plan(R, N, A, E)
    assert walks >= 2 and grid * tr < R, (tr, grid, walks)
    c = lo.kernel_case(R, N, A, E, SEED)
    check_mix("lica_mix:tiles %s" % inp, c, N, A, E, inp)


def test_plan_reports_the_tile():
    from marl_amd import ops
    assert ops.lica_plan(65, 5, 11, 32)[:2] == (32, 3) and ops.lica_plan(67, 16, 32, 64)[0] == 16
    assert ops.lica_plan(0, 5, 11, 32) == (0, 0, 0, 0)
    assert ops.lica_supported(16, 32, 64) and not ops.lica_supported(17, 32, 64) and not ops.lica_supported(5, 33, 32) \
        and not ops.lica_supported(5, 11, 65) and not ops.lica_supported(0, 11, 32)


@pytest.mark.parametrize("inp", ["x", "u"])
@pytest.mark.parametrize("case,pad", [((65, 5, 11, 32), 3), ((65, 5, 11, 32), 4), ((5, 3, 30, 7), 2)])
def test_wide_leading_dimensions_leave_the_gap_untouched(case, pad, inp):
    """ldh / lddh wider than needed (a pitch that keeps the 16-byte accesses, and two that do not): the sentinel in the gap stays"""
    R, N, A, E = case
    c = lo.kernel_case(R, N, A, E, SEED)
    check_mix("lica_mix:%s pad %d %s" % ("x".join(map(str, case)), pad, inp), c, N, A, E, inp, pad)


def test_an_index_outside_the_actions_is_an_all_zero_block():
    R, N, A, E = 65, 5, 11, 32
    c = lo.kernel_case(R, N, A, E, SEED)
    c["u"][3, 1], c["u"][40, 4], c["u"][64, 0] = -1, A, -1
    assert np.abs(lo.rows(c["hy"], N, A, E, u=c["u"])["pre"]).min() >= lo.KINK
    got = check_mix("lica_mix:bad index", c, N, A, E, "u")
    dW = got["dhy"].cpu().numpy()[:, :N * A * E].reshape(R, N, A * E)
    assert not dW[3, 1].any() and not dW[40, 4].any() and not dW[64, 0].any() and dW[3, 0].any()


# ---------------------------------------------------------------------------------------------------- loss_bwd
def run_loss(c, N, A, E, hy=None, u=None, q_tgt=None, r=None):
    from marl_amd import ops
    R, KE = len(c["hy"]), N * A * E
    hy = dev(c["hy"] if hy is None else hy)
    u = dev(c["u"] if u is None else u).reshape(-1)
    o = dict(q=_sent(R), dhy=_sent(R, KE + 2 * E), dq_tot=_sent(R), out2=_sent(2))
    ops.lica_loss_bwd(hy, u, dev(c["q_tgt"] if q_tgt is None else q_tgt), dev(c["r"] if r is None else r), dev(c["term"]),
                      dev(c["padded"]), lo.GAMMA, o["q"], o["dhy"], o["dq_tot"], o["out2"], R, N, A, E)
    return o


@pytest.mark.parametrize("case", [(65, 5, 11, 32), (130, 10, 18, 32)])
def test_loss_bwd_is_the_composition_bit_for_bit(case):
    """q, dhy, dq_tot and out2 of the one-launch form equal mix_fwd -> marl_td_loss -> mix_bwd"""
    from marl_amd import ops
    R, N, A, E = case
    c = lo.kernel_case(R, N, A, E, SEED)
    got = run_loss(c, N, A, E)
    hy, u = dev(c["hy"]), dev(c["u"]).reshape(-1)
    q, dq_tot, out2, dhy = _sent(R), _sent(R), _sent(2), _sent(R, N * A * E + 2 * E)
    ops.lica_mix_fwd(hy, None, u, q, R, N, A, E)
    ops.td_loss(q, dev(c["q_tgt"]), dev(c["r"]), dev(c["term"]), dev(c["padded"]), lo.GAMMA, dq_tot, out2, R)
    ops.lica_mix_bwd(hy, None, u, dq_tot, dhy, None, R, N, A, E)
    for k, want in (("q", q), ("dhy", dhy), ("dq_tot", dq_tot), ("out2", out2)):
        assert torch.equal(got[k], want), k
    assert float(got["out2"][1]) == float((c["padded"] == 0).sum())
    again = run_loss(c, N, A, E)
    for k in got:
        assert torch.equal(got[k], again[k]), k


@pytest.mark.parametrize("case", [(65, 5, 11, 32), (130, 10, 18, 32), (5, 3, 30, 7)])
def test_loss_bwd_vs_rows_with_nan_on_padded_rows(case):
    """NaN in hy, q_tgt and r of the padded rows and u = -7 there: exact zeros out, finite sums, the live rows as the oracle's"""
    R, N, A, E = case
    c = lo.kernel_case(R, N, A, E, SEED)
    pad = c["padded"] == 1
    assert pad.any()
    hy, q_tgt, r, u = c["hy"].copy(), c["q_tgt"].copy(), c["r"].copy(), c["u"].copy()
    hy[pad] = np.nan
    q_tgt[pad] = r[pad] = np.nan
    u[pad] = -7
    ref = lo.rows(c["hy"], N, A, E, u=c["u"], loss=dict(q_tgt=c["q_tgt"], r=c["r"], term=c["term"], padded=c["padded"], gamma=lo.GAMMA))
    got = run_loss(c, N, A, E, hy=hy, u=u, q_tgt=q_tgt, r=r)
    case = "lica_loss:%s" % "x".join(map(str, case))
    live = torch.tensor(~pad, device=DEV)
    parity.close(case, "q", got["q"][live].cpu().numpy(), ref["q"][~pad])
    for k in ("dhy", "dq_tot", "out2"):
        parity.close(case, k, got[k].cpu().numpy(), ref[k])
    assert not got["dhy"][~live].any() and not got["dq_tot"][~live].any()
    assert bool(torch.isfinite(got["out2"]).all()) and float(got["out2"][1]) == float((~pad).sum())


# ---------------------------------------------------------------------------------------------------- policy_probs_bwd
def run_probs_bwd(c, N, eps, beta, with_q=True, in_place=None):
    from marl_amd import ops
    R, A = c["logits"].shape
    z, a, g = dev(c["logits"]), dev(c["avail"]), dev(c["gpi"])
    out = {None: _sent(R, A), "logits": z, "gpi": g}[in_place]
    ent, out3 = _sent(R), _sent(3)
    ops.policy_probs_bwd(z, a, g, dev(c["q_pi"]) if with_q else None, dev(c["padded"]), eps, beta, out, ent, out3, R, N, A)
    return dict(dlogits=out, ent=ent, out3=out3)


@pytest.mark.parametrize("beta", lo.BETAS)
@pytest.mark.parametrize("eps", [0.0, 0.3])
@pytest.mark.parametrize("B,T,N,A", [(4, 6, 5, 11), (23, 7, 10, 18), (5, 4, 3, 30)])
def test_probs_bwd_vs_autograd(B, T, N, A, eps, beta):
    """rows with one available action, padded steps with logits and gpi of magnitude 1e6, whole rows shifted by +1e4; R = 120 (two
    tiles, the second partial), 1610 (seven workgroups) and A = 30 (the row-per-lane form).  q_pi NULL and given, in place on the
    logits and on gpi, two calls: equal bits"""
    c = lo.probs_bwd_case(B, T, N, A, seed=3)
    case = "probs_bwd:%dx%dx%dx%d eps=%g beta=%g" % (B, T, N, A, eps, beta)
    got = run_probs_bwd(c, N, eps, beta)
    for with_q, g in ((True, got), (False, run_probs_bwd(c, N, eps, beta, with_q=False))):
        ref = lo.probs_bwd_reference(c, N, eps, beta, with_q)
        for k in ("dlogits", "ent", "out3"):
            parity.close(case + (" q_pi" if with_q else ""), k, g[k].cpu().numpy(), ref[k])
        assert float(g["out3"][1]) == ref["out3"][1] == N * float((c["padded"] == 0).sum())
        assert torch.equal(g["dlogits"], got["dlogits"]) and torch.equal(g["ent"], got["ent"])
    pad, one = torch.tensor(c["pad_rows"], device=DEV), torch.tensor(c["one_rows"], device=DEV)
    assert not got["dlogits"][pad].any() and not got["ent"][pad].any()           # padded rows: exact zeros
    assert not got["dlogits"][one].any() and not got["ent"][one].any()           # one available action: exactly no gradient
    if eps == 0.0 and beta == 0.0:
        assert not got["dlogits"][dev(c["avail"]) == 0].any()                    # exactly 0 on unavailable actions
    for in_place in ("logits", "gpi"):
        o = run_probs_bwd(c, N, eps, beta, in_place=in_place)
        for k in got:
            assert torch.equal(o[k], got[k]), (in_place, k)
    again = run_probs_bwd(c, N, eps, beta)
    for k in got:
        assert torch.equal(got[k], again[k]), k


# ---------------------------------------------------------------------------------------------------- errors and empty shapes
def test_error_returns_and_empty_shapes():
    from marl_amd import _lib
    lib = _lib.load()
    INVALID = 1                                        # hipErrorInvalidValue
    R, N, A, E = 9, 3, 4, 8
    K, KE = N * A, N * A * E
    W = KE + 2 * E + 1
    c = lo.kernel_case(R, N, A, E, SEED)
    hy, x, u, dq = dev(c["hy"]), dev(c["x"]), dev(c["u"]).reshape(-1), dev(c["dq"])
    vec = dev(c["r"])
    q, dhy, dx, dq_tot, out2, ws = _sent(R), _sent(R, W), _sent(R, K), _sent(R), _sent(2), _sent(4096)
    outs = (q, dhy, dx, dq_tot, out2)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def fwd(hy=hy, ldh=W, x=None, u=u, q=q, rows=R, N=N, A=A, E=E):
        return lib.marl_lica_mix_fwd(p(hy), ldh, p(x), p(u), p(q), rows, N, A, E, None)

    def bwd(hy=hy, ldh=W, x=None, u=u, dq=dq, dhy=dhy, lddh=W, dx=dx, rows=R, N=N, A=A, E=E):
        return lib.marl_lica_mix_bwd(p(hy), ldh, p(x), p(u), p(dq), p(dhy), lddh, p(dx), rows, N, A, E, None)

    def loss(hy=hy, ldh=W, u=u, q_tgt=vec, r=vec, term=vec, padded=vec, q=q, dhy=dhy, lddh=W, dq_tot=dq_tot, out2=out2, ws=ws,
             rows=R, N=N, A=A, E=E):
        return lib.marl_lica_loss_bwd(p(hy), ldh, p(u), p(q_tgt), p(r), p(term), p(padded), 0.99, p(q), p(dhy), lddh, p(dq_tot),
                                      p(out2), p(ws), rows, N, A, E, None)
    shapes = (dict(N=17), dict(A=33), dict(E=65), dict(N=0), dict(A=0), dict(E=0))
    for f in (fwd, bwd, loss):
        for kw in shapes + (dict(hy=None), dict(u=None), dict(ldh=W - 1), dict(rows=1 << 31)):
            assert f(**kw) == INVALID, (f.__name__, kw)
        assert f(rows=0) == 0 and f(rows=-3) == 0
        assert f(rows=0, hy=None, u=None) == 0                               # rows <= 0: no launch, nothing looked at
    assert fwd(x=x) == INVALID and bwd(x=x) == INVALID                       # both of x and u
    assert fwd(q=None) == INVALID and bwd(dq=None) == INVALID
    assert bwd(dhy=None, dx=None) == INVALID and bwd(lddh=W - 2) == INVALID and loss(lddh=W - 2) == INVALID
    for name in ("q_tgt", "r", "term", "padded", "q", "dhy", "dq_tot", "out2", "ws"):
        assert loss(**{name: None}) == INVALID, name
    plan = (C.c_int * 4)()
    assert lib.marl_lica_plan(10, 17, 4, 8, plan) == INVALID and lib.marl_lica_plan(1 << 31, 3, 4, 8, plan) == INVALID
    # marl_policy_probs_bwd
    Rp, Np, Ap = 12, 3, 5
    z, a, g, pad, qp = _sent(Rp, Ap), torch.ones(Rp, Ap, device=DEV), _sent(Rp, Ap), torch.zeros(Rp // Np, device=DEV), _sent(Rp // Np)
    dz, ent, out3 = _sent(Rp, Ap), _sent(Rp), _sent(3)

    def pb(z=z, a=a, g=g, qp=qp, pad=pad, beta=0.0, dz=dz, ent=ent, out3=out3, ws=ws, rows=Rp, N=Np, A=Ap):
        return lib.marl_policy_probs_bwd(p(z), p(a), p(g), p(qp), p(pad), 0.1, beta, p(dz), p(ent), p(out3), p(ws), rows, N, A, None)
    for kw in (dict(z=None), dict(a=None), dict(g=None), dict(pad=None), dict(dz=None), dict(out3=None), dict(ws=None), dict(N=0),
               dict(N=5), dict(beta=-0.01), dict(beta=float("nan")), dict(dz=a)):
        assert pb(**kw) == INVALID, kw
    assert pb(rows=0) == 0 and pb(A=0) == 0 and pb(rows=0, z=None, a=None, g=None) == 0
    torch.cuda.synchronize()
    for t in outs + (dz, ent, out3):
        assert bool((t == SENT).all())                                       # nothing was written on any of them
    assert bool((a == 1).all())
    assert pb(qp=None, ent=None) == 0                                        # the optional ones
    torch.cuda.synchronize()
    assert not bool((dz == SENT).any()) and float(out3[1]) == Rp


# ---------------------------------------------------------------------------------------------------- the learner's wiring
@pytest.mark.parametrize("name", ["2s3z", "matrix"])
def test_hypernetworks_through_the_learners_lin_wiring(name):
    """hy = [W1 | b1 | wf | b2] from LICALearner._hyper_forward equals the torch module's four hypernetworks"""
    from marl_amd.algorithm.lica import LICALearner
    from marl_amd.controller.share_params import PolicyMAC
    args, state, batch = lo.learner_case(name)
    learner = LICALearner(PolicyMAC(args), args)
    learner.critic.load_state_dict({k: v.detach().float() for k, v in state.critic.items()})
    B, T, N, A, S = 7, 5, args.n_agents, args.n_actions, args.state_shape
    s = np.random.default_rng(2).standard_normal((B * T, S)).astype(np.float32)
    db = types.SimpleNamespace(B=B, T=T, N=N, A=A, s=dev(s))
    hy = learner._hyper_forward(learner.critic, db, "", False)
    with torch.no_grad():
        ref = torch.cat(lo.hyper(state.critic, torch.tensor(s.astype(np.float64))), dim=-1).numpy()
    assert hy.shape == ref.shape == (B * T, N * A * args.mixing_embed_dim + 2 * args.mixing_embed_dim + 1)
    parity.close("lica_hyper:" + name, "hy", hy.cpu().numpy(), ref)
    # and the module's own forward is the kernels' on that hy
    from marl_amd import ops
    x = np.random.default_rng(3).random((B * T, N * A)).astype(np.float32)
    q = _sent(B * T)
    ops.lica_mix_fwd(hy, dev(x), None, q, B * T, N, A, args.mixing_embed_dim)
    with torch.no_grad():
        want = lo.critic(state.critic, torch.tensor(x.astype(np.float64)), torch.tensor(s.astype(np.float64))).numpy()
    parity.close("lica_hyper:" + name, "Q", q.cpu().numpy(), want)
