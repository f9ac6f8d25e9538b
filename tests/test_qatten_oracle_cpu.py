"""tests/qatten_oracle.py against itself, and the host logic of --alg qatten.  No GPU.

The folded analytic contract (``rows``) equals autograd of the unfolded textbook form; the key layer in swapped roles gives autograd's
gradients; the float32 twin fixes the constants of the GPU bounds; the learner seeds are well conditioned; state_dict keys, argument
defaults, launcher and runner refusals."""
import types

import numpy as np
import pytest
import torch

from oracle import seeded
import qatten_oracle as qo

ALL = qo.CASES + [(70, 2, 1, 1, 2)]


def _unfolded(c, seed=0):
    """a case's p written as e Wk: e (H x (R, D)), Wk (H x (D, U)) random, p = e Wk per head - in float64, so nothing is rounded"""
    g = np.random.default_rng(seed)
    D = 8
    e = [torch.tensor(g.standard_normal((c.R, D)), requires_grad=True) for _ in range(c.H)]
    Wk = [torch.tensor(g.standard_normal((D, c.U)), requires_grad=True) for _ in range(c.H)]
    p = torch.cat([a.detach() @ W.detach() for a, W in zip(e, Wk)], 1).numpy() / np.sqrt(D) / c.scale
    return e, Wk, p, D


@pytest.mark.parametrize("shape", ALL, ids=str)
@pytest.mark.parametrize("with_loss", [False, True])
def test_folded_rows_equal_autograd_of_the_unfolded_mix(shape, with_loss):
    c = qo.kernel_case(*shape, seed=shape[0])
    e, Wk, p, D = _unfolded(c)
    t = lambda x: torch.tensor(np.asarray(x, dtype=np.float64))
    w_raw, cc, q = (t(x).requires_grad_(True) for x in (c.w_raw, c.c, c.q))
    s = t(np.nan_to_num(c.s))
    q_tot = qo.attend(e, Wk, w_raw, cc, q, s, c.N, c.U, D)
    o = qo.rows(c.s, p, c.w_raw, c.c, c.q, c.scale, c.N, c.U, c.H, g=None if with_loss else c.g, loss=c.loss if with_loss else None)
    if with_loss:
        q_tgt, r, term, padded, gamma = c.loss
        m = 1.0 - t(padded)
        L = ((m * (t(r) + gamma * t(q_tgt) * (1 - t(term)) - q_tot)) ** 2).sum()
        assert abs(o.num - float(L)) <= 1e-12 * max(float(L), 1.0) and o.den == float(m.sum())
    else:
        L = (q_tot * t(c.g)).sum()
    grads = torch.autograd.grad(L, [q, w_raw, cc] + e + Wk)
    close = lambda name, got, ref: np.testing.assert_allclose(got, ref.detach().numpy(), rtol=0, atol=1e-12 * max(float(ref.detach().abs().max()), 1e-30),
                                                               err_msg=name)
    close("q_tot", o.q_tot, q_tot)
    close("dq", o.dq, grads[0])
    close("dw_raw", o.dw_raw, grads[1])
    close("dq_tot (dc)", o.dq_tot, grads[2])
    # the key layer in swapped roles: p = e Wk, dWk = e^T dp, de = dp Wk^T (the scale of this test's p folded back)
    dp = o.dp.reshape(c.R, c.H, c.U) / np.sqrt(D) / c.scale
    for h in range(c.H):
        close("de_%d" % h, dp[:, h] @ Wk[h].detach().numpy().T, grads[3 + h])
        close("dWk_%d" % h, e[h].detach().numpy().T @ dp[:, h], grads[3 + c.H + h])


def test_one_agent_and_planted_rows():
    c = qo.kernel_case(1, 1, 1, 1, 1)
    o = qo.oracle_of(c)
    assert o.lam.item() == 1.0 and (o.dp == 0).all() and o.q_tot.item() == abs(float(c.w_raw[0, 0])) * float(c.q[0, 0]) + float(c.c[0])
    c = qo.kernel_case(65, 5, 24, 4, 120)
    o = qo.oracle_of(c, loss=True)
    P = qo.PLANTED
    assert (o.dw_raw[P["w_zero"], 0] == 0) and (c.w_raw[P["w_zero"], 1:] < 0).all()
    np.testing.assert_allclose(o.lam[P["p_zero"], 0], 1.0 / c.N, rtol=1e-15)
    l = c.scale * (c.p[3, :c.U].astype(np.float64) * c.s[3, :c.N * c.U].reshape(c.N, c.U)).sum(1)
    assert l.max() - np.sort(l)[-2] >= 100 and np.isfinite(o.dp).all() and abs(o.lam[P["saturated"], 0].max() - 1) < 1e-12
    dead = c.padded == 1
    assert dead.any() and (c.term == 1).any()
    for x in (o.dq, o.dp, o.dw_raw, o.dq_tot):
        assert (x[dead] == 0).all()
    assert np.isnan(qo.kernel_case(129, 10, 32, 4, 322).s[:, 320:]).all()


KS = (("q_tot", qo.K_QTOT), ("dq", qo.K_DQ), ("dw_raw", qo.K_DW), ("dp", qo.K_DP), ("dp_wide", qo.K_DP_WIDE))


def test_float32_twin_fixes_the_bound_constants():
    worst = dict(q_tot=0.0, dq=0.0, dw_raw=0.0, dp=0.0, dp_wide=0.0)
    for shape in ALL:
        c = qo.kernel_case(*shape, seed=shape[0])
        o, t = qo.oracle_of(c), qo.twin32(c.s, c.p, c.w_raw, c.c, c.q, c.scale, c.N, c.U, c.H, g=c.g)
        b = qo.bounds(o)
        for k, K in KS:
            err = np.abs(getattr(t, k[:2]).astype(np.float64) - getattr(o, k[:2])) if k.startswith("dp") else \
                np.abs(getattr(t, k).astype(np.float64) - getattr(o, k))
            bound = getattr(b, k) / K
            live = bound > 0
            assert (err[~live] == 0).all(), (shape, k)
            if live.any():
                worst[k] = max(worst[k], float((err[live] / bound[live]).max()))
    print("twin32 / rows, worst err / (u (1 + L) mag):", {k: round(v, 3) for k, v in worst.items()})
    for k, K in KS:
        assert worst[k] <= K / 4, (k, worst[k])
        assert K == 2.0 ** np.ceil(np.log2(4 * worst[k])), (k, worst[k], K)      # four times the ratio, rounded up to a power of two


@pytest.mark.parametrize("name", sorted(qo.LEARNER_CASES))
def test_learner_cases_are_well_conditioned(name):
    """the float32 run of the oracle learner passes the GPU test's parity bounds against the float64 run - in each of three
    rounding draws, with a margin of two"""
    assert qo.float32_fraction(name) <= 0.5


def test_train_steps_and_syncs_the_target():
    args, st, batch, _ = qo.learner_case("double_q", target_update_cycle=2)
    start = {k: x.detach().clone() for k, x in st.mixer.items()}
    for i in range(3):
        loss, grads, inter = qo.train(st, batch(i), i)
        assert np.isfinite(loss) and all(g is not None and torch.isfinite(g).all() for g in grads.values())
        same = all(torch.equal(st.target_mixer[k], start[k]) for k in start)
        assert same == (i < 2)
    assert all(torch.equal(st.target_mixer[k], st.mixer[k].detach()) for k in start)


# ------------------------------------------------------------------------------------------------ host logic
def test_state_dict_keys():
    from marl_amd.network.mixer import QattenMixer
    args = seeded.make_args("2s3z", "qatten")
    m = QattenMixer(args)
    assert list(m.state_dict()) == [k for k, _ in qo.param_shapes(args)]
    assert [tuple(v.shape) for v in m.state_dict().values()] == [s for _, s in qo.param_shapes(args)]
    assert (m.n_heads, m.embed_dim, m.unit_dim) == (4, 32, 24)
    for over in (dict(n_agents=17, state_shape=17 * 4), dict(qatten_unit_dim=65, state_shape=400), dict(qatten_heads=9),
                 dict(qatten_unit_dim=0), dict(qatten_unit_dim=25)):
        with pytest.raises(ValueError, match="qatten"):
            QattenMixer(seeded.make_args("2s3z", "qatten", **over))


@pytest.mark.parametrize("name, want", [("2s3z", 24), ("3s5z", 27), ("MMM2", 32)])
def test_argument_table(name, want):
    from marl_amd.common.arguments import get_qatten_args
    a = get_qatten_args(seeded.make_args(name, "qatten", qatten_heads=None, qatten_embed_dim=None, qatten_unit_dim=None))
    assert (a.qatten_heads, a.qatten_embed_dim, a.qatten_unit_dim) == (4, 32, want)
    b = get_qatten_args(seeded.make_args(name, "qatten", qatten_heads=2, qatten_embed_dim=16, qatten_unit_dim=3))
    assert (b.qatten_heads, b.qatten_embed_dim, b.qatten_unit_dim) == (2, 16, 3)


def test_launcher_refuses_before_the_environment_is_made():
    from marl_amd import main
    with pytest.raises(ValueError, match="state of width 1"):
        main.build(["--env", "matrix", "--alg", "qatten", "--n_envs", "8"])
    for extra in (["--qatten_unit_dim", "25"], ["--qatten_heads", "9"], ["--qatten_unit_dim", "65", "--map", "MMM2"]):
        with pytest.raises(ValueError, match="qatten"):
            main.build(["--alg", "qatten", "--map", "2s3z", "--n_envs", "8"] + extra)
    for suffix in ("+commnet", "+g2anet"):
        with pytest.raises(ValueError):
            main.actor_base("qatten" + suffix)
    assert main.actor_base("qatten") == ("qatten", None)


class _Logger:
    def setup_tb(self, path):
        pass


def _runner_with_stubs(monkeypatch, tmp_path, **over):
    from marl_amd import runner
    built = []
    for name in ("RolloutWorker", "ReplayBuffer", "SharedMAC", "IQLLearner", "QLearner", "QTRANLearner"):
        monkeypatch.setattr(runner, name, lambda *a, _n=name, **k: built.append(_n) or types.SimpleNamespace(kind=_n, record_sink=None))
    args = seeded.make_args("2s3z", "qatten")
    args.result_dir = str(tmp_path)
    args.__dict__.update(over)
    return runner, args, built


def test_runner_selects_qlearner(monkeypatch, tmp_path):
    runner, args, built = _runner_with_stubs(monkeypatch, tmp_path)
    r = runner.Runner(None, _Logger(), args)
    assert r.learner.kind == "QLearner" and r.mac.kind == "SharedMAC" and not r.on_policy
    assert built == ["SharedMAC", "RolloutWorker", "ReplayBuffer", "QLearner"]


@pytest.mark.parametrize("switch", ["RTW", "world_model", "MAIC"])
def test_runner_refuses_the_agent_switches_before_anything_is_built(switch, monkeypatch, tmp_path):
    runner, args, built = _runner_with_stubs(monkeypatch, tmp_path, **{switch: True})
    with pytest.raises(ValueError, match="qatten .* not with " + switch):
        runner.Runner(None, _Logger(), args)
    assert built == []
