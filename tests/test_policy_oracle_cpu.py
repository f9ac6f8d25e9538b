"""The stochastic policy and central-V on the CPU: properties of tests/policy_oracle.py (the float64 restatement the GPU tests hold
the kernels and the learner to), the sign of the actor gradient on the matrix game, the launcher's argument table, and the
float32 yardstick of every tensor the GPU files compare."""
import numpy as np
import pytest
import torch

import policy_oracle as po

EPSS = (0.0, 0.02, 0.5)


def _rows(seed, R=40, A=7):
    rng = np.random.default_rng(seed)
    z = torch.tensor(rng.standard_normal((R, A)) * 3.0)
    a = torch.tensor((rng.random((R, A)) < 0.6).astype(np.float64))
    a[:, 0] = 1.0
    a[:5] = 1.0                       # rows with every action available
    a[5:10] = 0.0
    a[5:10, 3] = 1.0                  # rows with exactly one (n = 1)
    u = torch.tensor([int(rng.choice(np.nonzero(r)[0])) for r in a.numpy()])
    return z, a, u


@pytest.mark.parametrize("eps", EPSS)
def test_policy_is_a_distribution_over_the_available_actions(eps):
    z, a, _ = _rows(1)
    a[-3:] = 0.0                      # rows without a policy
    pi = po.policy(z, a, eps)
    assert bool((pi[a == 0] == 0).all())
    np.testing.assert_allclose(pi[:-3].sum(-1).numpy(), 1.0, rtol=0, atol=1e-14)
    assert bool((pi[-3:] == 0).all()) and bool((po.log_prob(z, a, torch.zeros(len(z), dtype=torch.long), eps)[-3:] == 0).all())
    if eps == 0.0:
        masked = torch.softmax(z.masked_fill(a == 0, -float("inf"))[:-3], dim=-1)
        np.testing.assert_allclose(pi[:-3].numpy(), masked.numpy(), rtol=1e-13, atol=0)


@pytest.mark.parametrize("eps", EPSS)
def test_actor_gradient_agrees_with_a_central_difference(eps):
    """L_actor's numerator by every logit: autograd against (f(z + h) - f(z - h)) / 2h in float64, 1e-6 relative"""
    z, a, u = _rows(2)
    R, A = z.shape
    N = 2
    rng = np.random.default_rng(3)
    G, v = torch.tensor(rng.standard_normal(R // N)), torch.tensor(rng.standard_normal(R // N))
    padded = torch.zeros(R // N, dtype=torch.float64)
    f = lambda zz: po.actor_numerator(zz.view(R // N, N, A), a.view(R // N, N, A), u.view(R // N, N), G, v, padded, eps)[0]
    z.requires_grad_(True)
    (auto,) = torch.autograd.grad(f(z), z)
    h = 1e-6
    fd = torch.zeros_like(auto)
    with torch.no_grad():
        for r in range(R):
            for k in range(A):
                d = torch.zeros_like(z)
                d[r, k] = h
                fd[r, k] = (f(z + d) - f(z - d)) / (2 * h)
    assert float((auto - fd).abs().max()) <= 1e-6 * float(auto.abs().max())
    assert float(auto[5:10].abs().max()) < 1e-12          # one available action: log pi = 0 whatever the logits, no gradient
    if eps == 0.0:                    # and the closed form there: - Adv (delta_uk - pi_k)
        adv = (G - v).repeat_interleave(N)[:, None]
        onehot = torch.zeros(R, A, dtype=torch.float64).scatter_(1, u[:, None], 1.0)
        np.testing.assert_allclose(auto.numpy(), (-adv * (onehot - po.policy(z.detach(), a, 0.0))).numpy(), rtol=0, atol=1e-12)


UPDATES = 50      # oracle updates of the sign check (RMSprop's steps are about lr_actor = 1e-4 per weight: small, and enough for a sign)


def test_matrix_game_updates_raise_the_expected_payoff():
    """The sign of the actor gradient: on the nine joint actions of the payoff [[8,-12,-12],[-12,0,0],[-12,0,0]] the exact
    expected payoff under pi grows and the probability of a -12 outcome shrinks (strictly; no margin)"""
    _, state, batch = po.learner_case("matrix")
    pay0, bad0 = po.matrix_expectations(*po.matrix_policy(state))
    for i in range(UPDATES):
        po.train(state, batch(i), i, 0.0, 0.8)
    pay1, bad1 = po.matrix_expectations(*po.matrix_policy(state))
    assert pay1 > pay0 and bad1 < bad0, (pay0, pay1, bad0, bad1)


def test_launcher_builds_the_central_v_table(monkeypatch):
    import marl_amd.algorithm.central_v  # noqa: F401
    from marl_amd import main
    monkeypatch.setattr(main, "SyntheticSMACEnv", lambda *a, **k: type("E", (), {"get_env_info": lambda s: dict(
        n_actions=11, n_agents=5, state_shape=120, obs_shape=80, episode_limit=120)})())
    args, _ = main.build(["--alg", "central_v"])
    assert (args.lr_actor, args.lr_critic, args.critic_dim, args.td_lambda, args.epsilon) == (1e-4, 1e-3, 128, 0.8, 0.5)
    assert args.epsilon_anneal_scale == "episode"
    args, _ = main.build(["--alg", "central_v", "--td_lambda", "0.3"])
    assert args.td_lambda == 0.3
    args, _ = main.build(["--alg", "qmix"])
    assert args.td_lambda is None and args.epsilon == 1 and not hasattr(args, "lr_actor")


# ---------------------------------------------------------------------------------------------------- float32 yardstick
def two_updates(name, dtype, lam=0.8):
    """every tensor the GPU files compare, of two updates of a learner case"""
    _, state, batch = po.learner_case(name, dtype, td_lambda=lam)
    out = {}
    for i in range(2):
        lc, la, grads, inter = po.train(state, batch(i), i, po.EPS, lam)
        s = "step%d/" % i
        out[s + "l_critic"], out[s + "l_actor"] = lc, la
        for k in ("v", "td_targets", "adv", "logp"):
            out[s + k] = inter[k].detach().numpy()
        for k, g in grads.items():
            out[s + "grad " + k] = g.detach().numpy()
        out[s + "clip actor"], out[s + "clip critic"] = inter["agent.clip_coef"], inter["critic.clip_coef"]
        for k, p in list(state.agent.items()):
            out[s + "param agent." + k] = p.detach().numpy().copy()
        for k, p in list(state.critic.items()):
            out[s + "param critic." + k] = p.detach().numpy().copy()
        out["near_zero"] = out.get("near_zero", 0) + po.relu_near_zero(inter)        # both updates: the GPU file asserts it of each
    return out


@pytest.mark.parametrize("name,lam", po.YARDSTICK_RUNS)
def test_float32_oracle_stays_under_a_quarter_of_the_bound(name, lam):
    """The oracle in float32 against float64: a quarter of 1e-4 * max|ref| on every tensor, except those DESIGN section 10 lists
    with their measured float32-oracle error (po.F32_EXCEPTIONS; the GPU tests bound those alone by 4x that error)"""
    ref, f32 = two_updates(name, torch.float64, lam), two_updates(name, torch.float32, lam)
    assert ref["near_zero"] == 0, "a ReLU pre-activation within 1e-5 of zero: choose another seed"
    worst = {}
    for k, r in ref.items():
        if k == "near_zero":
            continue
        r = np.asarray(r, dtype=np.float64)
        err = float(np.abs(np.asarray(f32[k], dtype=np.float64) - r).max())
        scale = float(np.abs(r).max())
        print("%-8s %-40s f32 err %.3e  max|ref| %.3e  share of 1e-4 max|ref| %.3f" % (name, k, err, scale, err / (1e-4 * scale + 1e-30)))
        bound = 0.25 * 1e-4 * scale + 1e-7
        exc = po.F32_EXCEPTIONS.get((name, lam, k))
        if exc is not None:
            assert bound < err <= 1.5 * exc, (k, err, exc)          # still an exception, and still about the recorded size
        elif err > bound:
            worst[k] = (err, bound)
    assert not worst, worst


def test_sampler_restatement_rarely_draws_near_a_cdf_boundary():
    """the GPU comparison leaves out draws within 1e-5 of a float64 CDF boundary, on the condition that they are under 0.5 % of
    the draws: the restatement alone, on the seeds that test uses (expected share at 11 actions: about 2e-4)"""
    for tg, eps, seed in po.SAMPLER_SEEDS:
        z, a, alive = po.sampler_case(4096, 5, 11, seed)
        act, margin, u = po.sample(z, a, alive, eps, 5, 100, tg)
        live = alive != 0
        assert float((margin[live] < po.SAMPLER_EXCLUDE).mean()) < po.SAMPLER_CAP
        assert bool((act[~live] == -1).all()) and bool((np.take_along_axis(a[live], act[live][..., None], -1) == 1).all())
        assert ((0 <= u) & (u < 1)).all()
