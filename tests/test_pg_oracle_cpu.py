"""The entropy bonus and REINFORCE on the CPU: properties of tests/pg_oracle.py (the float64 restatement the GPU tests hold
marl_policy_loss_bwd_ex, ReinforceLearner and central-V's bonus to), the C-ABI entry's signature, the launcher's argument table,
and the float32 yardstick of every tensor the GPU file compares."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pg_oracle as pg
import policy_oracle as po
from test_policy_oracle_cpu import _rows

EPSS = (0.0, 0.02, 0.5)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(seed, R=40, N=2):
    z, a, u = _rows(seed, R)
    rng = np.random.default_rng(seed + 1)
    G, v = torch.tensor(rng.standard_normal(R // N)), torch.tensor(rng.standard_normal(R // N))
    return z, a, u, G, v, torch.zeros(R // N, dtype=torch.float64)


def _num(z, a, u, G, v, padded, eps, beta, N=2):
    R, A = z.shape
    return pg.numerator(z.view(R // N, N, A), a.view(R // N, N, A), u.view(R // N, N), G, v, padded, eps, beta)


@pytest.mark.parametrize("with_v", [True, False])
@pytest.mark.parametrize("eps", EPSS)
def test_gradient_agrees_with_a_central_difference(eps, with_v):
    """the numerator with beta = 1 by every logit: autograd against (f(z + h) - f(z - h)) / 2h in float64, 1e-6 relative"""
    z, a, u, G, v, padded = _case(2)
    v = v if with_v else None
    R, A = z.shape
    f = lambda zz: _num(zz, a, u, G, v, padded, eps, 1.0)[0]
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
    assert float(auto[5:10].abs().max()) < 1e-12          # one available action: H = 0 and log pi = 0 whatever the logits hold
    if eps == 0.0:                    # the closed form there: Adv' (delta_uk - pi_k) + pi_k (log pi_k + H), 0 on unavailable actions
        adv = (G if v is None else G - v).repeat_interleave(2)[:, None]
        onehot = torch.zeros(R, A, dtype=torch.float64).scatter_(1, u[:, None], 1.0)
        pi = po.policy(z.detach(), a, 0.0)
        H = pg.entropy(z.detach(), a, 0.0)[:, None]
        logpi = torch.log(torch.where(pi > 0, pi, torch.ones_like(pi)))
        np.testing.assert_allclose(auto.numpy(), (-adv * (onehot - pi) + pi * (logpi + H)).numpy(), rtol=0, atol=1e-12)
        assert float(auto[a == 0].abs().max()) < 1e-12


def test_entropy_at_eps_zero_is_the_categorical_entropy_over_the_available_actions():
    z, a, _ = _rows(1)
    H = pg.entropy(z, a, 0.0)
    for r in range(len(z)):
        k = a[r] > 0
        want = torch.distributions.Categorical(logits=z[r][k]).entropy()
        assert abs(float(H[r]) - float(want)) <= 1e-12
    assert float(H[5:10].abs().max()) == 0.0               # n = 1


@pytest.mark.parametrize("eps", EPSS)
def test_beta_zero_with_v_is_policy_oracles_loss_and_gradient(eps):
    z, a, u, G, v, padded = _case(3)
    padded[3] = 1.0
    R, A = z.shape
    z.requires_grad_(True)
    num, logp, H, den, _ = _num(z, a, u, G, v, padded, eps, 0.0)
    num0, logp0, den0 = po.actor_numerator(z.view(R // 2, 2, A), a.view(R // 2, 2, A), u.view(R // 2, 2), G, v, padded, eps)
    (g,), (g0,) = torch.autograd.grad(num, z), torch.autograd.grad(num0, z)
    assert abs(float(num.detach()) - float(num0.detach())) <= 1e-12 and float(den) == float(den0)
    assert float((g - g0).abs().max()) <= 1e-12
    m = (1.0 - padded)[:, None]
    assert float((logp - m * logp0).detach().abs().max()) <= 1e-12   # (this oracle's log pi is 0 on a padded step, as the kernel's output is)


@pytest.mark.parametrize("eps", [0.0, 0.3])
def test_special_rows(eps):
    """one available action; a taken action that is not available; a logit 200 below the largest available one; NaN logits on a
    padded step"""
    A = 6
    z = torch.tensor([[0.3, -1.0, 2.0, 0.5, 0.0, 1.0]] * 4, dtype=torch.float64)
    a = torch.tensor([[0, 0, 1, 0, 0, 0], [1, 1, 0, 1, 1, 1], [1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]], dtype=torch.float64)
    u = torch.tensor([2, 2, 0, 1])
    z[2, 4] = z[2].max() - 200.0
    z[3] = float("nan")
    G, padded = torch.tensor([0.7, -1.3, 0.4, 1e6]), torch.tensor([0.0, 0.0, 0.0, 1.0])
    z.requires_grad_(True)
    num, logp, H, den, hsum = pg.numerator(z.view(4, 1, A), a.view(4, 1, A), u.view(4, 1), G.double(), None, padded.double(), eps, 1.0)
    (g,) = torch.autograd.grad(num, z)
    num, logp, H, hsum = (x.detach() for x in (num, logp, H, hsum))
    assert bool(torch.isfinite(num)) and bool(torch.isfinite(g).all()) and float(den) == 3.0
    assert float(H[0]) == 0.0 and float(logp[0]) == 0.0 and float(g[0].abs().max()) < 1e-12          # n = 1
    assert float(H[1]) == 0.0 and float(logp[1]) == 0.0 and not g[1].any()         # the taken action is unavailable: no policy
    assert float(H[3]) == 0.0 and float(logp[3]) == 0.0 and not g[3].any()         # padded: its NaN logits are never looked at
    assert float(H[2]) > 0.0 and float(hsum) == float(H[2])
    # why the 0 log 0 rule exists: in float32 the probability 200 below underflows to 0 at eps = 0 and a naive pi log pi is NaN
    pi32 = po.policy(z.detach()[2].float(), a[2].float(), eps)
    naive = pi32 * torch.log(pi32)
    if eps == 0.0:
        assert float(pi32[4]) == 0.0 and bool(torch.isnan(naive[4]))
    H32 = pg.entropy(z.detach()[2].float(), a[2].float(), eps)
    assert bool(torch.isfinite(H32)) and abs(float(H32) - float(H[2])) <= 1e-5


def test_cabi_signature_of_the_ex_entry():
    """header == ctypes table == library for marl_policy_loss_bwd_ex (tests/test_cabi.py holds the whole set)"""
    from marl_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "marl_hip.h")).read(), flags=re.S)
    m = re.search(r"int\s+marl_policy_loss_bwd_ex\s*\((.*?)\)\s*;", txt, flags=re.S)
    assert m, "not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    res, argt = _lib.SIGNATURES["marl_policy_loss_bwd_ex"]
    assert len(params) == len(argt) == 17 and res is ctypes.c_int
    for p, t in zip(params, argt):
        want = ctypes.c_void_p if "*" in p else ctypes.c_float if p.startswith("float") else ctypes.c_long if p.startswith("long") \
            else ctypes.c_int
        assert t is want, (p, t)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "marl_policy_loss_bwd_ex")


def test_launcher_builds_the_reinforce_table(monkeypatch):
    from marl_amd import main
    monkeypatch.setattr(main, "SyntheticSMACEnv", lambda *a, **k: type("E", (), {"get_env_info": lambda s: dict(
        n_actions=11, n_agents=5, state_shape=120, obs_shape=80, episode_limit=120)})())
    args, _ = main.build(["--alg", "reinforce"])
    assert (args.lr_actor, args.epsilon, args.epsilon_anneal_scale, args.policy_entropy_coef) == (1e-4, 0.5, "episode", 0.0)
    assert not hasattr(args, "td_lambda")                  # the reference's table has none
    args, _ = main.build(["--alg", "central_v", "--policy_entropy_coef", "0.01"])
    assert args.policy_entropy_coef == 0.01 and args.td_lambda == 0.8
    args, _ = main.build(["--alg", "qmix"])
    assert args.policy_entropy_coef == 0.0 and args.epsilon == 1


# ---------------------------------------------------------------------------------------------------- float32 yardstick
def two_updates(alg, name, beta, dtype):
    """every tensor the GPU file compares, of two updates of a learner case"""
    out = {"near_zero": 0}
    if alg == "reinforce":
        _, state, batch = pg.learner_case(name, dtype, policy_entropy_coef=beta)
    else:
        _, state, batch = po.learner_case(name, dtype, policy_entropy_coef=beta)
    for i in range(2):
        s = "step%d/" % i
        if alg == "reinforce":
            loss, grads, inter = pg.train(state, batch(i), i, pg.EPS, beta)
            out[s + "loss"] = loss
        else:
            lc, la, grads, inter = pg.central_v_train(state, batch(i), i, pg.EPS, 0.8, beta)
            out[s + "l_critic"], out[s + "l_actor"] = lc, la
            out[s + "v"], out[s + "clip critic"] = inter["v"].detach().numpy(), inter["critic.clip_coef"]
        out[s + "entropy"] = float(inter["entropy"].detach())
        for k in ("td_targets", "logp", "ent"):
            out[s + k] = inter[k].detach().numpy()
        for k, g in grads.items():
            out[s + "grad " + k] = g.detach().numpy()
        out[s + "clip actor"] = inter["agent.clip_coef"]
        for k, p in list(state.agent.items()):
            out[s + "param agent." + k] = p.detach().numpy().copy()
        for k, p in list(getattr(state, "critic", {}).items()):
            out[s + "param critic." + k] = p.detach().numpy().copy()
        out["near_zero"] += po.relu_near_zero(inter)
    return out


@pytest.mark.parametrize("alg,name,beta", pg.YARDSTICK_RUNS)
def test_float32_oracle_stays_under_a_quarter_of_the_bound(alg, name, beta):
    """The oracle in float32 against float64: a quarter of 1e-4 * max|ref| on every tensor, except those DESIGN section 10 lists
    with their measured float32-oracle error (pg.F32_EXCEPTIONS; the GPU tests bound those alone by 4x that error)"""
    ref, f32 = two_updates(alg, name, beta, torch.float64), two_updates(alg, name, beta, torch.float32)
    assert ref["near_zero"] == 0, "a ReLU pre-activation within 1e-5 of zero: choose another seed"
    worst = {}
    for k, r in ref.items():
        if k == "near_zero":
            continue
        r = np.asarray(r, dtype=np.float64)
        err = float(np.abs(np.asarray(f32[k], dtype=np.float64) - r).max())
        scale = float(np.abs(r).max())
        print("%-9s %-7s %-5g %-40s f32 err %.3e  max|ref| %.3e  share of 1e-4 max|ref| %.3f"
              % (alg, name, beta, k, err, scale, err / (1e-4 * scale + 1e-30)))
        bound = 0.25 * 1e-4 * scale + 1e-7
        exc = pg.F32_EXCEPTIONS.get((alg, name, beta, k))
        if exc is not None:
            assert bound < err <= 1.5 * exc, (k, err, exc)          # still an exception, and still about the recorded size
        elif err > bound:
            worst[k] = (err, bound)
    assert not worst, worst
