"""COMA on the CPU: properties of tests/coma_oracle.py (the float64 restatement the GPU tests hold csrc/coma.hip and COMALearner to),
the launcher's argument table, and the float32 yardstick of every tensor the GPU file compares."""
import numpy as np
import pytest
import torch

import coma_oracle as co
import policy_oracle as po


def _forward(name, lam=0.8, beta=0.0, i=0):
    args, state, batch = co.learner_case(name, td_lambda=lam, policy_entropy_coef=beta)
    return args, state, batch, co.forward(state, batch(i), co.EPS, lam, beta)


@pytest.mark.parametrize("name", ["2s3z", "MMM2", "matrix"])
def test_factored_first_layer_equals_the_concatenated_one(name):
    """state product + observation product + gathered one-hot columns against one Linear over the (R, K) input: 1e-12 in float64"""
    args, state, batch, (_, _, inter) = _forward(name)
    b = batch(0)
    T = inter["T"]
    t = lambda k: torch.tensor(np.asarray(b[k])[:, :T], dtype=torch.float64)
    B, N, A = t("o").shape[0], args.n_agents, args.n_actions
    u = torch.tensor(np.asarray(b["u"])[:, :T]).reshape(B, T, N)
    x = inter["x"]
    assert x.shape[-1] == args.state_shape + args.obs_shape + 2 * N * A + N == state.critic["fc1.weight"].shape[1]
    if name == "matrix":
        assert x.shape[-1] == 16 and float(x[..., 2 + N * A:2 + 2 * N * A].abs().max()) == 0.0      # one-step episodes: no last action
    with torch.no_grad():
        whole = torch.nn.functional.linear(x, state.critic["fc1.weight"], state.critic["fc1.bias"])
        parts = co.factored_fc1(state.critic, t("s").reshape(B, T, -1), t("o"), u, A)
    assert float((whole - parts).abs().max()) <= 1e-12
    # agent i's own action block is zero, the others' blocks are their one-hots
    S, O = args.state_shape, args.obs_shape
    blocks = x[..., S + O:S + O + N * A].reshape(B, T, N, N, A)
    for i in range(N):
        assert float(blocks[:, :, i, i].abs().max()) == 0.0
    assert bool((blocks.sum(dim=(-1, -2)) == N - 1).all())


@pytest.mark.parametrize("name", ["2s3z", "MMM2", "matrix"])
def test_the_counterfactual_baseline_has_zero_mean_under_the_policy(name):
    """sum_k pi_k (Q_k - baseline) = 0 on every row with a policy"""
    args, state, batch, (_, _, inter) = _forward(name)
    b = batch(0)
    T = inter["T"]
    avail = torch.tensor(np.asarray(b["avail_u"])[:, :T], dtype=torch.float64)
    pi = po.policy(inter["logits"].detach(), avail, co.EPS)
    q = inter["q"].detach()
    base = (pi * q).sum(-1, keepdim=True)
    has = avail.sum(-1) > 0
    assert bool(has.any())
    assert float(((pi * (q - base)).sum(-1))[has].abs().max()) <= 1e-12
    # and Adv is Q(u) minus that baseline on the live rows
    live = (inter["mask"][:, :, None] > 0) & has
    u = torch.tensor(np.asarray(b["u"])[:, :T]).reshape(has.shape)
    qu = torch.gather(q, -1, u.unsqueeze(-1)).squeeze(-1)
    assert float((inter["adv"] - (qu - base.squeeze(-1)))[live].abs().max()) <= 1e-12


def test_q_next_is_zero_at_the_last_step_and_for_the_unterminated_episode():
    args, state, batch, (_, _, inter) = _forward("2s3z", lam=1.0)
    T = inter["T"]
    assert T == 5 < args.episode_limit
    qn = inter["q_next"]                                                                 # (B, N, T)
    assert float(qn[:, :, T - 1].abs().max()) == 0.0 and float(qn[:, :, :T - 1].abs().min()) > 0.0
    # episode 1 never terminates and is cut at T: at lambda = 1 its return is the discounted reward sum alone, no bootstrap
    r = np.asarray(batch(0)["r"])[1, :T, 0]
    want = sum(args.gamma ** k * r[k] for k in range(T))
    np.testing.assert_allclose(inter["td_targets"][1, 0].numpy(), want, rtol=1e-12)


def test_launcher_builds_the_coma_table(monkeypatch):
    import marl_amd.algorithm.coma  # noqa: F401
    from marl_amd import main
    monkeypatch.setattr(main, "SyntheticSMACEnv", lambda *a, **k: type("E", (), {"get_env_info": lambda s: dict(
        n_actions=11, n_agents=5, state_shape=120, obs_shape=80, episode_limit=120)})())
    args, _ = main.build(["--alg", "coma"])
    assert (args.lr_actor, args.lr_critic, args.critic_dim, args.td_lambda, args.epsilon) == (1e-4, 1e-3, 128, 0.8, 0.5)
    assert args.epsilon_anneal_scale == "episode" and args.target_update_cycle == 200
    args, _ = main.build(["--alg", "coma", "--td_lambda", "0.3"])
    assert args.td_lambda == 0.3


def test_critic_module_has_the_published_layout():
    from marl_amd.algorithm.coma import QCritic, critic_input_dim
    args, state, _ = co.learner_case("2s3z")
    c = QCritic(args)
    assert [(k, tuple(v.shape)) for k, v in c.state_dict().items()] == co.critic_param_shapes(args)
    assert critic_input_dim(args) == 315
    args, _, _ = co.learner_case("MMM2")
    assert critic_input_dim(args) == 868


# ---------------------------------------------------------------------------------------------------- float32 yardstick
def two_updates(name, dtype, lam, beta):
    """every tensor the GPU file compares, of two updates of a learner case"""
    _, state, batch = co.learner_case(name, dtype, td_lambda=lam, policy_entropy_coef=beta)
    out = {}
    for i in range(2):
        lc, la, grads, inter = co.train(state, batch(i), i, co.EPS, lam, beta)
        s = "step%d/" % i
        mask = inter["mask"].numpy()[:, :, None]
        out[s + "l_critic"], out[s + "l_actor"], out[s + "entropy"] = lc, la, float(inter["entropy"].detach())
        for k in ("q", "q_taken", "q_next", "adv", "logp", "ent"):
            out[s + k] = inter[k].detach().numpy()
        out[s + "td_targets"] = inter["td_targets"].numpy() * mask
        for k, g in grads.items():
            out[s + "grad " + k] = g.detach().numpy()
        for h in ("agent.", "critic."):
            out[s + h + "grad_norm"], out[s + h + "clip_coef"] = float(inter[h + "grad_norm"]), float(inter[h + "clip_coef"])
        for k, p in list(state.agent.items()):
            out[s + "param agent." + k] = p.detach().numpy().copy()
        for k, p in list(state.critic.items()):
            out[s + "param critic." + k] = p.detach().numpy().copy()
        out["near_zero"] = out.get("near_zero", 0) + co.relu_near_zero(inter)
    return out


@pytest.mark.parametrize("name,lam,beta", co.YARDSTICK_RUNS)
def test_float32_oracle_stays_under_a_quarter_of_the_bound(name, lam, beta):
    """The oracle in float32 against float64: a quarter of 1e-4 * max|ref| on every tensor, except those DESIGN section 10 lists with
    their measured float32-oracle error (co.F32_EXCEPTIONS; the GPU tests bound those alone by 4x that error)"""
    ref, f32 = two_updates(name, torch.float64, lam, beta), two_updates(name, torch.float32, lam, beta)
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
        exc = co.F32_EXCEPTIONS.get((name, lam, beta, k))
        if exc is not None:
            # no more than about the recorded size.  No lower limit: where RMSprop's step hangs on the rounding of a gradient near
            # zero, the float32 error depends on the host's summation order - the table holds the largest figure seen
            assert err <= 1.5 * exc, (k, err, exc)
        elif err > bound:
            worst[k] = (err, bound)
    assert not worst, worst


def test_kernel_case_contents():
    """the fc1 cases hold an action nobody takes and their pre-activations stay clear of the ReLU kink; the loss rows hold the
    special rows the GPU test relies on"""
    for (B, T, N, A, S, O) in co.FC1_SHAPES:
        assert (B * T * N) % 64 != 0
        for constant in (False, True):
            c = co.fc1_case(B, T, N, A, S, O, seed=co.FC1_SEED, constant=constant)
            assert not (c["u"] == A - 1).any()
            ref = co.fc1_reference(c, B, T, N, A)
            assert ref["near_zero"] == 0
            K0 = S + O
            for j in range(N):       # the never-taken action's columns: exactly zero, in the action and the last-action block
                assert float(np.abs(ref["dW"][:, K0 + j * A + A - 1]).max()) == 0.0
                assert float(np.abs(ref["dW"][:, K0 + N * A + j * A + A - 1]).max()) == 0.0
    rows = co.kernel_case(4, 6, 5, 11, seed=3)
    assert rows["pad_rows"].any() and len(rows["one_rows"]) > 0 and float(np.abs(rows["logits"]).max()) == 1.0e6
    ref = co.loss_reference(rows, 4, 6, 5, 0.3, 0.01)
    assert not ref["dlogits"][rows["pad_rows"]].any() and not ref["dq"][rows["pad_rows"]].any()
    assert float(np.abs(ref["adv"][rows["one_rows"]]).max()) == 0.0
