"""The CommNet actor without a GPU: the two statements of the head, CommNetAgent against the oracle, the identity-front argument,
the state dict, the launcher's tables and refusals, and the float32 yardstick of tests/test_gpu_commnet_learner.py's runs."""
import numpy as np
import pytest
import torch

from oracle import nets, seeded
import commnet_oracle as cn
import coma_oracle as co
import pg_oracle as pg
import policy_oracle as po

H = cn.H


def _head_params(A, seed, dtype=torch.float64):
    c = cn.head_case(3, 2, A, seed)
    return {k: torch.tensor(c[k].astype(np.float64), dtype=dtype) for k in cn.HEAD_PARAMS}


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("N", [2, 3, 5, 8, 10])
def test_the_two_head_forms_agree(N, K):
    p = _head_params(7, seed=N)
    h = torch.tanh(torch.tensor(np.random.default_rng(N + K).standard_normal((6 * N, H))))
    a, b = cn.head(p, h, N, K), cn.head_published(p, h, N, K)
    assert float((a - b).abs().max()) <= 1e-12
    if K == 1:                                   # round 0 still runs f_comm: decoding never sees h itself
        assert torch.equal(a, nets.lin(p, "decoding", cn.gru(p, "f_comm", torch.zeros_like(h), h)))
        assert float((a - nets.lin(p, "decoding", h)).abs().max()) > 1e-3


def _agent(shape="2s3z", k=3, **over):
    from marl_amd.network.commnet import CommNetAgent
    args = pg.make_args(shape, 6, **over)
    args.k = k
    I = args.obs_shape + (args.n_actions if args.last_action else 0) + (args.n_agents if args.reuse_network else 0)
    torch.manual_seed(4)
    return args, CommNetAgent(I, args), I


@pytest.mark.parametrize("k", [1, 2, 3])
def test_agent_forward_equals_the_oracle_step(k):
    args, agent, I = _agent(k=k)
    agent = agent.double()
    p = {n: x.detach() for n, x in agent.named_parameters()}
    rng = np.random.default_rng(k)
    x, h = torch.tensor(rng.standard_normal((3 * args.n_agents, I))), torch.tanh(torch.tensor(rng.standard_normal((3 * args.n_agents, H))))
    z, h_out = agent(x, h)
    zr, hr = cn.step(p, x, h, args.n_agents, k)
    assert float((z - zr).detach().abs().max()) <= 1e-12 and float((h_out - hr).detach().abs().max()) <= 1e-12
    # torch's own GRUCell is the gate order and formula of the oracle's gru
    assert float((agent.f_comm(x[:, :H], h).detach() - cn.gru(p, "f_comm", x[:, :H], h)).abs().max()) <= 1e-12


def test_identity_front_is_exact_in_float32():
    """relu(e I^T + 0) == e bit for bit for e = sigmoid(.) in float32: what lets the unroll kernels run f_obs unchanged"""
    _, agent, _ = _agent()
    x = torch.tensor(np.random.default_rng(0).standard_normal((4096, H)) * 30.0, dtype=torch.float32)
    x[::7, ::5] = -120.0                         # below float32's smallest exp: sigmoid gives e == 0 exactly, the edge of the argument
    x[1::7, ::3] = 120.0
    e = torch.sigmoid(x)
    assert float(e.min()) == 0.0 and float(e.max()) == 1.0 and bool((e[::7, ::5] == 0).all())
    y = torch.relu(e @ agent._front_w.T + agent._front_b)
    assert torch.equal(y, e)
    assert torch.equal(agent._front_w, torch.eye(H)) and float(agent._dummy_w.abs().max()) == 0.0


def test_state_dict_has_the_published_names_and_shapes():
    args, agent, I = _agent("MMM2")
    sd = agent.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == cn.param_shapes(args)
    assert list(sd)[:2] == ["encoding.weight", "encoding.bias"] and sd["encoding.weight"].shape == (64, I)
    assert len(list(agent.parameters())) == 12 and not any(p is b for p in agent.parameters() for b in agent.buffers())
    agent.load_state_dict({k: torch.zeros_like(v) for k, v in sd.items()})          # strict: the front-layer constants are not in it


# ---------------------------------------------------------------------------------------------------- launcher
@pytest.fixture
def fake_env(monkeypatch):
    from marl_amd import main
    made = []

    def env(*a, **k):
        made.append(1)
        return type("E", (), {"get_env_info": lambda s: dict(n_actions=11, n_agents=5, state_shape=120, obs_shape=80, episode_limit=120)})()
    monkeypatch.setattr(main, "SyntheticSMACEnv", env)
    monkeypatch.setitem(main.MAPS, "3m", (3, 30, 48, 9, 60))
    return made


def test_build_applies_the_tables(fake_env):
    from marl_amd import main
    args, _ = main.build(["--alg", "reinforce+commnet", "--map", "2s3z"])
    assert args.k == 3 and args.alg == "reinforce+commnet" and (args.lr_actor, args.epsilon_anneal_scale) == (1e-4, "episode")
    assert not hasattr(args, "td_lambda")
    args, _ = main.build(["--alg", "central_v+commnet", "--map", "3m"])
    assert args.k == 2 and args.td_lambda == 0.8
    args, _ = main.build(["--alg", "coma+commnet", "--map", "MMM2", "--commnet_k", "1", "--td_lambda", "0.3"])
    assert args.k == 1 and args.td_lambda == 0.3                      # a given --td_lambda survives the table
    args, _ = main.build(["--alg", "coma", "--map", "2s3z"])
    assert not hasattr(args, "k")


def test_refusals_before_anything_is_built(fake_env, tmp_path):
    from marl_amd import main
    from marl_amd.controller.share_params import CommNetMAC
    from marl_amd.runner import Runner
    from marl_amd.utils.logging import Logger
    for alg in ("qmix+commnet", "vdn+commnet", "qtran_base+commnet", "+commnet"):
        with pytest.raises(ValueError, match="central_v, coma or reinforce"):
            main.build(["--alg", alg])
    for sw in ("RTW", "world_model", "MAIC"):
        with pytest.raises(ValueError, match="not with " + sw):
            main.build(["--alg", "coma+commnet", "--" + sw, "True"])
    for k in ("0", "5"):
        with pytest.raises(ValueError, match="marl_commnet_supported"):
            main.build(["--alg", "reinforce+commnet", "--commnet_k", k])
    assert fake_env == []                                               # no environment was made by any of them
    args, env = main.build(["--alg", "reinforce+commnet", "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "model")])
    args.k = 7
    with pytest.raises(ValueError, match="marl_commnet_supported"):
        CommNetMAC(args)
    args.k = 3
    # the runner's own tables do not hold the name
    with pytest.raises(ValueError, match="cannot find!"):
        Runner(env, Logger(), args)
    # the switches are refused by the runner's existing logic too
    args.RTW = True
    with pytest.raises(ValueError, match="not with RTW"):
        main.make_runner(args, env, Logger())


def test_multi_rank_is_refused(monkeypatch):
    from marl_amd.algorithm import reinforce, policy_learner
    from marl_amd.controller.share_params import CommNetMAC
    args, _, _ = cn.learner_case("reinforce", "2s3z")
    mac = CommNetMAC(args)
    monkeypatch.setattr(policy_learner, "GradReducer", type("R", (), {"enabled": True}))
    with pytest.raises(NotImplementedError):
        reinforce.ReinforceLearner(mac, args)
    assert not hasattr(mac.agent, "_flat")


# ---------------------------------------------------------------------------------------------------- float32 yardstick
def two_updates(run, dtype, commnet=True):
    """every tensor the GPU learner file compares, of two updates of a run; ``commnet`` False: the plain oracle of the same case"""
    alg, name = run[0], run[1]
    beta = run[2] if alg == "reinforce" else (run[3] if alg == "coma" else 0.0)
    lam = None if alg == "reinforce" else run[2]
    over = dict(policy_entropy_coef=beta)
    if lam is not None:
        over["td_lambda"] = lam
    if commnet:
        args, state, batch = cn.learner_case(alg, name, dtype, **over)
    else:
        args, state, batch = {"reinforce": pg, "central_v": po, "coma": co}[alg].learner_case(name, dtype, **over)
    out = {}
    with cn.commnet_actor(cn.K_OF[name]):
        for i in range(2):
            s = "step%d/" % i
            if alg == "reinforce":
                loss, grads, inter = pg.train(state, batch(i), i, cn.EPS, beta)
                out[s + "l_actor"] = loss
            elif alg == "central_v":
                lc, la, grads, inter = po.train(state, batch(i), i, cn.EPS, lam)
                out[s + "l_critic"], out[s + "l_actor"], out[s + "v"] = lc, la, inter["v"].detach().numpy()
            else:
                lc, la, grads, inter = co.train(state, batch(i), i, cn.EPS, lam, beta)
                out[s + "l_critic"], out[s + "l_actor"] = lc, la
                for k in ("q", "q_taken", "q_next"):
                    out[s + k] = inter[k].detach().numpy()
                out[s + "adv"] = inter["adv"].detach().numpy() * inter["mask"].numpy()[:, :, None]
            m = inter["mask"].numpy()
            G = inter["td_targets"].detach().numpy()
            out[s + "td_targets"] = G * (m[:, :, None] if G.ndim == 3 else m)
            out[s + "logits"] = inter["logits"].detach().numpy() * m[:, :, None, None]
            out[s + "logp"] = inter["logp"].detach().numpy()
            if "ent" in inter:
                out[s + "ent"] = inter["ent"].detach().numpy()
            for k, g in grads.items():
                out[s + "grad " + k] = g.detach().numpy()
            for half in ("agent.", "critic."):
                if half + "grad_norm" in inter:
                    out[s + half + "grad_norm"], out[s + half + "clip_coef"] = inter[half + "grad_norm"], inter[half + "clip_coef"]
            for k, p in list(state.agent.items()):
                out[s + "param agent." + k] = p.detach().numpy().copy()
            for k, p in list(getattr(state, "critic", {}).items()):
                out[s + "param critic." + k] = p.detach().numpy().copy()
    return out


def _critic_key(k):
    t = k.split("/", 1)[1]
    return "critic." in t or t in ("l_critic", "v", "q", "q_taken", "q_next") or (t == "td_targets")


@pytest.mark.parametrize("run", cn.RUNS, ids=lambda r: "-".join(str(x) for x in r))
def test_float32_oracle_stays_under_a_quarter_of_the_bound(run):
    """The oracle in float32 against float64 on every run of the GPU learner file: a quarter of 1e-4 * max|ref| (+ parity's floor)
    on every compared tensor of both updates, under m where a tensor is masked.  The critic's tensors equal the plain oracle's bit
    for bit in float64 - V reads s alone, COMA's critic the batch's actions, G comes from the target critic - so their ReLU margins
    and float32 exceptions are the existing tables' (imported, not searched again); every other tensor that does not stay under is
    in commnet_oracle.F32_EXCEPTIONS with its float32-oracle error, derived here and never from GPU output."""
    alg = run[0]
    ref, f32 = two_updates(run, torch.float64), two_updates(run, torch.float32)
    if alg != "reinforce":
        plain = two_updates(run, torch.float64, commnet=False)
        for k, r in ref.items():
            if _critic_key(k):
                assert np.array_equal(np.asarray(r), np.asarray(plain[k])), k
    derived = {}
    for k, r in ref.items():
        r = np.asarray(r, dtype=np.float64)
        err = float(np.abs(np.asarray(f32[k], dtype=np.float64) - r).max())
        scale = float(np.abs(r).max())
        print("%-40s %-44s f32 err %.3e  max|ref| %.3e  share of 1e-4 max|ref| %.3f" % (run, k, err, scale, err / (1e-4 * scale + 1e-30)))
        if err > 0.25 * 1e-4 * scale + 1e-7 and not (alg != "reinforce" and _critic_key(k)):
            derived[run + (k,)] = err
    listed = {k: v for k, v in cn.F32_EXCEPTIONS.items() if k[:len(run)] == run and len(k) == len(run) + 1}
    assert set(derived) == set(listed), (derived, listed)
    for k, err in derived.items():
        assert err <= 1.5 * listed[k], (k, err, listed[k])
