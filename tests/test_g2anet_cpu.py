"""The G2ANet actor without a GPU: the two statements of the head, G2ANetAgent and torch's own bidirectional GRU against the oracle,
the state dict, the launcher's tables and refusals, the conditions the GPU head cases rely on, and the float32 yardstick of
tests/test_gpu_g2anet.py's head cases and tests/test_gpu_g2anet_learner.py's runs."""
import functools

import numpy as np
import pytest
import torch

import g2anet_oracle as go
import coma_oracle as co
import pg_oracle as pg
import policy_oracle as po

H = go.H


def _content(G, N, A, seed, dtype=torch.float64):
    c = go.head_case(G, N, A, seed)
    t = lambda k: torch.tensor(c[k].astype(np.float64), dtype=dtype)
    return {k: t(k) for k in go.HEAD_PARAMS}, t("hs"), t("noise")


@pytest.mark.parametrize("tau", [0.01, 1.0])
@pytest.mark.parametrize("hard", [True, False])
@pytest.mark.parametrize("N", [2, 3, 5, 8, 10])
def test_the_two_head_forms_agree(N, hard, tau):
    p, h, l = _content(6, N, 7, seed=N)
    a, b = go.head(p, h, l, N, hard, tau), go.head_published(p, h, l, N, hard, tau)
    assert float((a - b).abs().max()) <= 1e-12
    if not hard:                                 # w = 1: the noise and the hard layers are not read
        assert torch.equal(a, go.head(p, h, None, N, hard, tau))
    else:
        assert float((a - go.head(p, h, None, N, hard, tau)).abs().max()) > 1e-6


def _agent(shape="2s3z", hard=True, **over):
    from marl_amd.network.g2anet import G2ANetAgent
    args = pg.make_args(shape, 6, **over)
    args.hard, args.attention_dim = hard, 32
    I = args.obs_shape + (args.n_actions if args.last_action else 0) + (args.n_agents if args.reuse_network else 0)
    torch.manual_seed(4)
    return args, G2ANetAgent(I, args), I


@pytest.mark.parametrize("hard", [True, False])
def test_agent_forward_equals_the_oracle_step(hard):
    args, agent, I = _agent(hard=hard)
    agent = agent.double()
    N = args.n_agents
    p = {n: x.detach() for n, x in agent.named_parameters()}
    rng = np.random.default_rng(3)
    x, h = torch.tensor(rng.standard_normal((3 * N, I))), torch.tanh(torch.tensor(rng.standard_normal((3 * N, H))))
    l = torch.tensor(go.logistic(rng.integers(0, 1 << 24, size=(3 * N, N - 1))))
    z, h_out = agent(x, h, l)
    zr, hr = go.step(p, x, h, l, N, hard, go.TAU)
    assert float((z - zr).detach().abs().max()) <= 1e-12 and float((h_out - hr).detach().abs().max()) <= 1e-12
    # torch's own GRUCell and bidirectional GRU are the gate order and the two chains of the oracle
    assert float((agent.h(x[:, :H], h).detach() - go.gru(p, "h", x[:, :H], h)).abs().max()) <= 1e-12
    hg = h.reshape(3, N, H)
    part = go.partners(N)
    seq = torch.cat([hg.unsqueeze(2).expand(-1, -1, N - 1, -1), hg[:, part]], -1).permute(2, 0, 1, 3).reshape(N - 1, 3 * N, 2 * H)
    y, _ = agent.hard_bi_GRU(seq)
    s, fwd = torch.zeros(3 * N, H, dtype=torch.float64), []
    for t in range(N - 1):
        s = go.gru(p, go.GRU, seq[t], s, "_l0")
        fwd.append(s)
    s, bwd = torch.zeros(3 * N, H, dtype=torch.float64), [None] * (N - 1)
    for t in range(N - 2, -1, -1):
        s = go.gru(p, go.GRU, seq[t], s, "_l0_reverse")
        bwd[t] = s
    assert float((y.detach() - torch.cat([torch.stack(fwd), torch.stack(bwd)], -1)).abs().max()) <= 1e-12


def test_fresh_noise_is_drawn_when_none_is_given():
    args, agent, I = _agent()
    x, h = torch.randn(args.n_agents, I), torch.zeros(args.n_agents, H)
    assert not torch.equal(agent(x, h)[0], agent(x, h)[0])


def test_state_dict_has_the_published_names_and_shapes():
    args, agent, I = _agent("MMM2")
    sd = agent.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == go.param_shapes(args) and len(sd) == 22
    assert list(sd)[:2] == ["encoding.weight", "encoding.bias"] and sd["encoding.weight"].shape == (64, I)
    assert len(list(agent.parameters())) == 22 and not any(p is b for p in agent.parameters() for b in agent.buffers())
    agent.load_state_dict({k: torch.zeros_like(v) for k, v in sd.items()})          # strict: the dummy fc2 is not in it
    assert float(agent._dummy_w.abs().max()) == 0.0 and agent._dummy_w.shape == (args.n_actions, H)
    args.n_agents = 1
    from marl_amd.network.g2anet import G2ANetAgent
    with pytest.raises(ValueError, match="partner"):
        G2ANetAgent(I, args)


def test_noise_formula_is_finite_at_both_ends():
    l = go.logistic(np.array([0, 1, (1 << 23), (1 << 24) - 1]))
    assert np.isfinite(l).all() and abs(l[0]) <= 17.4 and abs(l[3]) <= 17.4 and l[0] == -l[3] and abs(l[2] - go.logistic(np.array([(1 << 23) - 1]))[0]) < 1e-6
    a, b = go.noise(5, 3, 40, 2, 6, 5), np.stack([go.noise(5, 3, 40 + t, 2, 1, 5)[:, 0] for t in range(6)], 1)
    assert a.shape == (2, 6, 5, 4) and np.array_equal(a, b) and not np.array_equal(a, go.noise(5, 4, 40, 2, 6, 5))


# ---------------------------------------------------------------------------------------------------- launcher
@pytest.fixture
def fake_env(monkeypatch):
    from marl_amd import main
    made = []

    def env(*a, **k):
        made.append(1)
        return type("E", (), {"get_env_info": lambda s: dict(n_actions=11, n_agents=5, state_shape=120, obs_shape=80, episode_limit=120)})()
    monkeypatch.setattr(main, "SyntheticSMACEnv", env)
    monkeypatch.setitem(main.MAPS, "27m", (27, 285, 1170, 36, 180))
    return made


def test_build_applies_the_tables(fake_env):
    from marl_amd import main
    args, _ = main.build(["--alg", "reinforce+g2anet", "--map", "2s3z"])
    assert args.hard is True and args.attention_dim == 32 and args.alg == "reinforce+g2anet" and args.g2anet_tau is None
    assert (args.lr_actor, args.epsilon_anneal_scale) == (1e-4, "episode") and not hasattr(args, "td_lambda") and not hasattr(args, "k")
    args, _ = main.build(["--alg", "central_v+g2anet", "--map", "MMM2", "--g2anet_hard", "False", "--g2anet_tau", "0.5"])
    assert args.hard is False and args.g2anet_tau == 0.5 and args.td_lambda == 0.8
    args, _ = main.build(["--alg", "coma+g2anet", "--map", "3s5z", "--td_lambda", "0.3"])
    assert args.hard is True and args.td_lambda == 0.3
    args, _ = main.build(["--alg", "coma+commnet", "--map", "2s3z"])
    assert args.k == 3 and not hasattr(args, "hard")
    assert main.commnet_base("coma+commnet") == "coma" and main.commnet_base("coma+g2anet") is None and main.commnet_base("coma") is None
    with pytest.raises(ValueError, match="the CommNet actor is trained by central_v, coma or reinforce, not by 'qmix'"):
        main.commnet_base("qmix+commnet")
    assert main.actor_base("reinforce+g2anet") == ("reinforce", "g2anet") and main.actor_base("qmix") == ("qmix", None)


def test_every_suffix_goes_through_its_table_entry(fake_env, monkeypatch):
    """for every suffix of the launcher's table: build() applies that actor's argument table and its command-line override, and
    make_runner hands the Runner that actor's controller class"""
    from marl_amd import main
    from marl_amd.controller import share_params as sp
    want = {"+commnet": ("k", "--commnet_k", "2", 2, sp.CommNetMAC), "+g2anet": ("hard", "--g2anet_hard", "False", False, sp.G2ANetMAC)}
    assert set(main._ACTORS) == set(want)
    handed = []
    monkeypatch.setattr(main, "Runner", lambda env, logger, args, learner_cls=None, mac_cls=None: handed.append(mac_cls))
    for suffix, (name, switch, given, value, cls) in want.items():
        table = getattr(main.build(["--alg", "reinforce" + suffix, "--map", "2s3z"])[0], name)
        args, env = main.build(["--alg", "reinforce" + suffix, "--map", "2s3z", switch, given])
        assert table is not None and getattr(args, name) == value != table
        main.make_runner(args, env, object())
        assert handed[-1] is cls


def test_backward_refuses_the_other_actors_planes():
    from types import SimpleNamespace
    from marl_amd.controller.share_params import CommNetMAC, G2ANetMAC, CommNetPlanes, G2ANetPlanes
    args = go.learner_case("reinforce", "2s3z")[0]
    args.k = 3
    N = args.n_agents
    db = SimpleNamespace(B=1, T=2, N=N, A=args.n_actions, O=args.obs_shape)
    hs = torch.zeros(1, 2, N, H)
    planes = {CommNetMAC: CommNetPlanes(hs, torch.zeros_like(hs)), G2ANetMAC: G2ANetPlanes(hs, torch.zeros(1, 2, N, N - 1))}
    for cls, other in ((CommNetMAC, G2ANetMAC), (G2ANetMAC, CommNetMAC)):
        for bad in (planes[other], hs):
            with pytest.raises(TypeError, match="%s.backward reads the %s " % (cls.__name__, type(planes[cls]).__name__)):
                cls(args).backward(db, None, bad, None, None)


def test_refusals_before_anything_is_built(fake_env, tmp_path):
    from marl_amd import main
    from marl_amd.controller.share_params import G2ANetMAC
    from marl_amd.runner import Runner
    from marl_amd.utils.logging import Logger
    for alg in ("qmix+g2anet", "vdn+g2anet", "+g2anet"):
        with pytest.raises(ValueError, match="the G2ANet actor is trained by central_v, coma or reinforce"):
            main.build(["--alg", alg])
    for sw in ("RTW", "world_model", "MAIC"):
        with pytest.raises(ValueError, match="not with " + sw):
            main.build(["--alg", "coma+g2anet", "--" + sw, "True"])
    with pytest.raises(ValueError, match="marl_g2anet_supported"):
        main.build(["--alg", "reinforce+g2anet", "--map", "27m"])
    with pytest.raises(ValueError, match="g2anet_tau"):
        main.build(["--alg", "reinforce+g2anet", "--g2anet_tau", "0"])
    assert fake_env == []                                               # no environment was made by any of them
    args, env = main.build(["--alg", "reinforce+g2anet", "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "model")])
    args.n_agents = 11
    with pytest.raises(ValueError, match="marl_g2anet_supported"):
        G2ANetMAC(args)
    args.n_agents, args.n_actions = 5, 33
    with pytest.raises(ValueError, match="marl_g2anet_supported"):
        G2ANetMAC(args)
    args.n_actions = 11
    with pytest.raises(ValueError, match="cannot find!"):                # the runner's own tables do not hold the name
        Runner(env, Logger(), args)
    args.RTW = True
    with pytest.raises(ValueError, match="not with RTW"):
        main.make_runner(args, env, Logger())


def test_supported_range():
    from marl_amd import ops
    assert all(ops.g2anet_supported(N, A, hard) for N in range(2, 11) for A in (1, 32) for hard in (True, False))
    assert not ops.g2anet_supported(1, 5) and not ops.g2anet_supported(11, 5) and not ops.g2anet_supported(5, 33) and not ops.g2anet_supported(5, 0)
    assert [ops.g2anet_groups_per_workgroup(N) for N in (1, 2, 3, 5, 8, 10, 11)] == [0, 8, 5, 3, 2, 1, 0]


def test_multi_rank_is_refused(monkeypatch):
    from marl_amd.algorithm import reinforce, policy_learner
    from marl_amd.controller.share_params import G2ANetMAC
    args, _, _ = go.learner_case("reinforce", "2s3z")
    mac = G2ANetMAC(args)
    monkeypatch.setattr(policy_learner, "GradReducer", type("R", (), {"enabled": True}))
    with pytest.raises(NotImplementedError):
        reinforce.ReinforceLearner(mac, args)
    assert not hasattr(mac.agent, "_flat")


# ---------------------------------------------------------------------------------------------------- the head cases
@functools.lru_cache(maxsize=None)
def _refs(G, N, A, hard, tau):
    c = go.head_case(G, N, A, go.head_seed(G, N, A))
    return go.head_reference(c, N, hard, tau), go.head_reference(c, N, hard, tau, dtype=torch.float32)


EXTRA = tuple((2 * (16 // N) + 1, N, A) for N, A in go.EXTRA_NA)


@pytest.mark.parametrize("G,N,A", list(go.HEAD_SHAPES) + list(go.MANY_TILES) + list(EXTRA))
def test_head_cases_exercise_what_the_gpu_file_relies_on(G, N, A):
    """on the float64 reference: at tau = 0.01 at least 1 % of the pairs (and at least two) have w inside (1e-3, 1 - 1e-3) - otherwise
    the hard gradient is not exercised; every gradient has max|ref| >= 0.02, but for the tensors that are exactly zero at N = 2;
    hard off: the ten hard tensors get exactly zero"""
    for hard, tau in go.HEAD_MODES:
        ref, _ = _refs(G, N, A, hard, tau)
        if hard and tau == 0.01:
            w = ref["w"]
            mid = int(((w > 1e-3) & (w < 1.0 - 1e-3)).sum())
            print("G=%d N=%d A=%d: %d of %d pairs inside (%.3f)" % (G, N, A, mid, w.size, mid / w.size))
            assert mid >= 2 and mid >= 0.01 * w.size
        for k in go.HEAD_PARAMS:
            top = float(np.abs(ref[k]).max())
            if (not hard and k in go.HARD_PARAMS) or (N == 2 and k in go.ZERO_AT_N2):
                assert top == 0.0, (k, top)
            else:
                assert top >= 0.02, (hard, tau, k, top)


def _derive(prefix, ref, f32, skip=lambda k: False):
    derived = {}
    for k, r in ref.items():
        r = np.asarray(r, dtype=np.float64)
        err = float(np.abs(np.asarray(f32[k], dtype=np.float64) - r).max())
        scale = float(np.abs(r).max())
        print("%-44s %-44s f32 err %.3e  max|ref| %.3e  share of 1e-4 max|ref| %.3f" % (prefix, k, err, scale, err / (1e-4 * scale + 1e-30)))
        if err > 0.25 * 1e-4 * scale + 1e-7 and not skip(k):
            derived[prefix + (k,)] = err
    listed = {k: v for k, v in go.F32_EXCEPTIONS.items() if k[:len(prefix)] == prefix and len(k) == len(prefix) + 1}
    assert set(derived) == set(listed), (derived, listed)
    for k, err in derived.items():
        assert err <= 1.5 * listed[k], (k, err, listed[k])


@pytest.mark.parametrize("G,N,A,hard,tau", [s + m for s in list(go.HEAD_SHAPES) + list(go.MANY_TILES) + list(EXTRA) for m in go.HEAD_MODES])
def test_float32_oracle_of_the_head_cases(G, N, A, hard, tau):
    """The head oracle in float32 against float64 on every head case of the GPU file: a quarter of 1e-4 * max|ref| (+ parity's floor)
    per tensor; a tensor that does not stay under is in g2anet_oracle.F32_EXCEPTIONS with its float32-oracle error, derived here and
    never from GPU output (the 1 / tau factor multiplies float32 rounding by 100 at tau = 0.01)"""
    ref, f32 = _refs(G, N, A, hard, tau)
    drop = lambda d: {k: v for k, v in d.items() if k != "w"}
    _derive(("head", G, N, A, hard, tau), drop(ref), drop(f32))


@pytest.mark.parametrize("name,flags", go.MAC_CASES)
def test_float32_oracle_of_the_controller_cases(name, flags):
    """the controller cases of the GPU file (logits and hs under m, the 22 gradients) in float32 against float64, as the head cases"""
    ref, f32 = (_mac_ref(name, flags, dt)[4] for dt in (torch.float64, torch.float32))
    assert len(ref) == 24
    _derive(("mac", name, flags), ref, f32)


def _mac_ref(name, flags, dtype):
    args = go.learner_case("reinforce", name, dtype, last_action=flags, reuse_network=flags)[0]
    return go.mac_reference(name, flags, lambda B, T, N: go.update_noise(args, 0, B, T, N), dtype)


# ---------------------------------------------------------------------------------------------------- float32 yardstick of the learners
def two_updates(run, dtype, g2anet=True):
    """every tensor the GPU learner file compares, of two updates of a run; ``g2anet`` False: the plain oracle of the same case"""
    alg, name = run[0], run[1]
    beta = run[2] if alg == "reinforce" else (run[3] if alg == "coma" else 0.0)
    lam = None if alg == "reinforce" else run[2]
    over = dict(policy_entropy_coef=beta)
    if lam is not None:
        over["td_lambda"] = lam
    if g2anet:
        args, state, batch = go.learner_case(alg, name, dtype, **over)
    else:
        args, state, batch = {"reinforce": pg, "central_v": po, "coma": co}[alg].learner_case(name, dtype, **over)
    out = {}
    with go.g2anet_actor(lambda step, B, T, N: go.update_noise(args, step, B, T, N)) as actor:
        for i in range(2):
            actor.step = i
            s = "step%d/" % i
            if alg == "reinforce":
                loss, grads, inter = pg.train(state, batch(i), i, go.EPS, beta)
                out[s + "l_actor"] = loss
            elif alg == "central_v":
                lc, la, grads, inter = po.train(state, batch(i), i, go.EPS, lam)
                out[s + "l_critic"], out[s + "l_actor"], out[s + "v"] = lc, la, inter["v"].detach().numpy()
            else:
                lc, la, grads, inter = co.train(state, batch(i), i, go.EPS, lam, beta)
                out[s + "l_critic"], out[s + "l_actor"] = lc, la
                for k in ("q", "q_taken", "q_next"):
                    out[s + k] = inter[k].detach().numpy()
                out[s + "adv"] = inter["adv"].detach().numpy() * inter["mask"].numpy()[:, :, None]
            if g2anet and dtype == torch.float64:
                assert po.relu_near_zero(inter) == 0          # encoding's ReLU: no pre-activation that carries a gradient near its kink
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


@pytest.mark.parametrize("run", go.RUNS, ids=lambda r: "-".join(str(x) for x in r))
def test_float32_oracle_stays_under_a_quarter_of_the_bound(run):
    """The oracle in float32 against float64 on every run of the GPU learner file (both fed the update noise of the numpy
    restatement): a quarter of 1e-4 * max|ref| (+ parity's floor) on every compared tensor of both updates, under m where a tensor is
    masked.  The critic's tensors equal the plain oracle's bit for bit in float64, so their float32 exceptions are the existing
    tables'; every other tensor that does not stay under is in g2anet_oracle.F32_EXCEPTIONS with its float32-oracle error."""
    alg = run[0]
    ref, f32 = two_updates(run, torch.float64), two_updates(run, torch.float32)
    if alg != "reinforce":
        plain = two_updates(run, torch.float64, g2anet=False)
        for k, r in ref.items():
            if _critic_key(k):
                assert np.array_equal(np.asarray(r), np.asarray(plain[k])), k
    _derive(run, ref, f32, skip=lambda k: alg != "reinforce" and _critic_key(k))
