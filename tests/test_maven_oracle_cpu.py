"""MAVEN on the CPU: the float64 oracle (tests/maven_oracle.py) against autograd of the literal hyper-layer formulation, the host wiring
(refusals, argument overrides, the record and the replay ring carrying the noise, records without noise untouched) and the conditioning
of every learner case the GPU test compares.  Runs with ``-m "not gpu"``."""
import types

import numpy as np
import pytest
import torch

from oracle import rollout as orollout, seeded
import maven_oracle as mo

t64 = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ the oracle itself
def test_noise_draw_is_the_counter_hash():
    for seed, env0, tg0, K, E in [(123, 0, 0, 16, 7), (0xFFFFFFFF, 5, 121 * 7, 3, 33), (1, 1 << 20, 2 ** 31 + 5, 32, 9), (9, 0, 4, 1, 4)]:
        got = mo.noise_draw(seed, env0, tg0, K, E)
        ref = orollout.key(seed, mo.ST_MAVEN, env0 + np.arange(E), tg0, 0) % np.uint32(K)
        assert got.dtype == np.int32 and np.array_equal(got, ref.astype(np.int32)) and (got >= 0).all() and (got < K).all()
    draws = mo.noise_draw(123, 0, 0, 16, 4096)
    assert set(draws.tolist()) == set(range(16))                      # uniform enough for every value to occur
    assert not np.array_equal(draws[:64], mo.noise_draw(123, 0, 121, 16, 64))


@pytest.mark.parametrize("B, T, N, A, K", [(1, 1, 1, 1, 1), (3, 4, 5, 11, 16), (2, 3, 16, 32, 32)])
def test_head_is_the_hyper_layer_on_one_hot_inputs(B, T, N, A, K):
    """value and every gradient of q' = fc2(h) + head_term against the literal Linear(K + N -> A H) / Linear(K + N -> A) formulation"""
    g = np.random.default_rng(B + T + N + A + K)
    Wl, bl = t64(g.standard_normal((A * mo.H, K + N))).requires_grad_(True), t64(g.standard_normal((A, K + N))).requires_grad_(True)
    fw, fb = t64(g.standard_normal((A, mo.H))).requires_grad_(True), t64(g.standard_normal(A)).requires_grad_(True)
    hs = t64(g.standard_normal((B, T, N, mo.H))).requires_grad_(True)
    noise = g.integers(0, K, size=B)
    cot = t64(g.standard_normal((B, T, N, A)))
    lit = mo.hyper_layer_q(Wl, bl, fw, fb, hs, noise, K)
    glit = torch.autograd.grad((lit * cot).sum(), [Wl, bl, fw, fb, hs])
    tab = {k: v.detach().clone().requires_grad_(True) for k, v in mo.tables_of_hyper_layer(Wl, bl, K, N, A).items()}
    fw2, fb2, hs2 = (x.detach().clone().requires_grad_(True) for x in (fw, fb, hs))
    mine = hs2 @ fw2.T + fb2 + mo.head_term(tab, hs2, noise)
    assert torch.allclose(mine, lit, rtol=1e-12, atol=1e-12)
    gm = torch.autograd.grad((mine * cot).sum(), [tab[k] for k in mo.TABLES] + [fw2, fb2, hs2])
    gtab = mo.tables_of_hyper_layer(glit[0], glit[1], K, N, A)          # the layers' gradients, cut into the same columns
    for k, x in zip(mo.TABLES, gm[:4]):
        assert torch.allclose(x, gtab[k], rtol=1e-11, atol=1e-11), k
    for x, y in zip(gm[4:], glit[2:]):
        assert torch.allclose(x, y, rtol=1e-11, atol=1e-11)
    # no parameter is redundant: every table entry that a drawn index reaches has a gradient of its own
    assert float(gm[1].abs().min()) > 0 and all(float(gm[0][k].abs().min()) > 0 for k in set(noise.tolist()))


def test_head_skips_an_episode_with_noise_out_of_range():
    c = mo.head_case(3, 17, 5, 11, 16)
    assert c.skipped[-1] and not (0 <= c.noise[-1] < 16) and np.isnan(c.hs[-1]).all() and (c.noise[1:-1] != c.noise[0]).all()
    o = mo.head_oracle(c)
    assert np.array_equal(o.q_out[-1], c.q[-1].astype(np.float64)) and not np.array_equal(o.q_out[0], c.q[0].astype(np.float64))
    assert (o.dhs[-1] == 0).all() and np.isfinite(o.dhs).all()
    used = sorted(set(c.noise[~c.skipped].tolist()))
    assert all((o.grads["noise_w"][k] == 0).all() for k in range(16) if k not in used)
    assert all(np.abs(o.grads["noise_w"][k]).max() > 0 for k in used)


def test_mi_rows_properties_and_a_finite_difference():
    c = mo.mi_case(3, 17, 5, 11, 120, 16)
    for lam in (0.001, 1.0):
        o = mo.mi_oracle(c, lam)
        dead = c.padded == 1
        assert dead[-1].all() and dead.any(axis=1)[1:].all() and not dead[0].any()
        assert (o.dq_dense[dead] == 0).all() and (o.ce[dead] == 0).all() and np.isfinite(o.dq_dense).all()
        live_unavail = (np.nan_to_num(c.avail) == 0) & ~dead[..., None, None]
        assert (o.dq_dense[live_unavail] == 0).all() and (o.p[live_unavail] == 0).all()
        assert o.p[0, 0, 0, -1] == 1.0 and (o.dq_dense[0, 0, 0] == 0).all()             # one available action: p = 1, no gradient
        assert np.allclose(o.p.sum(axis=3)[~dead], 1.0)
    # d (sum m ce) / d q at one live, available entry, by central differences
    b, t, n = 0, 3, 2
    a = int(np.nonzero(c.avail[b, t, n])[0][-1])
    f = lambda d: mo.mi_oracle(types.SimpleNamespace(**{**vars(c), "q": _bump(c.q, (b, t, n, a), d)}), 1.0).stats[0]
    fd = (f(1e-3) - f(-1e-3)) / 2e-3
    ref = mo.mi_oracle(c, 1.0).dq_dense[b, t, n, a]
    assert abs(fd - ref) <= 1e-3 * max(abs(ref), 1e-3), (fd, ref)        # (q is float32: the step is what limits the agreement)


def _bump(q, at, d):
    q = q.astype(np.float64).copy()
    q[at] += d
    return q


# ------------------------------------------------------------------------------------------------ host wiring
def test_argument_table_and_overrides():
    from marl_amd.common.arguments import get_common_args, get_mixer_args, get_maven_args
    a = get_mixer_args(get_common_args(["--alg", "maven"]))
    assert (a.noise_dim, a.lambda_mi) == (16, 0.001)                    # the table's, as before this algorithm existed
    get_maven_args(a)
    assert (a.noise_dim, a.lambda_mi, a.maven_discrim_dim) == (16, 0.001, 64)
    p = get_common_args(["--alg", "maven", "--noise_dim", "5", "--lambda_mi", "0.5"])
    assert (p.noise_dim, p.lambda_mi) == (5, 0.5) and get_common_args([]).noise_dim is None and get_common_args([]).lambda_mi is None
    for bad in (dict(noise_dim=0), dict(noise_dim=33), dict(noise_dim=True), dict(noise_dim=2.0), dict(lambda_mi=-1e-9), dict(lambda_mi=float("nan"))):
        with pytest.raises(ValueError):
            get_maven_args(types.SimpleNamespace(**{**dict(noise_dim=None, lambda_mi=None), **bad}))


class _StubEnv:
    def __init__(self, n_envs, n, o, s, a, t, seed=1):
        self.n_envs, self.info = n_envs, {"n_actions": a, "n_agents": n, "state_shape": s, "obs_shape": o, "episode_limit": t}

    def get_env_info(self):
        return self.info


def test_launcher_overrides_and_refusals(monkeypatch):
    from marl_amd import main
    made = []
    monkeypatch.setattr(main, "SyntheticSMACEnv", lambda *a, **k: made.append(1) or _StubEnv(*a, **k))
    args, _ = main.build(["--alg", "maven", "--map", "2s3z", "--n_envs", "8"])
    assert (args.noise_dim, args.lambda_mi, args.maven_discrim_dim, args.alg) == (16, 0.001, 64, "maven") and made == [1]
    args, _ = main.build(["--alg", "maven", "--map", "MMM2", "--n_envs", "8", "--noise_dim", "3", "--lambda_mi", "0"])
    assert (args.noise_dim, args.lambda_mi) == (3, 0.0)
    args, _ = main.build(["--alg", "qmix", "--map", "2s3z", "--n_envs", "8", "--noise_dim", "3", "--lambda_mi", "0.5"])
    assert (args.noise_dim, args.lambda_mi) == (16, 0.001)              # every other algorithm: the table's, as before
    made.clear()
    for argv in (["--noise_dim", "0"], ["--noise_dim", "33"], ["--lambda_mi", "-0.5"], ["--RTW", "True"], ["--world_model", "True"],
                 ["--MAIC", "True"]):
        with pytest.raises(ValueError):
            main.build(["--alg", "maven", "--map", "2s3z", "--n_envs", "8"] + argv)
    monkeypatch.setitem(main.MAPS, "wide", (16, 80, 2000, 32, 10))      # N A + S beyond a tile of x
    with pytest.raises(ValueError, match="marl_maven_supported"):
        main.build(["--alg", "maven", "--map", "wide", "--n_envs", "8"])
    assert made == []                                                    # each refused before the environment is made


def test_supported_range():
    from marl_amd import ops
    assert ops.maven_supported(5, 11, 16, 120) and ops.maven_supported(10, 18, 16, 322) and ops.maven_supported(16, 32, 32, 40)
    assert ops.maven_supported(1, 1, 1, 1) and ops.maven_supported(16, 32, 32, 320)
    for bad in ((0, 11, 16, 120), (17, 11, 16, 120), (5, 0, 16, 120), (5, 33, 16, 120), (5, 11, 0, 120), (5, 11, 33, 120), (5, 11, 16, 0),
                (16, 32, 32, 337), (16, 32, 32, 2000)):
        assert not ops.maven_supported(*bad), bad
    assert not ops.maven_supported(5, 11, 16, 120, 32)
    plan = ops.maven_plan(3, 17, 5, 11, 16, 120)
    assert plan[0] == 2 and plan[1] == 3 * 5 * 2 and plan[2] == 3 and plan[3] == 4 and plan[4] == 4 and plan[6] == 1 and plan[5] <= 96 * 1024
    assert ops.maven_plan(4096, 120, 10, 18, 16, 322)[4] == 256 and ops.maven_plan(0, 5, 5, 11, 16, 120) == (0,) * 8


def test_runner_and_learner_refusals(monkeypatch):
    from marl_amd.runner import Runner
    from marl_amd.controller.share_params import MAVENMAC, SharedMAC
    from marl_amd.algorithm import maven as alg
    args, *_ = mo.learner_case("2s3z")
    for over, exc in ((dict(RTW=True), ValueError), (dict(world_model=True), ValueError), (dict(MAIC=True), ValueError),
                      (dict(overlap_rollout=True), NotImplementedError)):
        with pytest.raises(exc, match="maven|MAVEN"):
            Runner(None, None, types.SimpleNamespace(**{**vars(args), **over}))
    with pytest.raises(TypeError, match="MAVENMAC"):
        alg.MAVENLearner(SharedMAC(args), args)
    mac = MAVENMAC(args)
    assert mac.head_name == "MAVEN" and mac.noise_dim == 16 and [k for k, _ in mac.agent.named_parameters()] == [k for k, _ in mo.agent_shapes(args)]
    assert [tuple(p.shape) for p in mac.agent.parameters()] == [s for _, s in mo.agent_shapes(args)]
    bound = 1.0 / np.sqrt(16 + args.n_agents)                            # nn.Linear(K + N, .)'s range for its columns
    for k in mo.TABLES:
        t = getattr(mac.agent.maven, k).detach()
        assert 0.9 * bound < float(t.abs().max()) <= bound and (t.numel() < 1000 or abs(float(t.mean())) < 0.05 * bound), k
    with pytest.raises(NotImplementedError):
        mac.choose_action(np.zeros(args.obs_shape), np.zeros(args.n_actions), 0, np.ones(args.n_actions), 0.0)
    with pytest.raises(NotImplementedError):
        mac._step_head(None, None, None, None, False)
    monkeypatch.setattr(alg, "GradReducer", lambda: types.SimpleNamespace(enabled=True))
    with pytest.raises(NotImplementedError, match="one rank"):
        alg.MAVENLearner(mac, args)
    for bad in (dict(noise_dim=0), dict(noise_dim=33), dict(lambda_mi=-1.0), dict(maven_discrim_dim=32)):
        with pytest.raises(ValueError):
            MAVENMAC(types.SimpleNamespace(**{**vars(args), **bad}))


def _record(E, noise=None, T=4, N=2, O=3, S=5, A=3, seed=0):
    from marl_amd.env.synthetic_smac import EpisodeRecord
    g = torch.Generator().manual_seed(seed)
    rec = EpisodeRecord(E, T, N, O, S, A, "cpu")
    for f in ("obs", "state_store", "avail", "r"):
        getattr(rec, f).copy_(torch.rand(getattr(rec, f).shape, generator=g))
    rec.length.fill_(T)
    if noise is not None:
        rec.noise = torch.tensor(noise, dtype=torch.int32)
    return rec


def test_record_carries_noise_and_records_without_it_are_untouched():
    from marl_amd.env.synthetic_smac import EpisodeRecord
    assert EpisodeRecord.FIELDS == ("obs", "state_store", "avail", "u", "r", "term", "padded", "length", "won")
    plain = _record(4)
    idx = torch.tensor([2, 0, 2])
    for other in (plain.slice(1, 3), plain.clone(), plain.index_select(idx), plain.select_small(idx)):
        assert other.noise is None and "noise" not in vars(other)
    assert "noise" not in vars(plain)
    rec = _record(4, noise=[5, 6, 7, 8])
    assert rec.slice(1, 3).noise.tolist() == [6, 7] and rec.slice(1, 3).noise.data_ptr() == rec.noise[1:].data_ptr()
    c = rec.clone()
    assert c.noise.tolist() == [5, 6, 7, 8] and c.noise.data_ptr() != rec.noise.data_ptr()
    assert rec.index_select(idx).noise.tolist() == [7, 5, 7]
    small = rec.select_small(idx)
    assert small.noise.tolist() == [7, 5, 7] and small.noise.dtype == torch.int32
    kept = small.noise
    rec.select_small(torch.tensor([1, 1, 3]), out=small)
    assert small.noise is kept and kept.tolist() == [6, 6, 8]              # gathered into the same array (persistent buffers)
    dst = _record(6)
    rec.copy_into(dst, torch.tensor([4, 5, 0, 1]))
    assert dst.noise.tolist() == [7, 8, 0, 0, 5, 6] and dst.noise.shape == (6,)
    plain.copy_into(dst, torch.tensor([0, 1, 2, 3]))
    assert dst.noise.tolist() == [7, 8, 0, 0, 5, 6]                        # a record without noise leaves the ring's alone


def test_replay_ring_and_batch_carry_noise():
    from marl_amd.common.replaybuffer import ReplayBuffer
    from marl_amd.rollout import EpisodeBatch
    from marl_amd.hostutil import DeviceBatch
    args = types.SimpleNamespace(n_actions=3, n_agents=2, state_shape=5, obs_shape=3, buffer_size=6, episode_limit=4)
    buf = ReplayBuffer(args)
    buf.store_episode(EpisodeBatch(_record(2)))
    assert buf.record.noise is None and "noise" not in vars(buf.record)      # no noise stored: the ring allocates as before
    buf.store_episode(EpisodeBatch(_record(3, noise=[4, 5, 6], seed=1)))
    assert buf.record.noise.shape == (6,) and buf.record.noise.tolist() == [0, 0, 4, 5, 6, 0]
    buf.store_episode(EpisodeBatch(_record(2, noise=[7, 8], seed=2)))         # wraps around
    assert buf.record.noise.tolist() == [8, 0, 4, 5, 6, 7]
    np.random.seed(0)
    sample = buf.sample(4)
    idx = sample.index
    assert sample.record.noise.tolist() == buf.record.noise[idx].tolist()
    db = DeviceBatch.from_record(buf.record, args, index=idx)
    assert db.noise.tolist() == buf.record.noise[idx].tolist() and db.noise.dtype == torch.int32
    assert db.avail_store[0] is buf.record.avail and db.avail_store[1] == 5 * 2 * 3 and db.o_map.tolist() == idx.tolist()
    assert DeviceBatch.from_record(_record(2), args).noise is None
    # the 11-key dict: noise beside it, or none
    sargs = seeded.make_args("matrix", "maven", episode_limit=1)
    batch = seeded.make_batch(sargs, 3, seed=1, lengths=[1, 1, 1])
    assert DeviceBatch.from_dict(batch, sargs, "cpu").noise is None
    batch["noise"] = np.array([2, 0, 1])
    db = DeviceBatch.from_dict(batch, sargs, "cpu")
    assert db.noise.tolist() == [2, 0, 1] and db.noise.dtype == torch.int32 and db.avail_store is None


# ------------------------------------------------------------------------------------------------ the learner cases
_COND = {}


def cond(name):
    if name not in _COND:
        _COND[name] = mo.conditioning(name)
    return _COND[name]


@pytest.mark.parametrize("name", list(mo.LEARNER_CASES))
def test_learner_case_is_well_conditioned(name):
    for i, c in enumerate(cond(name)):
        print(name, "update", i, "margins", c.margins, "relu %.3e" % c.relu)
        assert all(v >= 1.0 for v in c.margins.values()), (name, i, c.margins)
        assert c.relu >= mo.RELU_EPS, (name, i, c.relu)
        assert c.all_noise and c.same, (name, i)


@pytest.mark.parametrize("name", list(mo.LEARNER_CASES))
def test_float32_oracle_stays_under_a_quarter_of_the_bound_or_is_listed(name):
    for i, c in enumerate(cond(name)):
        for key, frac in c.frac.items():
            exc = mo.F32_EXCEPTIONS.get((name, i, key))
            if exc is None:
                assert frac <= 0.25, "%s update %d %s: the float32 oracle is at %.2f of the bound (err %.3e): list it" % (name, i, key, frac, c.err[key])
            else:
                assert not key.startswith("grad ") and c.err[key] <= 1.5 * exc, (name, i, key, c.err[key], exc)
    assert all(k[0] in mo.LEARNER_CASES for k in mo.F32_EXCEPTIONS)


def test_learner_cases_cover_what_the_issue_asks():
    cases = mo.LEARNER_CASES.values()
    assert {c[0] for c in cases} == {"2s3z", "MMM2", "matrix"} and all(4 <= c[1] <= 6 for c in cases)
    assert {c[5] for c in cases} == {0.001, 0.0} and {c[6] for c in cases} == {None, 0.8}
    args, st, batch, noise, lam = mo.learner_case("matrix_mi0")
    assert set(noise(0).tolist()) == {0, 1, 2}
    # with lambda_mi = 0 the discriminator gets a zero gradient and does not move
    before = {k: x.detach().clone() for k, x in st.discrim.items()}
    _, grads, _ = mo.train(st, batch(0), noise(0), 0, lam=lam)
    assert all(float(grads["discrim." + k].abs().max()) == 0 and torch.equal(before[k], st.discrim[k].detach()) for k in before)
