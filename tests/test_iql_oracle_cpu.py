"""Independent Q-learning on the CPU: properties of tests/iql_oracle.py (the float64 restatement the GPU tests hold csrc/iql.hip and
IQLLearner to), its agreement with the existing VDN oracle where the two coincide (one agent), the C ABI's declaration and the
runner / launcher wiring of ``--alg iql``."""
import types

import numpy as np
import pytest
import torch

from oracle import seeded, learners
import iql_oracle as io

CASES = [(1, 1, 1, 1), (3, 5, 3, 11), (5, 13, 10, 16), (3, 5, 1, 22), io.BIG + (17,)]


def _rows(c, double_q=True, avail=True, ret=None):
    return io.rows(c.q, c.u, c.q_sel if double_q else None, c.q_tgt, c.avail if avail else None, c.r, c.term, c.padded, io.GAMMA,
                   c.N, ret=ret)


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("B,T,N,A", CASES)
def test_closed_form_gradient_equals_autograd(B, T, N, A):
    c = io.kernel_case(B, T, N, A, seed=A)
    for kw in (dict(), dict(double_q=False), dict(avail=False), dict(ret=torch.tensor(c.ret).permute(0, 2, 1).reshape(-1))):
        o = _rows(c, **kw)
        dense = torch.zeros(c.R, A, dtype=torch.float64)
        dense[torch.arange(c.R), torch.tensor(c.u.astype(np.int64))] = o.dq_val
        assert torch.equal(dense, o.dq), kw                        # - 2 m td at the taken action, exact zeros elsewhere
        assert float(o.den) == float(c.N * (1 - c.padded).sum())
        dead = torch.tensor(c.dead)
        for x in (o.q_taken, o.q_next, o.dq_val, o.td):
            assert torch.isfinite(x).all() and bool((x[dead] == 0).all())
        assert torch.isfinite(o.num)


def test_case_has_the_edges_it_is_named_for():
    c = io.kernel_case(5, 13, 10, 16)
    live = ~c.dead
    k0, k1, k2, k3 = c.kinds
    assert (live & k0).any() and (live & k1).any() and (live & k2).any() and (live & k3).any() and c.dead.any()
    assert (c.avail[live & k2].sum(axis=1) == 0).all() and (c.avail[live & k3].sum(axis=1) == 1).all()
    assert np.isnan(c.q[c.dead]).all() and np.isnan(c.q_sel[c.dead]).all() and np.isnan(c.q_tgt[c.dead]).all() and np.isnan(c.avail[c.dead]).all()
    term, padded = c.term.reshape(c.B, c.T), c.padded.reshape(c.B, c.T)
    assert ((term == 1) & (padded == 0)).any() and padded[1].sum() == 0 and term[1].sum() == 0      # an unterminated episode
    assert io.BIG[0] * io.BIG[1] * io.BIG[2] == 64 * 6 + 1


def test_first_index_wins_ties_and_nothing_available_is_the_mask():
    c = io.kernel_case(5, 13, 10, 16)
    live = ~c.dead
    k0, k1, k2, _ = c.kinds
    clean = lambda x: np.where(c.dead[:, None], 0, x)
    q_next, arg = io.select(clean(c.q_sel), clean(c.q_tgt), clean(c.avail))
    assert (arg.numpy()[live & k0 & ~k1] == 0).all()               # the maximum sits at column 0 and at the last one
    assert (arg.numpy()[live & k1] == c.A - 2).all()
    assert (q_next.numpy()[live & k2] == io.MASK_BIG).all()
    # without double-Q the selection is the masked maximum of q_tgt
    q_max, _ = io.select(None, clean(c.q_tgt), clean(c.avail))
    want = np.where(clean(c.avail) == 0, io.MASK_BIG, clean(c.q_tgt).astype(np.float64)).max(axis=1)
    assert (q_max.numpy() == want).all()


@pytest.mark.parametrize("A", [a for a in io.A_SIZES + io.A_TWO_OPERANDS + io.A_ONE_OPERAND if a > 1])
@pytest.mark.parametrize("avail", [True, False])
def test_the_tie_rows_tell_the_tie_orders_apart(A, avail):
    """q_next is all the GPU tests see of a*: on every live tie row the first index gives TIE_FIRST, and a last-index argmax (``>=``
    for ``>``) would give TIE_LAST"""
    B, T, N = io.BIG
    c = io.kernel_case(B, T, N, A, seed=A)
    k0, k1, _, _ = c.kinds
    ties = ~c.dead & (k0 | k1)
    assert ties.sum() >= 32
    clean = lambda x: np.where(c.dead[:, None], 0, x)
    av = clean(c.avail) if avail else None
    q_next, arg = io.select(clean(c.q_sel), clean(c.q_tgt), av)
    assert (q_next.numpy()[ties] == io.TIE_FIRST).all()
    sel = clean(c.q_sel).astype(np.float64) if av is None else np.where(av == 0, io.MASK_BIG, clean(c.q_sel).astype(np.float64))
    last = A - 1 - np.argmax(sel[:, ::-1], axis=1)
    assert (last[ties] != arg.numpy()[ties]).all()
    assert (clean(c.q_tgt)[np.arange(c.R), last][ties] == io.TIE_LAST).all()


@pytest.mark.parametrize("B,T,N,A", CASES)
def test_lambda_zero_returns_the_one_step_targets(B, T, N, A):
    c = io.kernel_case(B, T, N, A, seed=3)
    o = _rows(c)
    # (a live row with nothing available carries the mask constant: the sizes differ by 1e7, the comparison is relative)
    G, G_bnt = io.lambda_returns(o.q_next, c.r, c.term, c.padded, io.GAMMA, 0.0, B, T, N)
    live = o.live
    assert torch.allclose(G[live], o.y[live], rtol=1e-14, atol=1e-12)
    assert torch.equal(G_bnt.permute(0, 2, 1).reshape(-1), G)
    G8, _ = io.lambda_returns(o.q_next, c.r, c.term, c.padded, io.GAMMA, 0.8, B, T, N)
    if T > 1 and B > 1:
        assert not torch.allclose(G8[live], o.y[live])
    # the returns as the target: the same loss as the one-step call
    o2 = _rows(c, ret=G)
    assert torch.allclose(o2.num, o.num, rtol=1e-12) and torch.allclose(o2.dq_val, o.dq_val, rtol=1e-12, atol=1e-9)


def test_a_padded_row_holding_nan_changes_nothing():
    c = io.kernel_case(5, 13, 3, 11)
    o = _rows(c)
    g = np.random.default_rng(0)
    for x in (c.q, c.q_sel, c.q_tgt, c.avail):
        x[c.dead] = g.standard_normal((int(c.dead.sum()), c.A)).astype(np.float32)
    o2 = _rows(c)
    for k in ("q_taken", "q_next", "y", "td", "num", "den", "dq", "dq_val"):
        assert torch.equal(getattr(o, k), getattr(o2, k)), k


# ------------------------------------------------------------------------------------------------ one agent: VDN's sum is the agent
@pytest.mark.parametrize("double_q", [True, False])
def test_one_agent_equals_the_vdn_oracle(double_q):
    args = seeded.make_args("2s3z", "vdn", episode_limit=6, n_agents=1, double_q=double_q)
    agent = seeded.seeded_state(seeded.agent_param_shapes(args), seed=11)
    batch = seeded.make_batch(args, 4, seed=100, lengths=[5, 3, -1, 4])
    vdn = learners.LearnerState(args, agent, {})
    iql = io.State(args, agent, dtype=torch.float32)
    for s in (vdn, iql):                                              # a target net that differs from the eval net
        s.target_agent = {k: x + 0.01 * torch.sin(torch.arange(x.numel(), dtype=x.dtype)).reshape(x.shape) for k, x in s.target_agent.items()}
    lv, iv = learners.q_forward(vdn, learners.clone_batch(batch))
    li, ii = io.forward(iql, learners.clone_batch(batch))
    assert iv["T"] == ii["T"]
    np.testing.assert_allclose(float(li.detach()), float(lv.detach()), rtol=2e-6)
    assert float(ii["den"]) == float(iv["den"])
    dv, = torch.autograd.grad(lv, iv["q_evals"])
    di, = torch.autograd.grad(li, ii["q_evals"])
    scale = float(dv.abs().max())
    assert scale > 0 and float((dv - di).abs().max()) <= 2e-6 * scale
    np.testing.assert_allclose(ii["q_next"].numpy().reshape(-1), iv["q_targets_chosen"].numpy().reshape(-1) * (1 - np.asarray(batch["padded"])[:, :ii["T"]].reshape(-1)),
                               rtol=1e-6, atol=1e-6)


def test_three_agents_are_not_vdn():
    """with more than one agent the two losses are different functions (the square of a sum is not the sum of squares)"""
    args = seeded.make_args("2s3z", "vdn", episode_limit=6, n_agents=3)
    agent = seeded.seeded_state(seeded.agent_param_shapes(args), seed=11)
    batch = seeded.make_batch(args, 4, seed=100, lengths=[5, 3, -1, 4])
    lv, _ = learners.q_forward(learners.LearnerState(args, agent, {}), learners.clone_batch(batch))
    li, ii = io.forward(io.State(args, agent), learners.clone_batch(batch))
    li, lv = float(li.detach()), float(lv.detach())
    assert abs(li - lv) > 1e-3 * abs(lv)
    assert float(ii["den"]) == 3 * (1 - np.asarray(batch["padded"])[:, :ii["T"]]).sum()


def test_train_steps_and_syncs_the_target():
    args = seeded.make_args("2s3z", "iql", episode_limit=5, target_update_cycle=2)
    st = io.State(args, seeded.seeded_state(seeded.agent_param_shapes(args), seed=11))
    before = {k: x.detach().clone() for k, x in st.agent.items()}
    for i in range(3):
        loss, grads, inter = io.train(st, seeded.make_batch(args, 3, seed=100 + i, lengths=[5, 2, 4]), i, lam=0.8 if i == 1 else None)
        assert np.isfinite(loss) and all(g is not None for g in grads.values())
        synced = all(torch.equal(st.target_agent[k], st.agent[k].detach()) for k in st.agent)
        assert synced == (i == 2)
    assert all(not torch.equal(before[k], st.agent[k].detach()) for k in before)


@pytest.mark.parametrize("name", list(io.LEARNER_CASES))
def test_learner_cases_are_well_conditioned(name):
    """what the seeds of iql_oracle.LEARNER_CASES were chosen for: the float32 oracle stays under a quarter of the GPU test's bound"""
    assert io.float32_fraction(name) <= 0.25
    args, st, batch, lam = io.learner_case(name)
    b = batch(0)
    assert learners.max_episode_len(b["terminated"], args.episode_limit) == io.LEARNER_T
    assert np.asarray(b["terminated"])[0, io.LEARNER_T - 1, 0] == 1 and np.asarray(b["padded"])[0].sum() == 0      # ends at the window
    assert sorted(np.asarray(b["padded"])[:, :, 0].sum(axis=1)) == [0, 0, 2, 3]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_header_declares_both_entry_points():
    from marl_amd import _lib
    res, args = _lib.SIGNATURES["marl_iql_loss_bwd"]
    assert res is _lib.I and len(args) == 21 and args[9:11] == [_lib.F, _lib.F] and args[16:20] == [_lib.I] * 4
    assert all(a is _lib.P for a in args[:9] + args[11:16] + args[20:])
    res, args = _lib.SIGNATURES["marl_iql_select"]
    assert res is _lib.I and len(args) == 14 and args[6] is _lib.F and args[9:13] == [_lib.I] * 4


# ------------------------------------------------------------------------------------------------ runner and launcher
class _Logger:
    def setup_tb(self, path):
        pass


def _runner_with_stubs(monkeypatch, tmp_path, **over):
    from marl_amd import runner
    built = []
    # (the controllers of the agent switches are the real ones: the runner's switch table holds the classes themselves)
    for name in ("RolloutWorker", "ReplayBuffer", "SharedMAC", "IQLLearner", "QLearner", "QTRANLearner"):
        monkeypatch.setattr(runner, name, lambda *a, _n=name, **k: built.append(_n) or types.SimpleNamespace(kind=_n, record_sink=None))
    args = seeded.make_args("2s3z", "iql")
    args.result_dir = str(tmp_path)
    args.__dict__.update(over)
    return runner, args, built


def test_alg_iql_selects_iqllearner(monkeypatch, tmp_path):
    runner, args, built = _runner_with_stubs(monkeypatch, tmp_path)
    r = runner.Runner(None, _Logger(), args)
    assert r.learner.kind == "IQLLearner" and r.mac.kind == "SharedMAC" and r.buffer.kind == "ReplayBuffer" and not r.on_policy
    assert built == ["SharedMAC", "RolloutWorker", "ReplayBuffer", "IQLLearner"]
    # through the launcher's make_runner as well: it names no learner class for iql
    from marl_amd import main
    del built[:]
    r = main.make_runner(args, None, logger=_Logger())
    assert r.learner.kind == "IQLLearner" and "QLearner" not in built


@pytest.mark.parametrize("over,exc,text,before_build", [
    (dict(world_model=True), ValueError, "Mixer iql not recognised.", True),            # pinned by tests/test_host_logic.py
    (dict(RTW=True), ValueError, "learner iql cannot find!", False),                    # as they answered before IQLLearner existed
    (dict(MAIC=True), ValueError, "learner iql cannot find!", False),
], ids=["world_model", "RTW", "MAIC"])
def test_iql_with_an_agent_switch_answers_as_before(over, exc, text, before_build, monkeypatch, tmp_path):
    runner, args, built = _runner_with_stubs(monkeypatch, tmp_path, **over)
    with pytest.raises(exc) as info:
        runner.Runner(None, _Logger(), args)
    assert type(info.value) is exc and str(info.value) == text
    assert "IQLLearner" not in built and (built == []) == before_build


def test_a_name_that_only_contains_iql_is_not_iql(monkeypatch, tmp_path):
    runner, args, built = _runner_with_stubs(monkeypatch, tmp_path, alg="iql+commnet")
    with pytest.raises(ValueError, match="learner iql\\+commnet cannot find!"):
        runner.Runner(None, _Logger(), args)
    assert "IQLLearner" not in built


@pytest.mark.parametrize("suffix", ["+commnet", "+g2anet"])
def test_launcher_refuses_iql_with_an_actor_suffix_as_it_refuses_qmix(suffix):
    from marl_amd import main
    texts = {}
    for base in ("iql", "qmix"):
        with pytest.raises(ValueError) as info:
            main.actor_base(base + suffix)
        texts[base] = str(info.value)
        with pytest.raises(ValueError) as info:
            main.build(["--alg", base + suffix, "--map", "2s3z", "--n_envs", "8"])
        assert str(info.value) == texts[base]
    assert texts["iql"] == texts["qmix"].replace("qmix", "iql")
    assert main.actor_base("iql") == ("iql", None)
