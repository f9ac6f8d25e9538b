"""IQLLearner on the MI355X against tests/iql_oracle.py run over the oracle's float64 agent unroll: three updates in both gemm modes,
without double-Q, on TD(lambda) returns, the target sync, model files and resume state, hipGraph replay from a replay ring, and the
launcher.  Needs a real MI355X: ``pytest -m gpu``.

Bounds: those of the VDN learner parity test (tests/test_gpu_learners.py) - parity.close at 1e-4 * max|ref| (+ 1e-7) for the loss
and every parameter tensor of the first update, 1e-3 for the later ones (RMSprop's first steps amplify rounding) - in BOTH gemm
modes."""
import os

import numpy as np
import pytest
import torch

from oracle import seeded, learners
import iql_oracle as io
import parity

pytestmark = pytest.mark.gpu

B = io.LEARNER_B


def build_product(args, gemm_mode=None):
    from marl_amd.controller.share_params import SharedMAC
    from marl_amd.algorithm.iql import IQLLearner
    args.cuda = True
    if gemm_mode is not None:
        args.gemm_mode = gemm_mode
    mac = SharedMAC(args)
    agent = seeded.seeded_state(seeded.agent_param_shapes(args), seed=io.AGENT_SEED)
    mac.agent.load_state_dict({k: torch.tensor(x) for k, x in agent.items()})
    learner = IQLLearner(mac, args)
    return mac, learner


def plain(**more):
    """args and batches of the "double_q" case"""
    args, _, batch, _ = io.learner_case("double_q", **more)
    return args, batch


def three_updates(case, gemm_mode):
    """three updates of the product beside three of the float64 oracle; returns (learner, oracle state)"""
    args, st, batch_of, lam = io.learner_case(case)
    _, learner = build_product(io.learner_case(case)[0], gemm_mode)
    assert learner.mixer is None and learner.target_mixer is None and learner.td_lambda == lam
    for i, tol in enumerate(io.LEARNER_TOL):
        batch = batch_of(i)
        loss = learner.train(learners.clone_batch(batch), i)
        oloss, ograds, ointer = io.train(st, learners.clone_batch(batch), i, lam=lam)
        c = "iql_train:%s[%s]/step%d" % (case, gemm_mode, i)
        assert learner.max_episode_len == ointer["T"]
        parity.close(c, "loss", loss, oloss, tol=tol)
        den = float(learner.last_stats[1].item())
        assert den == float(ointer["den"]) == args.n_agents * float((1 - np.asarray(batch["padded"])[:, :ointer["T"]]).sum())
        d = learner._dbg
        assert set(d) == {"q_evals", "q_targets", "q_taken", "q_next"} | ({"td_targets"} if lam is not None else set())
        shape = (B, ointer["T"], args.n_agents)
        parity.close(c, "q_taken", d["q_taken"].reshape(shape).cpu().numpy(), ointer["q_taken"].numpy(), tol=tol)
        parity.close(c, "q_next", d["q_next"].reshape(shape).cpu().numpy(), ointer["q_next"].numpy(), tol=tol)
        if lam is not None:
            live = (1 - np.asarray(batch["padded"])[:, :ointer["T"]]).reshape(B, 1, -1)
            parity.close(c, "td_targets", d["td_targets"].cpu().numpy() * live, ointer["td_targets"].numpy() * live, tol=tol)
        for n, p in learner.eval_net.agent.named_parameters():
            if i == 0:
                parity.close(c, "grad " + n, p.grad.detach().cpu().numpy() / den, ograds["agent." + n].numpy(), tol=tol)
            parity.close(c, "param " + n, p.detach().cpu().numpy(), st.agent[n].detach().numpy(), tol=tol)
    return learner, st


def test_three_updates_vs_oracle(gemm_mode):
    three_updates("double_q", gemm_mode)


def test_three_updates_without_double_q(gemm_mode):
    three_updates("max", gemm_mode)


@pytest.mark.parametrize("lam", [0.0, 0.8])
def test_three_updates_on_lambda_returns(lam, gemm_mode):
    learner, st = three_updates("lam%g" % lam, gemm_mode)
    args, one, batch_of, _ = io.learner_case("double_q")
    if lam == 0.0:
        # lambda 0 is the one-step update: the same parameters, within the same tolerance, as the ONE-STEP oracle's
        for i in range(3):
            io.train(one, batch_of(i), i)
        for n, p in learner.eval_net.agent.named_parameters():
            parity.close("iql_train:lam0 vs one-step[%s]" % gemm_mode, "param " + n, p.detach().cpu().numpy(), one.agent[n].detach().numpy(), tol=1e-3)
    else:
        l1, _, _ = io.train(one, batch_of(0), 0)
        l8, _, _ = io.train(io.learner_case("double_q")[1], batch_of(0), 0, lam=0.8)
        assert abs(l8 - l1) > 1e-3 * abs(l1)                                         # another loss


def test_target_sync_fires_at_target_update_cycle():
    args, batch_of = plain(target_update_cycle=2)
    _, learner = build_product(args)
    tgt, cur = learner.target_net.agent._flat.flat, learner.eval_net.agent._flat.flat
    start = tgt.clone()
    assert torch.equal(tgt, cur)
    for i in range(3):
        assert np.isfinite(learner.train(learners.clone_batch(batch_of(i)), i))
        if i < 2:
            assert torch.equal(tgt, start) and not torch.equal(tgt, cur), i
        else:
            assert torch.equal(tgt, cur) and not torch.equal(tgt, start)
    with pytest.raises(NotImplementedError):
        learner.get_q_and_q_tot_table()


def test_model_files_and_resume_state(tmp_path):
    args, batch_of = plain(model_dir=str(tmp_path))
    _, learner = build_product(args)
    for i in range(2):
        learner.train(learners.clone_batch(batch_of(i)), i)
    learner.save_models(0)
    files = sorted(os.listdir(learner.model_dir))
    assert files == ["0_rnn_net_params.pkl"], files                                  # no mixer file
    os.rename(learner.model_dir + "/0_rnn_net_params.pkl", learner.model_dir + "/rnn_net_params.pkl")
    _, fresh = build_product(plain(model_dir=str(tmp_path))[0])
    assert not torch.equal(fresh._flat.flat, learner._flat.flat)
    fresh.load_models()
    assert torch.equal(fresh._flat.flat, learner._flat.flat)
    # resume state: parameters, the target agent (no target mixer), the optimizer - and the next update is the same, bit for bit
    sd = learner.resume_state()
    assert set(sd) == {"alg", "n_params", "params", "optimizer", "target_agent"} and sd["alg"] == "iql"
    ck = str(tmp_path / "resume.pt")
    learner.save_resume(ck)
    _, other = build_product(plain(model_dir=str(tmp_path))[0])
    other.load_resume(ck)
    for a, b in ((learner._flat.flat, other._flat.flat), (learner.target_net.agent._flat.flat, other.target_net.agent._flat.flat),
                 (learner.optimizer.s1, other.optimizer.s1)):
        assert torch.equal(a, b)
    assert other.optimizer.t == learner.optimizer.t == 2
    la = learner.train(learners.clone_batch(batch_of(2)), 2)
    lb = other.train(learners.clone_batch(batch_of(2)), 2)
    assert la == lb and torch.equal(learner._flat.flat, other._flat.flat)


def _ring_run(mode, updates, lam=None):
    """tests/test_gpu_edges.py:test_hip_graph_replay_equals_eager's loop on IQLLearner"""
    import bench
    from marl_amd.controller.share_params import SharedMAC
    from marl_amd.algorithm.iql import IQLLearner
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    from marl_amd.common.replaybuffer import ReplayBuffer
    args = bench.make_args("iql", "2s3z", 12)
    E = 96
    args.buffer_size, args.batch_size, args.hip_graph = 2 * E, E, mode
    if lam is not None:
        args.td_lambda = lam
    torch.manual_seed(0)
    np.random.seed(7)
    mac = SharedMAC(args)
    learner = IQLLearner(mac, args)
    env = SyntheticSMACEnv(E, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, 12, seed=3, fixed_length=True)
    w = RolloutWorker(env, mac, args)
    buf = ReplayBuffer(args)
    w.record_sink = buf
    losses = []
    for i in range(updates):
        buf.store_episode(w.generate_episodes(E)[0])
        losses.append(learner.train(buf.sample(E), i))
    return learner, losses, learner._flat.flat.detach().cpu().numpy().copy()


@pytest.mark.parametrize("lam", [None, 0.8])
def test_hip_graph_replay_equals_eager(lam):
    from marl_amd.algorithm.common import GraphedUpdate
    out = {}
    for mode in (False, True):
        learner, losses, flat = _ring_run(mode, GraphedUpdate.WARMUP + 2, lam)
        out[mode] = (losses, flat)
        if mode:
            g = learner.graphs
            assert not g.disabled, getattr(g, "error", "")
            assert any(e["graph"] is not None for e in g.entries.values()), "no graph was captured"
            assert g.replays >= 2
        else:
            assert learner.graphs is None
    assert all(np.isfinite(x) for x in out[False][0])
    assert out[False][0] == out[True][0]
    np.testing.assert_array_equal(out[False][1], out[True][1])


def test_launcher_trains_two_steps(tmp_path):
    from marl_amd.main import build, make_runner
    from marl_amd.algorithm.iql import IQLLearner
    from marl_amd.utils.logging import Logger
    args, env = build(["--alg", "iql", "--map", "2s3z", "--n_envs", "8", "--n_steps", "1", "--evaluate_epoch", "0",
                       "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "model")])
    args.save_cycle = 10 ** 9
    torch.manual_seed(3)
    r = make_runner(args, env, Logger())
    assert type(r.learner) is IQLLearner and r.buffer is not None and not r.on_policy
    before = r.learner._flat.flat.clone()
    for _ in range(2):
        r.args.n_steps = r.time_steps + 1
        r.run(0)
    assert r.train_steps == 2 == len(r.losses) and all(np.isfinite(float(x)) for x in r.losses)
    assert not torch.equal(before, r.learner._flat.flat)
