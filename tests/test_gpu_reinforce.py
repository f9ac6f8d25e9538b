"""REINFORCE and the entropy bonus on the MI355X: ReinforceLearner and CentralVLearner with policy_entropy_coef against
tests/pg_oracle.py (float64), the refusals, the runner's on-policy loop with --alg reinforce and the launcher's argument table.

Bounds: tests/parity.close at 1e-4 * max|ref| on every tensor of both updates; a tensor whose FLOAT32 ORACLE already misses a
quarter of that (tests/test_pg_oracle_cpu.py measures it) is bounded by 4x its float32-oracle error,
pg_oracle.F32_EXCEPTIONS."""
import os

import numpy as np
import pytest
import torch

from oracle import learners
import parity
import pg_oracle as pg
import policy_oracle as po
import test_gpu_central_v as cv

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def build_product(name, gemm_mode=None, **over):
    """(args, oracle state, batch(i), controller, learner) of a REINFORCE case: the same seeded weights on both sides"""
    from marl_amd.controller.share_params import PolicyMAC
    from marl_amd.algorithm.reinforce import ReinforceLearner
    args, state, batch = pg.learner_case(name, **over)
    if gemm_mode is not None:
        args.gemm_mode = gemm_mode
    mac = PolicyMAC(args)
    mac.agent.load_state_dict({k: x.detach().to(torch.float32) for k, x in state.agent.items()})
    return args, state, batch, mac, ReinforceLearner(mac, args)


def compare_update(c, name, i, learner, state, batch, beta):
    """one update on both sides and every comparison of it; returns the oracle's intermediates"""
    args = learner.args
    b = batch(i)
    loss = learner.train(learners.clone_batch(b), i, epsilon=pg.EPS)
    lo, ograds, inter = pg.train(state, learners.clone_batch(b), i, pg.EPS, beta)
    assert po.relu_near_zero(inter) == 0
    T, N = inter["T"], args.n_agents
    B = inter["mask"].shape[0]
    assert learner.max_episode_len == T
    d = learner._dbg
    assert set(d) == {"logits", "td_targets", "logp", "ent", "dlogits"}
    mask = inter["mask"].numpy()
    parity.close(c, "G", d["td_targets"].view(B, T).cpu().numpy() * mask, inter["td_targets"].numpy() * mask)
    parity.close(c, "logp", d["logp"].view(B, T, N).cpu().numpy(), inter["logp"].detach().numpy())
    parity.close(c, "ent", d["ent"].view(B, T, N).cpu().numpy(), inter["ent"].detach().numpy())
    parity.close(c, "loss", float(loss), lo)
    parity.close(c, "entropy", float(learner.entropy), float(inter["entropy"].detach()))
    den = float(learner.last_stats[1].item())
    assert den == float(inter["den"])
    named = [("agent." + k, p) for k, p in learner.eval_net.agent.named_parameters()]
    for n, p in named:
        parity.close(c, "grad " + n, p.grad.detach().cpu().numpy() / den, ograds[n].detach().numpy())
    norm = float(torch.sqrt(learner.optimizer.sumsq[0]).item()) / den
    parity.close(c, "grad_norm", norm, inter["agent.grad_norm"])
    parity.close(c, "clip_coef", min(1.0, args.grad_norm_clip / (norm + 1e-6)), inter["agent.clip_coef"])
    for n, p in named:
        ref = state.agent[n[len("agent."):]].detach().numpy()
        exc = pg.F32_EXCEPTIONS.get(("reinforce", name, beta, "step%d/param %s" % (i, n)))
        if exc is None:
            parity.close(c, "param " + n, p.detach().cpu().numpy(), ref)
        else:
            err = float(np.abs(p.detach().cpu().numpy() - ref).max())
            print("%s param %s: err %.3e, bound 4 x %.2e" % (c, n, err, exc))
            assert err <= 4.0 * exc, (c, n, err, exc)
    return inter


@pytest.mark.parametrize("beta", pg.BETAS)
@pytest.mark.parametrize("name,gemm_mode", [("2s3z", "f32"), ("2s3z", "bf16x6"), ("MMM2", "f32"), ("matrix", "f32")])
def test_two_updates_vs_oracle(name, gemm_mode, beta):
    """2s3z: ragged, one episode of length 1, one unterminated and cut at max_episode_len (quirk Q2: no bootstrap), unavailable
    actions"""
    args, state, batch, mac, learner = build_product(name, gemm_mode, policy_entropy_coef=beta)
    args.target_update_cycle = None                            # not read
    for i in (0, 1):
        inter = compare_update("reinforce:%s[%s] beta=%g/step%d" % (name, gemm_mode, beta, i), name, i, learner, state, batch, beta)
        if name == "2s3z":
            assert inter["T"] == 5 < args.episode_limit and float(inter["M"]) == 1 + 5 + 4 + 5
    with pytest.raises(NotImplementedError):
        learner.get_q_and_q_tot_table()


def test_central_v_with_the_bonus_vs_oracle(monkeypatch):
    """two updates of CentralVLearner at policy_entropy_coef = 0.01 on 2s3z: every comparison of test_gpu_central_v's update, with
    the oracle's actor loss carrying the bonus, and H / the mean entropy on top"""
    beta = 0.01
    args, state, batch, mac, learner = cv.build_product("2s3z", "f32", policy_entropy_coef=beta)
    monkeypatch.setattr(po, "train", lambda st, b, ts, eps, lam: pg.central_v_train(st, b, ts, eps, lam, beta))
    for i in (0, 1):
        c = "central_v+H:2s3z/step%d" % i
        inter = cv.compare_update(c, "2s3z", i, learner, state, batch, i, 0.8)
        B, T, N = inter["ent"].shape
        parity.close(c, "ent", learner._dbg["ent"].view(B, T, N).cpu().numpy(), inter["ent"].detach().numpy())
        parity.close(c, "entropy", float(learner.entropy), float(inter["entropy"].detach()))


def test_central_v_without_the_bonus_launches_no_ex(monkeypatch):
    from marl_amd import ops

    def refuse(*a, **k):
        raise AssertionError("policy_loss_bwd_ex launched at policy_entropy_coef = 0")
    monkeypatch.setattr(ops, "policy_loss_bwd_ex", refuse)
    for over in ({}, {"policy_entropy_coef": 0.0}):
        args, state, batch, mac, learner = cv.build_product("2s3z", "f32", **over)
        assert np.isfinite(float(learner.train(learners.clone_batch(batch(0)), 0, epsilon=po.EPS)))
        assert "ent" not in learner._dbg


def test_refusals(monkeypatch):
    from marl_amd.algorithm import reinforce, central_v, policy_learner
    from marl_amd.controller.share_params import PolicyMAC, SharedMAC
    args, _, _ = pg.learner_case("2s3z")

    class Reducer:
        enabled = True
    mac = PolicyMAC(args)
    with monkeypatch.context() as m:
        m.setattr(policy_learner, "GradReducer", Reducer)    # the constructor is PolicyLearner's
        with pytest.raises(NotImplementedError):
            reinforce.ReinforceLearner(mac, args)
    assert not hasattr(mac.agent, "_flat")                # nothing was built
    args.policy_entropy_coef = -0.01
    with pytest.raises(ValueError):
        reinforce.ReinforceLearner(mac, args)
    cargs, _, _ = po.learner_case("2s3z", policy_entropy_coef=-0.01)
    with pytest.raises(ValueError):
        central_v.CentralVLearner(mac, cargs)
    assert not hasattr(mac.agent, "_flat")
    args.policy_entropy_coef = 0.0
    with pytest.raises(ValueError):
        reinforce.ReinforceLearner(SharedMAC(args), args)


# ---------------------------------------------------------------------------------------------------- the runner
def _runner(tmp_path, tag, argv=(), **over):
    """--alg reinforce on the synthetic 2s3z environment: 8 environments, episodes of 6 steps at most"""
    from marl_amd.main import build
    from marl_amd.runner import Runner
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    from marl_amd.utils.logging import Logger
    args, _ = build(["--map", "2s3z", "--alg", "reinforce", "--n_envs", "8", "--n_steps", "1", "--evaluate_epoch", "8",
                     "--result_dir", str(tmp_path / (tag + "_res")), "--model_dir", str(tmp_path / (tag + "_model"))] + list(argv))
    args.episode_limit = 6
    env = SyntheticSMACEnv(8, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, 6, seed=args.seed)
    for k, v in over.items():
        setattr(args, k, v)
    torch.manual_seed(3)
    return args, env, (lambda: Runner(env, Logger(), args))


def _iterate(r):
    r.args.n_steps = r.time_steps + 1
    return r.run(0)


def test_runner_trains_on_policy(tmp_path):
    from marl_amd.algorithm.reinforce import ReinforceLearner
    args, env, make = _runner(tmp_path, "a", ["--policy_entropy_coef", "0.01"])
    r = make()
    assert isinstance(r.learner, ReinforceLearner) and r.learner.beta == 0.01 and r.buffer is None
    p0 = r.learner._flat.flat.clone()
    for k in range(3):
        loss = _iterate(r)
        assert np.isfinite(float(loss)) and np.isfinite(float(r.learner.entropy)) and float(r.learner.entropy) > 0
        np.testing.assert_allclose(r.rolloutWorker.epsilon, 0.5 - (k + 1) * 0.00064, rtol=1e-12)      # one anneal per rollout
    assert r.train_steps == 3 == len(r.losses) and all(np.isfinite(float(x)) for x in r.losses)
    assert not torch.equal(p0, r.learner._flat.flat)
    # model files: the rnn parameters alone
    r.learner.save_models(0)
    d = r.learner.model_dir
    assert sorted(os.listdir(d)) == ["0_rnn_net_params.pkl"]
    os.replace(d + "/0_rnn_net_params.pkl", d + "/rnn_net_params.pkl")
    args2, env2, make2 = _runner(tmp_path, "b")
    r2 = make2()
    assert not torch.equal(r2.learner._flat.flat, r.learner._flat.flat)
    r2.learner.model_dir = d
    r2.learner.load_models()
    assert torch.equal(r2.learner._flat.flat, r.learner._flat.flat)
    # full resume: the next iteration is the same, bit for bit
    ck = str(tmp_path / "resume.pt")
    r.save_resume(ck)
    args3, env3, make3 = _runner(tmp_path, "c", ["--policy_entropy_coef", "0.01"], resume=ck)
    r3 = make3()
    assert (r3.train_steps, r3.rolloutWorker.epsilon, r3.env.episode) == (r.train_steps, r.rolloutWorker.epsilon, r.env.episode)
    for x in (r, r3):
        _iterate(x)
    assert float(r.losses[-1]) == float(r3.losses[-1]) and len(r3.losses) == 1
    assert torch.equal(r.learner._flat.flat, r3.learner._flat.flat) and torch.equal(r.learner.optimizer.s1, r3.learner.optimizer.s1)
    # a resume state of another learner is refused
    sd = r.learner.resume_state()
    sd["alg"] = "central_v"
    with pytest.raises(ValueError):
        r3.learner.load_resume_state(sd)


def test_runner_refusals(tmp_path):
    args, env, make = _runner(tmp_path, "o", overlap_rollout=True)
    with pytest.raises(NotImplementedError):
        make()
    for switch in ("world_model", "RTW", "MAIC"):
        args, env, make = _runner(tmp_path, "w" + switch, **{switch: True})
        with pytest.raises(ValueError):
            make()
    args, env, make = _runner(tmp_path, "c")
    args.alg = "coma"
    with pytest.raises(ValueError, match="learner coma cannot find!"):
        make()


def test_launcher_builds_the_reinforce_table():
    from marl_amd.main import build
    args, env = build(["--alg", "reinforce", "--map", "2s3z", "--n_envs", "2"])
    assert (args.lr_actor, args.epsilon, args.epsilon_anneal_scale) == (1e-4, 0.5, "episode")
    assert args.policy_entropy_coef == 0.0 and (args.n_agents, args.n_actions) == (5, 11)
