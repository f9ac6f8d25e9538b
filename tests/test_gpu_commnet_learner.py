"""The three +commnet algorithms on the MI355X: ReinforceLearner, CentralVLearner and COMALearner over CommNetMAC against the float64
oracles with the CommNet actor (tests/commnet_oracle.py), the unchanged plain path, and a training run of the launcher's runner.

Every comparison is the existing learner files' own ``compare_update`` (losses, intermediates under m, gradients before the clip,
norms and clip coefficients, every parameter after each step) run under commnet_oracle.commnet_actor, plus the logits under m.
Bounds: 1e-4 * max|ref| (tests/parity.close); the float32 exceptions are the critic's entries of the plain oracles' tables - the
critic's tensors are the plain runs' bit for bit, tests/test_commnet_cpu.py asserts it - and commnet_oracle.F32_EXCEPTIONS for the rest."""
import os

import numpy as np
import pytest
import torch

from oracle import learners
import parity
import commnet_oracle as cn
import coma_oracle as co
import pg_oracle as pg
import policy_oracle as po
import test_gpu_central_v as cv
import test_gpu_coma as tc
import test_gpu_reinforce as tr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def build_product(alg, name, **over):
    """(args, oracle state, batch(i), CommNetMAC, learner): the same seeded weights on both sides"""
    from marl_amd.controller.share_params import CommNetMAC
    from marl_amd.algorithm.central_v import CentralVLearner
    from marl_amd.algorithm.coma import COMALearner
    from marl_amd.algorithm.reinforce import ReinforceLearner
    args, state, batch = cn.learner_case(alg, name, **over)
    t = lambda d: {k: x.detach().to(torch.float32) for k, x in d.items()}
    mac = CommNetMAC(args)
    mac.agent.load_state_dict(t(state.agent))
    learner = {"reinforce": ReinforceLearner, "central_v": CentralVLearner, "coma": COMALearner}[alg](mac, args)
    if alg != "reinforce":
        learner.critic.load_state_dict(t(state.critic))
        learner.target_critic.load_state_dict(t(state.critic))
    return args, state, batch, mac, learner


def _critic_entry(tensor):
    t = tensor.split("/", 1)[1]
    return "critic." in t or t == "l_critic"


def _tables(monkeypatch):
    """the exception tables the three compare_update functions look into: the plain oracles' critic entries and the CommNet ones"""
    own = lambda alg: {k[1:]: v for k, v in cn.F32_EXCEPTIONS.items() if k[0] == alg}
    monkeypatch.setattr(pg, "F32_EXCEPTIONS", {("reinforce",) + k: v for k, v in own("reinforce").items()})
    monkeypatch.setattr(po, "F32_EXCEPTIONS", dict({k: v for k, v in po.F32_EXCEPTIONS.items() if _critic_entry(k[-1])}, **own("central_v")))
    monkeypatch.setattr(co, "F32_EXCEPTIONS", dict({k: v for k, v in co.F32_EXCEPTIONS.items() if _critic_entry(k[-1])}, **own("coma")))


def _logits(c, learner, inter):
    m = inter["mask"].numpy()[:, :, None, None]
    z = inter["logits"].detach().numpy()
    got = learner._dbg["logits"].view(z.shape).cpu().numpy()
    assert np.isfinite(got).all()                      # padded steps: finite, not the oracle's
    parity.close(c, "logits", got * m, z * m)


RUN_IDS = ["-".join(str(x) for x in r) for r in cn.RUNS]


@pytest.mark.parametrize("run", cn.RUNS, ids=RUN_IDS)
def test_two_updates_vs_oracle(run, monkeypatch):
    alg, name = run[0], run[1]
    _tables(monkeypatch)
    with cn.commnet_actor(cn.K_OF[name]):
        if alg == "reinforce":
            beta = run[2]
            args, state, batch, mac, learner = build_product(alg, name, policy_entropy_coef=beta)
            for i in (0, 1):
                c = "reinforce+commnet:%s beta=%g/step%d" % (name, beta, i)
                inter = tr.compare_update(c, name, i, learner, state, batch, beta)
                _logits(c, learner, inter)
        elif alg == "central_v":
            lam = run[2]
            args, state, batch, mac, learner = build_product(alg, name, td_lambda=lam)
            for i in (0, 1):
                c = "central_v+commnet:%s lam=%g/step%d" % (name, lam, i)
                inter = cv.compare_update(c, name, i, learner, state, batch, i, lam)
                _logits(c, learner, inter)
        else:
            lam, beta = run[2], run[3]
            args, state, batch, mac, learner = build_product(alg, name, td_lambda=lam, policy_entropy_coef=beta)
            for i in (0, 1):
                c = "coma+commnet:%s lam=%g/step%d" % (name, lam, i)
                inter = tc.compare_update(c, name, i, learner, state, batch, i, lam, beta)
                _logits(c, learner, inter)
    if name == "2s3z":
        assert inter["T"] == 5 < args.episode_limit
    assert learner.model_dir.endswith("/%s+commnet/%s" % (alg, args.map))


@pytest.mark.parametrize("alg", ["reinforce", "central_v", "coma"])
def test_plain_path_is_unchanged(alg, monkeypatch):
    """PolicyMAC: one update gives, bit for bit, the parameters a copy of the learner gives with the new dispatch bypassed -
    agent_backward called directly, no hs plane asked for"""
    from marl_amd.algorithm import common, policy_learner as mod         # the one module that calls the two seam functions
    build = {"reinforce": tr.build_product, "central_v": cv.build_product, "coma": tc.build_product}[alg]
    out = []
    for bypass in (False, True):
        with monkeypatch.context() as m:
            if bypass:
                m.setattr(mod, "policy_hs", lambda mac, g, shape: None)
                m.setattr(mod, "policy_backward", lambda mac, db, saved, hs, dlogits, buf: common.agent_backward(
                    mac, db, "cur", saved, None, dlogits, None, buf))
            args, state, batch, mac, learner = build("2s3z", "f32")
            assert not hasattr(mac, "backward")
            learner.train(learners.clone_batch(batch(0)), 0, epsilon=po.EPS)
            out.append((learner._flat.flat.clone(), learner._flat.gradx.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_end_to_end_through_main(tmp_path):
    """main.build and main.make_runner on --alg reinforce+commnet --map 2s3z --n_envs 8, then Runner.run (its evaluation cycle
    included) one iteration at a time for a few hundred environment steps, as the existing learner files drive it: episodes of 6 steps
    at most, not main.main's own loop over the map's 120 (the table's save_cycle of 5000 updates would write no checkpoint in a
    test's time, so the test saves one itself).  Finite losses, a checkpoint under
    reinforce+commnet/2s3z/, a fresh controller that loads it reproduces the logits of a fixed batch bit for bit; a Runner on the bare
    name without make_runner's classes answers "cannot find!" """
    from marl_amd.main import build, make_runner
    from marl_amd.runner import Runner
    from marl_amd.controller.share_params import CommNetMAC
    from marl_amd.algorithm.reinforce import ReinforceLearner
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    from marl_amd.utils.logging import Logger
    args, _ = build(["--map", "2s3z", "--alg", "reinforce+commnet", "--n_envs", "8", "--n_steps", "1", "--evaluate_epoch", "8",
                     "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "model")])
    assert args.k == 3
    args.episode_limit = 6
    env = SyntheticSMACEnv(8, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, 6, seed=args.seed)
    torch.manual_seed(3)
    r = make_runner(args, env, Logger())
    assert isinstance(r.mac, CommNetMAC) and isinstance(r.learner, ReinforceLearner) and r.buffer is None
    p0 = r.learner._flat.flat.clone()
    while r.time_steps < 300:
        loss = tr._iterate(r)
        assert np.isfinite(float(loss)) and np.isfinite(float(r.learner.entropy))
    assert r.train_steps >= 6 and not torch.equal(p0, r.learner._flat.flat)
    r.learner.save_models(0)
    d = r.learner.model_dir
    assert d.replace(os.sep, "/").endswith("/reinforce+commnet/2s3z") and sorted(os.listdir(d)) == ["0_rnn_net_params.pkl"]
    # a fixed batch: the last evaluation-style rollout's record, unrolled by the trained and by a fresh, loaded controller
    rec = r.rolloutWorker.generate_episodes(evaluate=True)[0].record
    E, T, N, A = 8, rec.T, args.n_agents, args.n_actions

    def logits_of(mac):
        z = torch.empty(E, T, N, A, device=DEV)
        mac.unroll(rec.obs, (T + 1) * N, 0, rec.u, T * N, -1, E, T, z, None, torch.empty(E * N, 64, device=DEV), None, h0=None)
        return z
    torch.manual_seed(99)
    fresh = CommNetMAC(args)
    fresh.cuda()
    assert not torch.equal(logits_of(fresh), logits_of(r.mac))
    fresh.load_models(d + "/0_rnn_net_params.pkl")
    assert torch.equal(logits_of(fresh), logits_of(r.mac))
    with pytest.raises(ValueError, match="cannot find!"):
        Runner(env, Logger(), args)
