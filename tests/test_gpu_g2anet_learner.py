"""The three +g2anet algorithms on the MI355X: ReinforceLearner, CentralVLearner and COMALearner over G2ANetMAC against the float64
oracles with the G2ANet actor (tests/g2anet_oracle.py), the unchanged PolicyMAC and CommNetMAC paths, and a training run of the
launcher's runner.

Every comparison is the existing learner files' own ``compare_update`` (losses, intermediates under m, gradients before the clip,
norms and clip coefficients, every parameter after each step) run under g2anet_oracle.g2anet_actor, plus the logits under m.  The
oracle consumes the float32 noise the device draws for (args.seed, train step), read back once per update.  Bounds: 1e-4 * max|ref|
(tests/parity.close); the float32 exceptions are the critic's entries of the plain oracles' tables - the critic's tensors are the
plain runs' bit for bit, tests/test_g2anet_cpu.py asserts it - and g2anet_oracle.F32_EXCEPTIONS for the rest."""
import os

import numpy as np
import pytest
import torch

from oracle import learners
import parity
import g2anet_oracle as go
import coma_oracle as co
import pg_oracle as pg
import policy_oracle as po
import test_gpu_central_v as cv
import test_gpu_coma as tc
import test_gpu_commnet_learner as tcn
import test_gpu_reinforce as tr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def build_product(alg, name, **over):
    """(args, oracle state, batch(i), G2ANetMAC, learner): the same seeded weights on both sides"""
    from marl_amd.controller.share_params import G2ANetMAC
    from marl_amd.algorithm.central_v import CentralVLearner
    from marl_amd.algorithm.coma import COMALearner
    from marl_amd.algorithm.reinforce import ReinforceLearner
    args, state, batch = go.learner_case(alg, name, **over)
    t = lambda d: {k: x.detach().to(torch.float32) for k, x in d.items()}
    mac = G2ANetMAC(args)
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
    """the exception tables the three compare_update functions look into: the plain oracles' critic entries and the G2ANet ones"""
    own = lambda alg: {k[1:]: v for k, v in go.F32_EXCEPTIONS.items() if k[0] == alg}
    monkeypatch.setattr(pg, "F32_EXCEPTIONS", {("reinforce",) + k: v for k, v in own("reinforce").items()})
    monkeypatch.setattr(po, "F32_EXCEPTIONS", dict({k: v for k, v in po.F32_EXCEPTIONS.items() if _critic_entry(k[-1])}, **own("central_v")))
    monkeypatch.setattr(co, "F32_EXCEPTIONS", dict({k: v for k, v in co.F32_EXCEPTIONS.items() if _critic_entry(k[-1])}, **own("coma")))


def _device_noise(args):
    """the update's noise as the device draws it, read back: what the oracle consumes"""
    from marl_amd import ops
    from marl_amd.controller.share_params import G2ANET_UPDATE_SALT

    def noise_fn(step, B, T, N):
        buf = torch.empty(B, T, N, N - 1, device=DEV)
        ops.g2anet_noise(args.seed ^ G2ANET_UPDATE_SALT, 0, step * args.episode_limit, buf, B, T, N)
        return buf.cpu().numpy()
    return noise_fn


def _logits(c, learner, inter):
    m = inter["mask"].numpy()[:, :, None, None]
    z = inter["logits"].detach().numpy()
    got = learner._dbg["logits"].view(z.shape).cpu().numpy()
    assert np.isfinite(got).all()
    parity.close(c, "logits", got * m, z * m)


RUN_IDS = ["-".join(str(x) for x in r) for r in go.RUNS]


@pytest.mark.parametrize("run", go.RUNS, ids=RUN_IDS)
def test_two_updates_vs_oracle(run, monkeypatch):
    alg, name = run[0], run[1]
    _tables(monkeypatch)
    over = dict(policy_entropy_coef=run[2]) if alg == "reinforce" else dict(td_lambda=run[2])
    if alg == "coma":
        over["policy_entropy_coef"] = run[3]
    args, state, batch, mac, learner = build_product(alg, name, **over)
    with go.g2anet_actor(_device_noise(args)) as actor:
        for i in (0, 1):
            actor.step = i
            c = "%s+g2anet:%s %s/step%d" % (alg, name, "-".join(str(x) for x in run[2:]), i)
            if alg == "reinforce":
                inter = tr.compare_update(c, name, i, learner, state, batch, run[2])
            elif alg == "central_v":
                inter = cv.compare_update(c, name, i, learner, state, batch, i, run[2])
            else:
                inter = tc.compare_update(c, name, i, learner, state, batch, i, run[2], run[3])
            _logits(c, learner, inter)
            assert mac.train_step == i
    if name == "2s3z":
        assert inter["T"] == 5 < args.episode_limit
    assert learner.model_dir.endswith("/%s+g2anet/%s" % (alg, args.map))


@pytest.mark.parametrize("alg", ["reinforce", "central_v", "coma"])
def test_plain_path_is_unchanged(alg, monkeypatch):
    """PolicyMAC: one update gives, bit for bit, the parameters a copy of the learner gives with the seam bypassed - agent_backward
    called directly, no planes asked for; the controller has no train-step setter to call"""
    from marl_amd.algorithm import common, policy_learner as mod
    build = {"reinforce": tr.build_product, "central_v": cv.build_product, "coma": tc.build_product}[alg]
    out = []
    for bypass in (False, True):
        with monkeypatch.context() as m:
            if bypass:
                m.setattr(mod, "policy_hs", lambda mac, g, shape: None)
                m.setattr(mod, "policy_backward", lambda mac, db, saved, hs, dlogits, buf: common.agent_backward(
                    mac, db, "cur", saved, None, dlogits, None, buf))
            args, state, batch, mac, learner = build("2s3z", "f32")
            assert not hasattr(mac, "backward") and not hasattr(mac, "set_train_step")
            learner.train(learners.clone_batch(batch(0)), 7, epsilon=po.EPS)
            out.append((learner._flat.flat.clone(), learner._flat.gradx.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_commnet_path_is_unchanged():
    """CommNetMAC: an update does not depend on the train step it is told (no setter, no noise), bit for bit"""
    out = []
    for step in (0, 7):
        args, state, batch, mac, learner = tcn.build_product("reinforce", "2s3z")
        assert not hasattr(mac, "set_train_step")
        learner.train(learners.clone_batch(batch(0)), step, epsilon=po.EPS)
        out.append((learner._flat.flat.clone(), learner._flat.gradx.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_update_noise_is_keyed_by_the_train_step():
    """the same batch at the same step: the same bits (a resume redraws the same noise); at another step: other logits"""
    out = []
    for step in (0, 0, 1):
        args, state, batch, mac, learner = build_product("reinforce", "2s3z")
        learner.train(learners.clone_batch(batch(0)), step, epsilon=po.EPS)
        out.append((learner._dbg["logits"].clone(), learner._flat.flat.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and not torch.equal(out[0][0], out[2][0])


def test_end_to_end_through_main(tmp_path):
    """main.build and main.make_runner on --alg reinforce+g2anet --map 2s3z --n_envs 8, then Runner.run one iteration at a time for a
    handful of updates with episodes of 6 steps at most: finite losses, parameters that move, a checkpoint of the 22 tensors under
    reinforce+g2anet/2s3z/ that a fresh controller loads to the same bits; a Runner on the bare name answers "cannot find!" """
    from marl_amd.main import build, make_runner
    from marl_amd.runner import Runner
    from marl_amd.controller.share_params import G2ANetMAC
    from marl_amd.algorithm.reinforce import ReinforceLearner
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    from marl_amd.utils.logging import Logger
    args, _ = build(["--map", "2s3z", "--alg", "reinforce+g2anet", "--n_envs", "8", "--n_steps", "1", "--evaluate_epoch", "8",
                     "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "model")])
    assert args.hard is True
    args.episode_limit = 6
    env = SyntheticSMACEnv(8, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, 6, seed=args.seed)
    torch.manual_seed(3)
    r = make_runner(args, env, Logger())
    assert isinstance(r.mac, G2ANetMAC) and isinstance(r.learner, ReinforceLearner) and r.buffer is None
    p0 = r.learner._flat.flat.clone()
    while r.time_steps < 150:
        loss = tr._iterate(r)
        assert np.isfinite(float(loss)) and np.isfinite(float(r.learner.entropy))
    assert r.train_steps >= 3 and not torch.equal(p0, r.learner._flat.flat) and r.mac.train_step == r.train_steps - 1
    r.learner.save_models(0)
    d = r.learner.model_dir
    assert d.replace(os.sep, "/").endswith("/reinforce+g2anet/2s3z") and sorted(os.listdir(d)) == ["0_rnn_net_params.pkl"]
    sd = torch.load(d + "/0_rnn_net_params.pkl", map_location="cpu")
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == go.param_shapes(args)
    torch.manual_seed(99)
    fresh = G2ANetMAC(args)
    fresh.cuda()
    trained = {k: v.detach().cpu() for k, v in r.mac.agent.state_dict().items()}
    assert not all(torch.equal(v.cpu(), trained[k]) for k, v in fresh.agent.state_dict().items())
    fresh.load_models(d + "/0_rnn_net_params.pkl")
    assert all(torch.equal(v.cpu(), trained[k]) for k, v in fresh.agent.state_dict().items())
    rec = r.rolloutWorker.generate_episodes(evaluate=True)[0].record
    E, T, N, A = 8, rec.T, args.n_agents, args.n_actions

    def logits_of(mac):
        z = torch.empty(E, T, N, A, device=DEV)
        mac.set_train_step(5)
        mac.unroll(rec.obs, (T + 1) * N, 0, rec.u, T * N, -1, E, T, z, None, torch.empty(E * N, 64, device=DEV), None, h0=None)
        return z
    assert torch.equal(logits_of(fresh), logits_of(r.mac))
    with pytest.raises(ValueError, match="cannot find!"):
        Runner(env, Logger(), args)
