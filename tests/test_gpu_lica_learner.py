"""LICALearner on the MI355X against tests/lica_oracle.py (float64 autograd of the textbook critic and of the pi definition): two
consecutive updates across a target sync, the td_lambda settings, the entropy bonus, both gemm modes, the refusals, checkpoints and
resume, and the runner's on-policy loop.

Bounds: tests/parity.close at 1e-4 * max|ref| on every tensor.  The exceptions are the tensors whose FLOAT32 ORACLE already misses a
quarter of that (tests/test_lica_oracle_cpu.py measures it on the CPU): those alone are bounded by 4x their
float32-oracle error, lica_oracle.F32_EXCEPTIONS."""
import os

import numpy as np
import pytest
import torch

from oracle import learners
import lica_oracle as lo
import parity
import policy_oracle as po

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
NO_TABLE = "LICA has no Q table: its critic mixes the agents' action distributions into one value"


def build_product(name, gemm_mode=None, **over):
    """(args, oracle state, batch(i), controller, learner) of a learner case: the same seeded weights on both sides"""
    from marl_amd.controller.share_params import PolicyMAC
    from marl_amd.algorithm.lica import LICALearner
    args, state, batch = lo.learner_case(name, **over)
    if gemm_mode is not None:
        args.gemm_mode = gemm_mode
    t = lambda d: {k: x.detach().to(torch.float32) for k, x in d.items()}
    mac = PolicyMAC(args)
    mac.agent.load_state_dict(t(state.agent))
    learner = LICALearner(mac, args)
    learner.critic.load_state_dict(t(state.critic))
    learner.target_critic.load_state_dict(t(state.critic))
    return args, state, batch, mac, learner


def named_params(learner):
    return [("agent." + k, p) for k, p in learner.eval_net.agent.named_parameters()] + \
           [("critic." + k, p) for k, p in learner.critic.named_parameters()]


def bounded(c, key, name, got, ref):
    """parity.close, or 4x the float32-oracle error for the tensors lica_oracle.F32_EXCEPTIONS lists"""
    exc = lo.F32_EXCEPTIONS.get(key)
    if exc is None:
        return parity.close(c, name, got, ref)
    err = float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)).max())
    print("%s %s: err %.3e, bound 4 x %.2e" % (c, name, err, exc))
    assert err <= 4.0 * exc, (c, name, err, exc)
    return err


def compare_update(c, name, i, learner, state, batch, train_step, lam, beta=0.0):
    """one update on both sides and every comparison of it; returns the oracle's intermediates"""
    args = learner.args
    b = batch(i)
    loss = learner.train(learners.clone_batch(b), train_step, epsilon=lo.EPS)
    lc, la, ograds, inter = lo.train(state, learners.clone_batch(b), train_step, lo.EPS, lam, beta)
    assert lo.relu_near_zero(inter) == 0
    T, N, A = inter["T"], args.n_agents, args.n_actions
    B = inter["mask"].shape[0]
    assert learner.max_episode_len == T
    d = learner._dbg
    assert set(d) == {"logits", "q", "q_tgt", "q_next", "td_targets", "pi", "q_pi", "dpi", "dlogits", "ent"}
    mask = inter["mask"].numpy()
    key = lambda k: (name, 0.0 if lam is None else lam, beta, "step%d/%s" % (i, k))
    n = lambda k: inter[k].detach().numpy()
    shapes = dict(logits=(B, T, N, A), q=(B, T), q_tgt=(B, T), q_next=(B, T), pi=(B, T, N, A), q_pi=(B, T), dpi=(B, T, N * A),
                  dlogits=(B, T, N, A), ent=(B, T, N))
    for k, shape in shapes.items():
        got, ref = d[k].view(*shape).cpu().numpy(), n(k)
        if k in ("pi", "q_pi"):                                             # (a padded step's pi and Q(s, pi) are part of no loss)
            mk = mask.reshape(mask.shape + (1,) * (len(shape) - 2))
            got, ref = got * mk, ref * mk
        bounded(c, key(k), k, got, ref)
    bounded(c, key("td_targets"), "G", d["td_targets"].view(B, T).cpu().numpy() * mask, n("td_targets") * mask)
    bounded(c, key("l_critic"), "L_critic", float(loss), lc)
    bounded(c, key("l_actor"), "L_actor", float(learner.actor_loss), la)
    if beta != 0.0:
        bounded(c, key("entropy"), "entropy", float(learner.entropy), float(inter["entropy"].detach()))
    den, M = float(inter["den"]), float(inter["M"])
    assert float(learner.actor_stats[1].item()) == den == N * M and float(learner.last_stats[1].item()) == M
    for pn, p in named_params(learner):
        bounded(c, key("grad " + pn), "grad " + pn, p.grad.detach().cpu().numpy() / (den if pn.startswith("agent.") else M),
                ograds[pn].detach().numpy())
    for half, opt, dn in (("agent.", learner.optimizer, den), ("critic.", learner.critic_optimizer, M)):
        norm = float(torch.sqrt(opt.sumsq[0]).item()) / dn
        bounded(c, key(half + "grad_norm"), half + "grad_norm", norm, inter[half + "grad_norm"])
        bounded(c, key(half + "clip_coef"), half + "clip_coef", min(1.0, args.grad_norm_clip / (norm + 1e-6)), inter[half + "clip_coef"])
    oparams = dict([("agent." + k, x) for k, x in state.agent.items()] + [("critic." + k, x) for k, x in state.critic.items()])
    for pn, p in named_params(learner):
        bounded(c, key("param " + pn), "param " + pn, p.detach().cpu().numpy(), oparams[pn].detach().numpy())
    return inter


@pytest.mark.parametrize("name,gemm_mode", [("2s3z", "f32"), ("2s3z", "bf16x6"), ("MMM2", "f32"), ("matrix", "f32")])
def test_two_updates_across_a_target_sync(name, gemm_mode):
    """2s3z: ragged, one episode of length 1, one unterminated and cut at max_episode_len (no bootstrap), unavailable actions.
    target_update_cycle = 1: the target critic follows after the second update, not before"""
    args, state, batch, mac, learner = build_product(name, gemm_mode)
    assert args.target_update_cycle == 1
    init_critic = learner._cflat.flat.clone()
    for i in (0, 1):
        inter = compare_update("lica:%s[%s]/step%d" % (name, gemm_mode, i), name, i, learner, state, batch, i, 0.8)
        if name == "2s3z":
            assert inter["T"] == 5 < args.episode_limit and float(inter["M"]) == 1 + 5 + 4 + 5
            assert not learner._dbg["q_next"].view(4, 5)[:, 4].any()
        if i == 0:
            assert torch.equal(learner.target_critic._flat.flat, init_critic)       # no sync at train_step 0
    assert torch.equal(learner.target_critic._flat.flat, learner._cflat.flat) and not torch.equal(init_critic, learner._cflat.flat)
    for k, p in learner.target_critic.named_parameters():
        bounded("lica:%s/sync" % name, (name, 0.8, 0.0, "step1/param critic." + k), "target " + k, p.detach().cpu().numpy(),
                state.target_critic[k].numpy())
    with pytest.raises(NotImplementedError, match=NO_TABLE):
        learner.get_q_and_q_tot_table()


@pytest.mark.parametrize("lam", [0.0, 1.0])
def test_td_lambda_zero_and_one(lam):
    args, state, batch, mac, learner = build_product("2s3z", "f32", td_lambda=lam)
    for i in (0, 1):
        compare_update("lica:2s3z lam=%g/step%d" % (lam, i), "2s3z", i, learner, state, batch, i, lam)


def test_entropy_bonus_vs_oracle():
    beta = 0.01
    args, state, batch, mac, learner = build_product("2s3z", "f32", policy_entropy_coef=beta)
    assert learner.beta == beta
    for i in (0, 1):
        compare_update("lica+H:2s3z/step%d" % i, "2s3z", i, learner, state, batch, i, 0.8, beta)


def test_refusals(monkeypatch):
    from marl_amd.algorithm import lica, policy_learner
    from marl_amd.controller.share_params import PolicyMAC, SharedMAC
    args, _, _ = lo.learner_case("2s3z")

    class Reducer:
        enabled = True
    mac = PolicyMAC(args)
    with monkeypatch.context() as m:
        m.setattr(policy_learner, "GradReducer", Reducer)   # LICALearner's constructor is PolicyLearner's
        with pytest.raises(NotImplementedError):
            lica.LICALearner(mac, args)
    assert not hasattr(mac.agent, "_flat")                # nothing was built
    for field, bad, exc in (("td_lambda", 1.5, ValueError), ("policy_entropy_coef", -0.01, ValueError),
                            ("mixing_embed_dim", 65, ValueError)):
        keep = getattr(args, field)
        setattr(args, field, bad)
        with pytest.raises(exc):
            lica.LICALearner(mac, args)
        setattr(args, field, keep)
    with pytest.raises(ValueError):
        lica.LICALearner(SharedMAC(args), args)           # a non-stochastic controller


def test_checkpoints_and_resume_state(tmp_path):
    args, state, batch, mac, learner = build_product("2s3z", "f32", model_dir=str(tmp_path / "model"))
    learner.train(learners.clone_batch(batch(0)), 0, epsilon=lo.EPS)
    # model files: the published layout
    learner.save_models(0)
    d = learner.model_dir
    assert sorted(os.listdir(d)) == ["0_critic_net_params.pkl", "0_rnn_net_params.pkl"]
    sd = torch.load(d + "/0_critic_net_params.pkl")
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == lo.critic_param_shapes(args)
    for kind in ("rnn_net", "critic_net"):
        os.replace(d + "/0_%s_params.pkl" % kind, d + "/%s_params.pkl" % kind)
    args2, _, _, _, other = build_product("2s3z", "f32", model_dir=str(tmp_path / "model"))
    assert not torch.equal(other._cflat.flat, learner._cflat.flat)
    other.load_models()
    assert torch.equal(other._flat.flat, learner._flat.flat) and torch.equal(other._cflat.flat, learner._cflat.flat)
    # resume state: the next update is the same, bit for bit
    rs = learner.resume_state()
    assert rs["alg"] == "lica"
    args3, _, _, _, third = build_product("2s3z", "f32")
    third.load_resume_state(rs)
    losses = [x.train(learners.clone_batch(batch(1)), 1, epsilon=lo.EPS) for x in (learner, third)]
    assert float(losses[0]) == float(losses[1]) and float(learner.actor_loss) == float(third.actor_loss)
    for a, b in ((learner._flat.flat, third._flat.flat), (learner._cflat.flat, third._cflat.flat),
                 (learner.target_critic._flat.flat, third.target_critic._flat.flat), (learner.optimizer.s1, third.optimizer.s1),
                 (learner.critic_optimizer.s1, third.critic_optimizer.s1)):
        assert torch.equal(a, b)
    # a central-V resume state is refused (another alg, another critic)
    from marl_amd.algorithm.central_v import CentralVLearner
    from marl_amd.controller.share_params import PolicyMAC
    cargs, _, _ = po.learner_case("2s3z")
    cv = CentralVLearner(PolicyMAC(cargs), cargs)
    with pytest.raises(ValueError):
        third.load_resume_state(cv.resume_state())


# ---------------------------------------------------------------------------------------------------- the runner
def _build(tmp_path, tag, argv):
    from marl_amd.main import build
    return build(list(argv) + ["--alg", "lica", "--result_dir", str(tmp_path / (tag + "_res")),
                               "--model_dir", str(tmp_path / (tag + "_model"))])


def _two_iterations(r, stop=False):
    """two on-policy updates with target_update_cycle = 1: finite losses, both networks move, the target critic follows at the sync
    (after the second update) and only there.  ``stop``: episode lengths vary, so the loop is ended after the second update by
    taking --n_steps down, not by a step count worked out ahead"""
    r.args.target_update_cycle = 1
    a0, c0, t0 = r.learner._flat.flat.clone(), r.learner._cflat.flat.clone(), r.learner.target_critic._flat.flat.clone()
    assert torch.equal(c0, t0)
    seen = []
    step = r.learner._finish_update

    def spy(train_step):
        out = step(train_step)
        seen.append((train_step, r.learner.target_critic._flat.flat.clone(), r.learner._cflat.flat.clone()))
        if stop and train_step == 1:
            r.args.n_steps = 0
        return out
    r.learner._finish_update = spy
    loss = r.run(0)
    assert r.train_steps == 2 == len(r.losses) == len(seen)
    assert all(np.isfinite(float(x)) for x in r.losses) and np.isfinite(float(loss)) and np.isfinite(float(r.learner.actor_loss))
    assert not torch.equal(a0, r.learner._flat.flat) and not torch.equal(c0, r.learner._cflat.flat)
    (s0, tgt0, cr0), (s1, tgt1, cr1) = seen
    assert (s0, s1) == (0, 1)
    assert torch.equal(tgt0, t0) and not torch.equal(cr0, c0)                # update 0: the critic moved, the target did not
    assert torch.equal(tgt1, cr1) and not torch.equal(tgt1, t0)              # update 1: the sync
    with pytest.raises(NotImplementedError, match=NO_TABLE):
        r.learner.get_q_and_q_tot_table()


def test_runner_matrix_game_two_iterations(tmp_path):
    from marl_amd.algorithm.lica import LICALearner
    from marl_amd.main import make_runner
    args, env = _build(tmp_path, "m", ["--env", "matrix", "--n_envs", "8", "--n_steps", "16", "--evaluate_epoch", "8"])
    assert (args.n_agents, args.n_actions, args.state_shape) == (2, 3, 1) and args.td_lambda == 0.8
    torch.manual_seed(3)
    r = make_runner(args, env)
    assert isinstance(r.learner, LICALearner) and r.buffer is None
    _two_iterations(r)


def test_runner_2s3z_two_iterations(tmp_path):
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    from marl_amd.main import make_runner
    args, _ = _build(tmp_path, "s", ["--map", "2s3z", "--n_envs", "8", "--n_steps", "100000", "--evaluate_epoch", "8"])
    args.episode_limit = 6
    env = SyntheticSMACEnv(8, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, 6, seed=args.seed)
    torch.manual_seed(3)
    r = make_runner(args, env)
    _two_iterations(r, stop=True)


def test_runner_refusals(tmp_path):
    from marl_amd.main import make_runner
    from marl_amd.runner import Runner
    from marl_amd.utils.logging import Logger
    for over, exc in ((dict(overlap_rollout=True), NotImplementedError), (dict(world_model=True), ValueError),
                      (dict(RTW=True), ValueError), (dict(MAIC=True), ValueError)):
        args, env = _build(tmp_path, "r", ["--env", "matrix", "--n_envs", "8"])
        for k, v in over.items():
            setattr(args, k, v)
        with pytest.raises(exc):
            make_runner(args, env)
    # the learner is named by the launcher: a Runner on the bare name keeps refusing it
    args, env = _build(tmp_path, "r", ["--env", "matrix", "--n_envs", "8"])
    with pytest.raises(ValueError, match="learner lica cannot find!"):
        Runner(env, Logger(), args)
