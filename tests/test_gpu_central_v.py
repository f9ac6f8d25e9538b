"""Central-V on the MI355X: CentralVLearner against tests/policy_oracle.py (float64) in both gemm modes, the td_lambda settings, the
refusals, the sampling rollout of PolicyMAC, and the runner's on-policy loop.

Bounds: tests/parity.close at 1e-4 * max|ref| on every tensor of both updates.  The exceptions are the tensors whose FLOAT32
ORACLE already misses a quarter of that (tests/test_policy_oracle_cpu.py measures it; DESIGN section 10 lists them): those alone
are bounded by 4x their float32-oracle error, policy_oracle.F32_EXCEPTIONS."""
import os

import numpy as np
import pytest
import torch

from oracle import learners, nets, seeded
import parity
import policy_oracle as po

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def build_product(name, gemm_mode=None, **over):
    """(args, oracle state, batch(i), controller, learner) of a learner case: the same seeded weights on both sides"""
    from marl_amd.controller.share_params import PolicyMAC
    from marl_amd.algorithm.central_v import CentralVLearner
    args, state, batch = po.learner_case(name, **over)
    if gemm_mode is not None:
        args.gemm_mode = gemm_mode
    t = lambda d: {k: x.detach().to(torch.float32) for k, x in d.items()}
    mac = PolicyMAC(args)
    mac.agent.load_state_dict(t(state.agent))
    learner = CentralVLearner(mac, args)
    learner.critic.load_state_dict(t(state.critic))
    learner.target_critic.load_state_dict(t(state.critic))
    return args, state, batch, mac, learner


def named_params(learner):
    return [("agent." + k, p) for k, p in learner.eval_net.agent.named_parameters()] + \
           [("critic." + k, p) for k, p in learner.critic.named_parameters()]


def compare_update(c, name, i, learner, state, batch, train_step, lam):
    """one update on both sides and every comparison of it; returns the oracle's intermediates"""
    args = learner.args
    b = batch(i)
    loss = learner.train(learners.clone_batch(b), train_step, epsilon=po.EPS)
    lc, la, ograds, inter = po.train(state, learners.clone_batch(b), train_step, po.EPS, lam)
    assert po.relu_near_zero(inter) == 0
    T, N = inter["T"], args.n_agents
    B = inter["v"].shape[0]
    assert learner.max_episode_len == T
    d = learner._dbg
    V, G = d["v"].view(B, T).cpu().numpy(), d["td_targets"].view(B, T).cpu().numpy()
    mask = inter["mask"].numpy()
    parity.close(c, "V", V, inter["v"].detach().numpy())
    parity.close(c, "G", G * mask, inter["td_targets"].numpy() * mask)          # (a padded step's G is not part of any loss)
    parity.close(c, "Adv", (G - V) * mask, inter["adv"].numpy() * mask)
    parity.close(c, "logp", d["logp"].view(B, T, N).cpu().numpy(), inter["logp"].detach().numpy())
    parity.close(c, "L_critic", float(loss), lc)
    parity.close(c, "L_actor", float(learner.actor_loss), la)
    dens = {"agent.": float(learner.actor_stats[1].item()), "critic.": float(learner.last_stats[1].item())}
    assert dens["critic."] == float(inter["M"]) and dens["agent."] == float(inter["den_actor"])
    for n, p in named_params(learner):
        parity.close(c, "grad " + n, p.grad.detach().cpu().numpy() / dens[n.split(".")[0] + "."], ograds[n].detach().numpy())
    for half, opt in (("agent.", learner.optimizer), ("critic.", learner.critic_optimizer)):
        norm = float(torch.sqrt(opt.sumsq[0]).item()) / dens[half]
        parity.close(c, half + "grad_norm", norm, inter[half + "grad_norm"])
        parity.close(c, half + "clip_coef", min(1.0, args.grad_norm_clip / (norm + 1e-6)), inter[half + "clip_coef"])
    oparams = dict([("agent." + k, x) for k, x in state.agent.items()] + [("critic." + k, x) for k, x in state.critic.items()])
    for n, p in named_params(learner):
        ref = oparams[n].detach().numpy()
        exc = po.F32_EXCEPTIONS.get((name, lam, "step%d/param %s" % (i, n)))
        if exc is None:
            parity.close(c, "param " + n, p.detach().cpu().numpy(), ref)
        else:
            err = float(np.abs(p.detach().cpu().numpy() - ref).max())
            print("%s param %s: err %.3e, bound 4 x %.2e" % (c, n, err, exc))
            assert err <= 4.0 * exc, (c, n, err, exc)
    return inter


@pytest.mark.parametrize("name,gemm_mode", [("2s3z", "f32"), ("2s3z", "bf16x6"), ("MMM2", "f32"), ("matrix", "f32")])
def test_two_updates_vs_oracle(name, gemm_mode):
    """2s3z: ragged, one episode of length 1, one unterminated and cut at max_episode_len (quirk Q2), unavailable actions"""
    args, state, batch, mac, learner = build_product(name, gemm_mode)
    init_critic = learner._cflat.flat.clone()
    for i in (0, 1):
        inter = compare_update("central_v:%s[%s]/step%d" % (name, gemm_mode, i), name, i, learner, state, batch, i, 0.8)
        if name == "2s3z":
            assert inter["T"] == 5 < args.episode_limit and float(inter["M"]) == 1 + 5 + 4 + 5
    assert torch.equal(learner.target_critic._flat.flat, init_critic)      # no sync at train_step 0 and 1
    with pytest.raises(NotImplementedError):
        learner.get_q_and_q_tot_table()


@pytest.mark.parametrize("name", ["2s3z", "matrix"])
def test_target_critic_follows_at_train_step_200(name):
    args, state, batch, mac, learner = build_product(name, "f32")
    assert args.target_update_cycle == 200
    before = learner.target_critic._flat.flat.clone()
    compare_update("central_v:%s/step200" % name, name, 0, learner, state, batch, 200, 0.8)
    assert torch.equal(learner.target_critic._flat.flat, learner._cflat.flat) and not torch.equal(before, learner._cflat.flat)
    for k, p in learner.target_critic.named_parameters():
        parity.close("central_v:%s/step200" % name, "target " + k, p.detach().cpu().numpy(), state.target_critic[k].numpy())


@pytest.mark.parametrize("lam", [0.0, 1.0])
def test_td_lambda_zero_and_one(lam):
    args, state, batch, mac, learner = build_product("2s3z", "f32", td_lambda=lam)
    for i in (0, 1):
        compare_update("central_v:2s3z lam=%g/step%d" % (lam, i), "2s3z", i, learner, state, batch, i, lam)


def test_td_lambda_none_is_zero_bit_for_bit():
    out = []
    for lam in (None, 0.0):
        args, state, batch, mac, learner = build_product("2s3z", "f32", td_lambda=lam)
        loss = learner.train(learners.clone_batch(batch(0)), 0, epsilon=po.EPS)
        out.append((loss, float(learner.actor_loss), learner._dbg["td_targets"].clone(), learner._flat.flat.clone(),
                    learner._cflat.flat.clone(), learner._flat.gradx.clone(), learner._cflat.gradx.clone()))
    assert out[0][:2] == out[1][:2]
    for x, y in zip(out[0][2:], out[1][2:]):
        assert torch.equal(x, y)


def test_refusals(monkeypatch):
    from marl_amd.algorithm import central_v, policy_learner
    from marl_amd.controller.share_params import PolicyMAC, SharedMAC
    args, _, _ = po.learner_case("2s3z")

    class Reducer:
        enabled = True
    mac = PolicyMAC(args)
    with monkeypatch.context() as m:
        m.setattr(policy_learner, "GradReducer", Reducer)    # the constructor is PolicyLearner's
        with pytest.raises(NotImplementedError):
            central_v.CentralVLearner(mac, args)
    assert not hasattr(mac.agent, "_flat")                # nothing was built
    for bad in (1.5, -0.1):
        args.td_lambda = bad
        with pytest.raises(ValueError):
            central_v.CentralVLearner(mac, args)
    assert not hasattr(mac.agent, "_flat")
    args.td_lambda = 0.8
    with pytest.raises(ValueError):
        central_v.CentralVLearner(SharedMAC(args), args)


# ---------------------------------------------------------------------------------------------------- the rollout
def _rollout_setup(E=8, T=120, seed=11):
    from marl_amd.controller.share_params import PolicyMAC, SharedMAC
    args = po.make_args("2s3z", T, seed=77, epsilon=0.3, anneal_epsilon=0.01, min_epsilon=0.02, epsilon_anneal_scale="episode")
    agent = seeded.seeded_state(seeded.agent_param_shapes(args), seed=seed)
    macs = []
    for cls in (PolicyMAC, SharedMAC):
        mac = cls(args)
        mac.agent.load_state_dict({k: torch.tensor(v) for k, v in agent.items()})
        mac.cuda()
        macs.append(mac)
    return args, agent, macs[0], macs[1]


def _env(args, E, T, fixed=False):
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    return SyntheticSMACEnv(E, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, T, seed=5, env0=2, fixed_length=fixed)


def test_sampling_rollout_vs_float64_policy():
    """The synthetic observations do not depend on the actions, so every step is checked on its own: the recorded observations
    and previous actions through the float64 agent, the float64 CDF, the sampler's restatement - under the exclusion rule and
    the cap of the kernel test"""
    from marl_amd.rollout import RolloutWorker
    from marl_amd.algorithm.central_v import CentralVLearner
    E, T = 8, 120
    args, agent, pmac, _ = _rollout_setup(E, T)
    env = _env(args, E, T)
    w = RolloutWorker(env, pmac, args)
    ep, rew, wins, steps = w.generate_episodes(E)
    eps_used = 0.3 - 0.01                              # the 'episode' scale: one anneal per rollout, in front of it
    assert w.epsilon == eps_used
    rec = ep.record
    N, A, H = args.n_agents, args.n_actions, args.rnn_hidden_dim
    u, length = rec.u.cpu().numpy().astype(np.int64), rec.length.cpu().numpy()
    obs, avail = rec.obs.cpu().numpy()[:, :T], rec.avail.cpu().numpy()[:, :T]
    live = np.arange(T)[None] < length[:, None]
    assert (u[~live] == -1).all() and (u[live] >= 0).all() and steps == int(length.sum())
    assert not ep["u"].cpu().numpy()[~live].any() and bool((rec.padded.cpu().numpy() == ~live).all())
    onehot = np.zeros((E, T, N, A))
    np.put_along_axis(onehot, np.maximum(u, 0)[..., None], (u >= 0)[..., None].astype(np.float64), axis=3)
    p64 = {k: torch.tensor(v, dtype=torch.float64) for k, v in agent.items()}
    with torch.no_grad():
        logits, _, _ = nets.agent_unroll(p64, torch.tensor(obs, dtype=torch.float64), nets.shifted_onehot(torch.tensor(onehot)),
                                         torch.zeros(E * N, H, dtype=torch.float64), True, True)
    logits = logits.numpy()
    near = total = 0
    for t in range(T):
        want, margin, _ = po.sample(logits[:, t], avail[:, t], live[:, t], eps_used, 77, env.env0, env.global_step(t))
        far = live[:, t, None] & (margin >= po.SAMPLER_EXCLUDE)
        assert (u[:, t][far] == want[far]).all(), t
        assert (np.take_along_axis(avail[:, t], np.maximum(u[:, t], 0)[..., None], -1)[live[:, t]] == 1).all()
        near += int((live[:, t, None] & ~far).sum())
        total += int(live[:, t].sum()) * N
    assert near < po.SAMPLER_CAP * total
    # the learner accepts the record as it is
    learner = CentralVLearner(pmac, args)
    assert np.isfinite(float(learner.train(ep, 0, epsilon=w.epsilon))) and np.isfinite(float(learner.actor_loss))


def test_evaluation_rollout_is_the_greedy_one_and_launch_episodes_refuses():
    from marl_amd.rollout import RolloutWorker
    E, T = 8, 120
    args, _, pmac, smac = _rollout_setup(E, T)
    recs = []
    for mac in (pmac, smac):
        w = RolloutWorker(_env(args, E, T), mac, args)
        ep, rew, wins, steps = w.generate_episodes(E, evaluate=True)
        assert w.epsilon == 0.3
        recs.append((ep.record, rew, wins, steps))
    for f in ("obs", "state", "avail", "u", "r", "term", "padded", "length", "won"):
        assert torch.equal(getattr(recs[0][0], f), getattr(recs[1][0], f)), f
    assert recs[0][1:] == recs[1][1:]
    w = RolloutWorker(_env(args, E, T), pmac, args)
    with pytest.raises(RuntimeError, match="stochastic"):
        w.launch_episodes()


# ---------------------------------------------------------------------------------------------------- the runner
def _runner(tmp_path, tag, argv=(), **over):
    from marl_amd.main import build
    from marl_amd.runner import Runner
    from marl_amd.utils.logging import Logger
    args, env = build(["--env", "matrix", "--alg", "central_v", "--n_envs", "64", "--n_steps", "320",
                       "--result_dir", str(tmp_path / (tag + "_res")), "--model_dir", str(tmp_path / (tag + "_model")),
                       "--evaluate_epoch", "64"] + list(argv))
    for k, v in over.items():
        setattr(args, k, v)
    torch.manual_seed(3)
    return args, env, (lambda: Runner(env, Logger(), args))


def test_runner_trains_on_policy(tmp_path):
    args, env, make = _runner(tmp_path, "a")
    r = make()
    a0, c0 = r.learner._flat.flat.clone(), r.learner._cflat.flat.clone()
    loss = r.run(0)
    assert r.buffer is None and r.train_steps == 5 == len(r.losses)                 # one update per rollout of 64 one-step episodes
    assert all(np.isfinite(float(x)) for x in r.losses) and np.isfinite(float(loss)) and np.isfinite(float(r.learner.actor_loss))
    assert not torch.equal(a0, r.learner._flat.flat) and not torch.equal(c0, r.learner._cflat.flat)
    np.testing.assert_allclose(r.rolloutWorker.epsilon, 0.5 - 5 * 0.00064, rtol=1e-12)      # one anneal per rollout
    assert len(r.eval_episode_rewards) >= 2                                                # evaluate() ran
    # model files
    r.learner.save_models(0)
    d = r.learner.model_dir
    for kind in ("rnn_net", "critic_net"):
        os.replace(d + "/0_%s_params.pkl" % kind, d + "/%s_params.pkl" % kind)
    args2, env2, make2 = _runner(tmp_path, "b")
    r2 = make2()
    assert not torch.equal(r2.learner._cflat.flat, r.learner._cflat.flat)
    r2.learner.model_dir = d
    r2.learner.load_models()
    assert torch.equal(r2.learner._flat.flat, r.learner._flat.flat) and torch.equal(r2.learner._cflat.flat, r.learner._cflat.flat)
    # full resume: the next iteration is the same, bit for bit
    ck = str(tmp_path / "resume.pt")
    r.save_resume(ck)
    args3, env3, make3 = _runner(tmp_path, "c", resume=ck)
    r3 = make3()
    assert (r3.train_steps, r3.rolloutWorker.epsilon, r3.env.episode) == (r.train_steps, r.rolloutWorker.epsilon, r.env.episode)
    for x in (r, r3):
        x.args.n_steps = x.time_steps + 1
        x.run(0)
    assert float(r.losses[-1]) == float(r3.losses[-1]) and len(r3.losses) == 1
    L, L3 = r.learner, r3.learner
    for a, b in ((L._flat.flat, L3._flat.flat), (L._cflat.flat, L3._cflat.flat), (L.target_critic._flat.flat, L3.target_critic._flat.flat),
                 (L.optimizer.s1, L3.optimizer.s1), (L.critic_optimizer.s1, L3.critic_optimizer.s1)):
        assert torch.equal(a, b)


def test_runner_refusals(tmp_path):
    args, env, make = _runner(tmp_path, "o", overlap_rollout=True)
    with pytest.raises(NotImplementedError):
        make()
    args, env, make = _runner(tmp_path, "w", world_model=True)
    with pytest.raises(ValueError):
        make()
    args, env, make = _runner(tmp_path, "c")
    args.alg = "coma"
    with pytest.raises(ValueError, match="learner coma cannot find!"):
        make()
