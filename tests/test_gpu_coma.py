"""COMA on the MI355X: the kernels of csrc/coma.hip and COMALearner against tests/coma_oracle.py (float64, the critic over the
CONCATENATED input), the td_lambda settings, the entropy bonus, the refusals, checkpoints and resume, and the runner's on-policy loop.

Bounds: tests/parity.close at 1e-4 * max|ref| on every tensor.  The exceptions are the tensors whose FLOAT32 ORACLE already misses a
quarter of that (tests/test_coma_oracle_cpu.py measures it; DESIGN section 10 lists them): those alone are bounded by 4x their
float32-oracle error, coma_oracle.F32_EXCEPTIONS."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import learners
import coma_oracle as co
import parity
import policy_oracle as po

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def dev(x, dt=None):
    return torch.tensor(np.ascontiguousarray(x), device=DEV, dtype=dt)


# ---------------------------------------------------------------------------------------------------- the kernels
def run_fc1(c, B, T, N, A, S, O):
    """the critic's first layer and its backward as COMALearner composes them; returns h1, dpre, dsum, dW, db"""
    from marl_amd import ops
    D, K, C = co.FC1_D, c["W"].shape[1], 2 * N * A + N
    BT, R = B * T, B * T * N
    W, b, s, o, dh1 = (dev(c[k]) for k in ("W", "b", "s", "o", "dh1"))
    u = dev(c["u"]).reshape(-1)
    wt, pre_s, h1 = (torch.empty(n, D, device=DEV) for n in (C, BT, R))
    ops.coma_onehot_cols(W, S + O, wt, C, D)
    assert torch.equal(wt, W[:, S + O:].t().contiguous())
    ops.linear(ops.src(s), W[:, :S], b, pre_s, BT, D, S, ldw=K)
    ops.linear(ops.src(o), W[:, S:S + O], None, h1, R, D, O, ldw=K)
    ops.coma_fc1_fwd(pre_s, wt, u, h1, B, T, N, A, D)
    dW, db = torch.zeros(D, K, device=DEV), torch.zeros(D, device=DEV)
    dpre, dsum = torch.empty(R, D, device=DEV), torch.empty(BT, D, device=DEV)
    ops.coma_fc1_bwd(dh1, h1, u, dpre, dsum, dW, S + O, B, T, N, A, D)
    ops.linear_wgrad(dsum, ops.src(s), dW[:, :S], db, BT, D, S, lddw=K)
    ops.linear_wgrad(dpre, ops.src(o), dW[:, S:S + O], None, R, D, O, lddw=K)
    return dict(h1=h1, dpre=dpre, dsum=dsum, dW=dW, db=db)


@pytest.mark.parametrize("constant", [False, True])
@pytest.mark.parametrize("shape", co.FC1_SHAPES)
def test_fc1_forward_backward_vs_oracle(shape, constant):
    """the factored first layer against one Linear over the concatenated (R, K) input, forward and backward; an action nobody
    takes (exact zero columns); ``constant``: every agent takes action 1 at every step.  Two calls: equal bits"""
    B, T, N, A, S, O = shape
    c = co.fc1_case(B, T, N, A, S, O, co.FC1_SEED, constant)
    ref = co.fc1_reference(c, B, T, N, A)
    assert ref["near_zero"] == 0
    got = run_fc1(c, B, T, N, A, S, O)
    case = "coma_fc1:%s%s" % ("x".join(map(str, shape)), " const" if constant else "")
    for k in ("h1", "dpre", "dsum", "dW", "db"):
        parity.close(case, k, got[k].cpu().numpy(), ref[k])
    K0, g = S + O, got["dW"].cpu().numpy()
    for j in range(N):
        assert not g[:, K0 + j * A + A - 1].any() and not g[:, K0 + N * A + j * A + A - 1].any()
    if T == 1:
        assert not g[:, K0 + N * A:K0 + 2 * N * A].any()                 # one-step episodes: no last action
    again = run_fc1(c, B, T, N, A, S, O)
    for k in got:
        assert torch.equal(got[k], again[k]), k


def test_fc1_empty_shapes_and_bad_indices():
    from marl_amd import _lib
    lib = _lib.load()
    assert lib.marl_coma_fc1_fwd(None, None, None, None, 0, 5, 5, 11, 128, None) == 0
    assert lib.marl_coma_fc1_bwd(None, None, None, None, None, None, 0, 0, None, 0, 3, 0, 5, 11, 128, None) == 0
    assert lib.marl_coma_q_taken(None, None, None, 1, 3, 5, 0, 11, None) == 0
    assert lib.marl_coma_loss_bwd(*([None] * 6), 0.0, 0.0, *([None] * 9), 0, 1, 1, 1, None) == 0
    assert lib.marl_coma_onehot_cols(None, 0, 0, None, 0, 128, None) == 0
    # an index outside [0, A) is an all-zero one-hot on both sides
    B, T, N, A, S, O = co.FC1_SHAPES[0]
    c = co.fc1_case(B, T, N, A, S, O, co.FC1_SEED)
    c["u"][1, 2, 3] = -1
    c["u"][2, 0, 0] = A
    ref = co.fc1_reference(c, B, T, N, A)
    got = run_fc1(c, B, T, N, A, S, O)
    for k in ("h1", "dW"):
        parity.close("coma_fc1:bad index", k, got[k].cpu().numpy(), ref[k])


def run_loss(rows, B, T, N, A, eps, beta):
    from marl_amd import ops
    R = B * T * N
    z, a, q, G, padded = (dev(rows[k]) for k in ("logits", "avail", "q", "G", "padded"))
    u = dev(rows["u"])
    dz, dq = torch.full((R, A), 7.0, device=DEV), torch.full((R, A), 7.0, device=DEV)
    logp, ent, adv, qt = (torch.full((R,), 7.0, device=DEV) for _ in range(4))
    cs, ast = torch.zeros(2, device=DEV), torch.zeros(3, device=DEV)
    ops.coma_loss_bwd(z, a, q, u, G, padded, eps, beta, dz, dq, logp, ent, adv, qt, cs, ast, B, T, N, A)
    return dict(dlogits=dz, dq=dq, logp=logp, ent=ent, adv=adv, q_taken=qt, critic_stats=cs, actor_stats=ast)


@pytest.mark.parametrize("beta", co.BETAS)
@pytest.mark.parametrize("eps", [0.0, 0.3])
@pytest.mark.parametrize("B,T,N,A", [(4, 6, 5, 11), (23, 7, 10, 18), (5, 4, 3, 30)])
def test_loss_bwd_vs_oracle(B, T, N, A, eps, beta):
    """rows with one available action, padded steps with logits and Q of magnitude 1e6, whole rows shifted by +1e4; R = 120 (two
    tiles, the second partial), 1610 (seven workgroups) and A = 30 (the row-per-lane form).  Two calls: equal bits"""
    rows = co.kernel_case(B, T, N, A, seed=3)
    ref = co.loss_reference(rows, B, T, N, eps, beta)
    got = run_loss(rows, B, T, N, A, eps, beta)
    case = "coma_loss:%dx%dx%dx%d eps=%g beta=%g" % (B, T, N, A, eps, beta)
    for k in ("q_taken", "adv", "logp", "ent", "dlogits", "dq", "critic_stats", "actor_stats"):
        parity.close(case, k, got[k].cpu().numpy(), ref[k])
    assert float(got["critic_stats"][1]) == float(got["actor_stats"][1]) == ref["critic_stats"][1]
    pad = torch.tensor(rows["pad_rows"], device=DEV)
    for k in ("dlogits", "dq", "logp", "ent", "adv", "q_taken"):
        assert not got[k][pad].any(), k                                  # padded rows: exact zeros
    dq, u = got["dq"].cpu().numpy(), rows["u"].astype(np.int64)
    off = np.ones_like(dq, dtype=bool)
    off[np.arange(len(u)), u] = False
    assert not dq[off].any()                                             # exact zeros beside the taken action's column
    assert not got["adv"][torch.tensor(rows["one_rows"], device=DEV)].any()
    again = run_loss(rows, B, T, N, A, eps, beta)
    for k in got:
        assert torch.equal(got[k], again[k]), k


def test_loss_bwd_in_place():
    """dlogits over the logits and dq over q: the same bits as with separate outputs"""
    from marl_amd import ops
    B, T, N, A = 4, 6, 5, 11
    rows = co.kernel_case(B, T, N, A, seed=3)
    want = run_loss(rows, B, T, N, A, 0.3, 0.01)
    R = B * T * N
    z, a, q, G, padded, u = (dev(rows[k]) for k in ("logits", "avail", "q", "G", "padded", "u"))
    logp, ent, adv, qt = (torch.empty(R, device=DEV) for _ in range(4))
    cs, ast = torch.zeros(2, device=DEV), torch.zeros(3, device=DEV)
    ops.coma_loss_bwd(z, a, q, u, G, padded, 0.3, 0.01, z, q, logp, ent, adv, qt, cs, ast, B, T, N, A)
    assert torch.equal(z, want["dlogits"]) and torch.equal(q, want["dq"]) and torch.equal(cs, want["critic_stats"])


@pytest.mark.parametrize("B,T,N,A", [(4, 6, 5, 11), (9, 1, 2, 3), (7, 13, 10, 18)])
def test_q_taken_shift_and_zero_tail(B, T, N, A):
    from marl_amd import ops
    rng = np.random.default_rng(5)
    q = rng.standard_normal((B, T, N, A)).astype(np.float32)
    u = rng.integers(0, A, (B, T, N)).astype(np.int32)
    taken = np.take_along_axis(q, u[..., None].astype(np.int64), -1)[..., 0].transpose(0, 2, 1)      # (B, N, T)
    for shift in (0, 1, 2):
        out = torch.full((B, N, T), 7.0, device=DEV)
        ops.coma_q_taken(dev(q), dev(u).reshape(-1), out, shift, B, T, N, A)
        want = np.zeros((B, N, T), dtype=np.float32)
        if shift < T:
            want[:, :, :T - shift] = taken[:, :, shift:]
        assert np.array_equal(out.cpu().numpy(), want), shift


# ---------------------------------------------------------------------------------------------------- the learner
def build_product(name, gemm_mode=None, **over):
    """(args, oracle state, batch(i), controller, learner) of a learner case: the same seeded weights on both sides"""
    from marl_amd.controller.share_params import PolicyMAC
    from marl_amd.algorithm.coma import COMALearner
    args, state, batch = co.learner_case(name, **over)
    if gemm_mode is not None:
        args.gemm_mode = gemm_mode
    t = lambda d: {k: x.detach().to(torch.float32) for k, x in d.items()}
    mac = PolicyMAC(args)
    mac.agent.load_state_dict(t(state.agent))
    learner = COMALearner(mac, args)
    learner.critic.load_state_dict(t(state.critic))
    learner.target_critic.load_state_dict(t(state.critic))
    return args, state, batch, mac, learner


def named_params(learner):
    return [("agent." + k, p) for k, p in learner.eval_net.agent.named_parameters()] + \
           [("critic." + k, p) for k, p in learner.critic.named_parameters()]


def bounded(c, key, name, got, ref):
    """parity.close, or 4x the float32-oracle error for the tensors coma_oracle.F32_EXCEPTIONS lists"""
    exc = co.F32_EXCEPTIONS.get(key)
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
    loss = learner.train(learners.clone_batch(b), train_step, epsilon=co.EPS)
    lc, la, ograds, inter = co.train(state, learners.clone_batch(b), train_step, co.EPS, lam, beta)
    assert co.relu_near_zero(inter) == 0
    T, N, A = inter["T"], args.n_agents, args.n_actions
    B = inter["mask"].shape[0]
    assert learner.max_episode_len == T
    d = learner._dbg
    assert set(d) == {"logits", "q", "q_taken", "q_next", "td_targets", "adv", "logp", "dlogits", "ent"}
    mask = inter["mask"].numpy()[:, :, None]
    key = lambda k: (name, 0.0 if lam is None else lam, beta, "step%d/%s" % (i, k))
    n = lambda k: inter[k].detach().numpy()
    parity.close(c, "Q", d["q"].view(B, T, N, A).cpu().numpy(), n("q"))
    parity.close(c, "q_taken", d["q_taken"].view(B, T, N).cpu().numpy(), n("q_taken"))
    parity.close(c, "q_next", d["q_next"].view(B, N, T).cpu().numpy(), n("q_next"))
    G = d["td_targets"].view(B, N, T).permute(0, 2, 1).cpu().numpy()
    parity.close(c, "G", G * mask, n("td_targets") * mask)                      # (a padded step's G is not part of any loss)
    parity.close(c, "Adv", d["adv"].view(B, T, N).cpu().numpy() * mask, n("adv") * mask)
    parity.close(c, "logp", d["logp"].view(B, T, N).cpu().numpy(), n("logp"))
    bounded(c, key("l_critic"), "L_critic", float(loss), lc)
    bounded(c, key("l_actor"), "L_actor", float(learner.actor_loss), la)
    if beta != 0.0:
        parity.close(c, "ent", d["ent"].view(B, T, N).cpu().numpy(), n("ent"))
        parity.close(c, "entropy", float(learner.entropy), float(inter["entropy"].detach()))
    den = float(inter["den"])
    assert float(learner.actor_stats[1].item()) == den == float(learner.last_stats[1].item()) == N * float(inter["M"])
    for pn, p in named_params(learner):
        bounded(c, key("grad " + pn), "grad " + pn, p.grad.detach().cpu().numpy() / den, ograds[pn].detach().numpy())
    for half, opt in (("agent.", learner.optimizer), ("critic.", learner.critic_optimizer)):
        norm = float(torch.sqrt(opt.sumsq[0]).item()) / den
        bounded(c, key(half + "grad_norm"), half + "grad_norm", norm, inter[half + "grad_norm"])
        bounded(c, key(half + "clip_coef"), half + "clip_coef", min(1.0, args.grad_norm_clip / (norm + 1e-6)), inter[half + "clip_coef"])
    oparams = dict([("agent." + k, x) for k, x in state.agent.items()] + [("critic." + k, x) for k, x in state.critic.items()])
    for pn, p in named_params(learner):
        bounded(c, key("param " + pn), "param " + pn, p.detach().cpu().numpy(), oparams[pn].detach().numpy())
    return inter


@pytest.mark.parametrize("name,gemm_mode", [("2s3z", "f32"), ("2s3z", "bf16x6"), ("MMM2", "f32"), ("matrix", "f32")])
def test_two_updates_vs_oracle(name, gemm_mode):
    """2s3z: ragged, one episode of length 1, one unterminated and cut at max_episode_len (no bootstrap), unavailable actions"""
    args, state, batch, mac, learner = build_product(name, gemm_mode)
    init_critic = learner._cflat.flat.clone()
    for i in (0, 1):
        inter = compare_update("coma:%s[%s]/step%d" % (name, gemm_mode, i), name, i, learner, state, batch, i, 0.8)
        if name == "2s3z":
            assert inter["T"] == 5 < args.episode_limit and float(inter["M"]) == 1 + 5 + 4 + 5
            assert not learner._dbg["q_next"].view(4, 5, 5)[:, :, 4].any()
    assert torch.equal(learner.target_critic._flat.flat, init_critic)      # no sync at train_step 0 and 1
    with pytest.raises(NotImplementedError):
        learner.get_q_and_q_tot_table()


@pytest.mark.parametrize("name", ["2s3z", "matrix"])
def test_target_critic_follows_at_train_step_200(name):
    args, state, batch, mac, learner = build_product(name, "f32")
    assert args.target_update_cycle == 200
    before = learner.target_critic._flat.flat.clone()
    compare_update("coma:%s/step200" % name, name, 0, learner, state, batch, 200, 0.8)
    assert torch.equal(learner.target_critic._flat.flat, learner._cflat.flat) and not torch.equal(before, learner._cflat.flat)
    for k, p in learner.target_critic.named_parameters():
        bounded("coma:%s/step200" % name, (name, 0.8, 0.0, "step0/param critic." + k), "target " + k, p.detach().cpu().numpy(),
                state.target_critic[k].numpy())


@pytest.mark.parametrize("lam", [0.0, 1.0])
def test_td_lambda_zero_and_one(lam):
    args, state, batch, mac, learner = build_product("2s3z", "f32", td_lambda=lam)
    for i in (0, 1):
        compare_update("coma:2s3z lam=%g/step%d" % (lam, i), "2s3z", i, learner, state, batch, i, lam)


def test_td_lambda_none_is_zero_bit_for_bit():
    out = []
    for lam in (None, 0.0):
        args, state, batch, mac, learner = build_product("2s3z", "f32", td_lambda=lam)
        loss = learner.train(learners.clone_batch(batch(0)), 0, epsilon=co.EPS)
        out.append((loss, float(learner.actor_loss), learner._dbg["td_targets"].clone(), learner._flat.flat.clone(),
                    learner._cflat.flat.clone(), learner._flat.gradx.clone(), learner._cflat.gradx.clone()))
    assert out[0][:2] == out[1][:2]
    for x, y in zip(out[0][2:], out[1][2:]):
        assert torch.equal(x, y)


def test_entropy_bonus_vs_oracle():
    beta = 0.01
    args, state, batch, mac, learner = build_product("2s3z", "f32", policy_entropy_coef=beta)
    assert learner.beta == beta
    for i in (0, 1):
        compare_update("coma+H:2s3z/step%d" % i, "2s3z", i, learner, state, batch, i, 0.8, beta)


def test_refusals(monkeypatch):
    from marl_amd.algorithm import coma, policy_learner
    from marl_amd.controller.share_params import PolicyMAC, SharedMAC
    args, _, _ = co.learner_case("2s3z")

    class Reducer:
        enabled = True
    mac = PolicyMAC(args)
    with monkeypatch.context() as m:
        m.setattr(policy_learner, "GradReducer", Reducer)   # COMALearner's constructor is PolicyLearner's
        with pytest.raises(NotImplementedError):
            coma.COMALearner(mac, args)
    assert not hasattr(mac.agent, "_flat")                # nothing was built
    for field, bad in (("td_lambda", 1.5), ("td_lambda", -0.1), ("policy_entropy_coef", -0.01)):
        keep = getattr(args, field)
        setattr(args, field, bad)
        with pytest.raises(ValueError):
            coma.COMALearner(mac, args)
        setattr(args, field, keep)
    assert not hasattr(mac.agent, "_flat")
    with pytest.raises(ValueError):
        coma.COMALearner(SharedMAC(args), args)


def test_checkpoints_and_resume_state(tmp_path):
    from marl_amd.algorithm.central_v import CentralVLearner
    from marl_amd.controller.share_params import PolicyMAC
    args, state, batch, mac, learner = build_product("2s3z", "f32", model_dir=str(tmp_path / "model"))
    learner.train(learners.clone_batch(batch(0)), 0, epsilon=co.EPS)
    # model files: the published layout
    learner.save_models(0)
    d = learner.model_dir
    assert sorted(os.listdir(d)) == ["0_critic_net_params.pkl", "0_rnn_net_params.pkl"]
    sd = torch.load(d + "/0_critic_net_params.pkl")
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == co.critic_param_shapes(args)
    for kind in ("rnn_net", "critic_net"):
        os.replace(d + "/0_%s_params.pkl" % kind, d + "/%s_params.pkl" % kind)
    args2, _, _, _, other = build_product("2s3z", "f32", model_dir=str(tmp_path / "model"))
    assert not torch.equal(other._cflat.flat, learner._cflat.flat)
    other.load_models()
    assert torch.equal(other._flat.flat, learner._flat.flat) and torch.equal(other._cflat.flat, learner._cflat.flat)
    # resume state: the next update is the same, bit for bit
    rs = learner.resume_state()
    assert rs["alg"] == "coma"
    args3, _, _, _, third = build_product("2s3z", "f32")
    third.load_resume_state(rs)
    losses = [x.train(learners.clone_batch(batch(1)), 1, epsilon=co.EPS) for x in (learner, third)]
    assert float(losses[0]) == float(losses[1]) and float(learner.actor_loss) == float(third.actor_loss)
    for a, b in ((learner._flat.flat, third._flat.flat), (learner._cflat.flat, third._cflat.flat),
                 (learner.target_critic._flat.flat, third.target_critic._flat.flat), (learner.optimizer.s1, third.optimizer.s1),
                 (learner.critic_optimizer.s1, third.critic_optimizer.s1)):
        assert torch.equal(a, b)
    # a central-V resume state is refused (another alg, another critic)
    cargs, _, _ = po.learner_case("2s3z")
    cv = CentralVLearner(PolicyMAC(cargs), cargs)
    with pytest.raises(ValueError):
        third.load_resume_state(cv.resume_state())
    with pytest.raises(ValueError):
        cv.load_resume_state(rs)


# ---------------------------------------------------------------------------------------------------- the runner
def _build(tmp_path, tag, argv):
    from marl_amd.main import build
    return build(list(argv) + ["--alg", "coma", "--result_dir", str(tmp_path / (tag + "_res")),
                               "--model_dir", str(tmp_path / (tag + "_model"))])


def _matrix_payoff(learner):
    st = types.SimpleNamespace(args=learner.args, dtype=torch.float64,
                               agent={k: p.detach().double().cpu() for k, p in learner.eval_net.agent.named_parameters()})
    return po.matrix_expectations(*po.matrix_policy(st))[0]


def test_runner_matrix_game_payoff_does_not_fall(tmp_path):
    """--env matrix --alg coma --n_envs 64 for 640 steps = ten on-policy updates: finite losses, and the exact expected payoff of
    the policy (eps = 0) is not below the initial one.  Ten, not five: the advantage comes from a critic that starts at random, so
    the first few updates may move the policy either way; in the float64 oracle, on sampled batches of 64 episodes from six
    different initialisations, the payoff was above its start from the tenth update on in every run (gains of 0.04 to 0.26)."""
    from marl_amd.algorithm.coma import COMALearner
    from marl_amd.main import make_runner
    args, env = _build(tmp_path, "m", ["--env", "matrix", "--n_envs", "64", "--n_steps", "640", "--evaluate_epoch", "64"])
    torch.manual_seed(3)
    r = make_runner(args, env)
    assert isinstance(r.learner, COMALearner) and r.buffer is None and args.td_lambda == 0.8
    pay0 = _matrix_payoff(r.learner)
    loss = r.run(0)
    assert r.train_steps == 10 == len(r.losses)
    assert all(np.isfinite(float(x)) for x in r.losses) and np.isfinite(float(loss)) and np.isfinite(float(r.learner.actor_loss))
    pay1 = _matrix_payoff(r.learner)
    print("matrix game: expected payoff %.4f -> %.4f" % (pay0, pay1))
    assert pay1 >= pay0, (pay0, pay1)


def test_runner_2s3z_one_on_policy_update(tmp_path):
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    from marl_amd.main import make_runner
    args, _ = _build(tmp_path, "s", ["--map", "2s3z", "--n_envs", "8", "--n_steps", "1", "--evaluate_epoch", "8"])
    args.episode_limit = 6
    env = SyntheticSMACEnv(8, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, 6, seed=args.seed)
    torch.manual_seed(3)
    r = make_runner(args, env)
    a0, c0 = r.learner._flat.flat.clone(), r.learner._cflat.flat.clone()
    loss = r.run(0)
    assert r.train_steps == 1 and np.isfinite(float(loss)) and np.isfinite(float(r.learner.actor_loss))
    assert not torch.equal(a0, r.learner._flat.flat) and not torch.equal(c0, r.learner._cflat.flat)
    with pytest.raises(NotImplementedError):
        r.learner.get_q_and_q_tot_table()


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
    with pytest.raises(ValueError, match="learner coma cannot find!"):
        Runner(env, Logger(), args)
