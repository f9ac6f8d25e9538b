"""World-model agent on the MI355X: the head kernels (csrc/world_head.hip) against the float64 oracle, the learner against the
reference fixtures and the oracle in both gemm modes, bitwise repeatability and graph replay, the untouched terminate_out,
checkpoints, rollouts, the Runner and the drop-in."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import seeded, learners
import parity
import world_oracle as wo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _t(d):
    return {k: torch.tensor(np.asarray(v)) for k, v in d.items()}


def build_product(case, gemm_mode=None):
    from marl_amd.controller.share_params import SharedMACWithState
    from marl_amd.algorithm.q_learner_state import QLearnerWithState
    args, agent, mixer = wo.case_states(case)
    args.cuda = True
    if gemm_mode is not None:
        args.gemm_mode = gemm_mode
    mac = SharedMACWithState(args)
    mac.agent.load_state_dict(_t(agent))
    learner = QLearnerWithState(mac, args)
    if mixer:
        learner.mixer.load_state_dict(_t(mixer))
        learner.target_mixer.load_state_dict(_t(mixer))
    return args, mac, learner


def named_product_params(learner):
    out = [("agent." + k, p) for k, p in learner.eval_net.agent.named_parameters()]
    return out + [("mixer." + k, p) for k, p in learner.mixer.named_parameters()]


# a parameter sample whose gradient is below this fraction of its tensor's largest sampled gradient is left to the norm check:
# RMSprop's first step moves it by lr * g / (0.1 |g| + 1e-8), so an fp32-level difference in g (world_qmix_2s3z samples an fc1
# entry at 2.5e-7 of the largest gradient) moves it by up to lr * 10 - a property of the update, not of the kernels
TINY_GRAD = 1e-5


def check_pins(fix, prefix, named, tol, case, scale=1.0, grad_prefix=None):
    """samples and norms of the pinned tensors; grad_prefix: the same step's gradient pins, whose near-zero entries (TINY_GRAD)
    are not compared one by one in the parameter samples"""
    names = sorted({k[len(prefix) + 1:].rsplit("/", 1)[0] for k in fix.files if k.startswith(prefix + "/")})
    assert names
    got = dict(named)
    for n in names:
        a = got[n].detach().cpu().numpy().astype(np.float64).ravel() * scale
        if "%s/%s/none" % (prefix, n) in fix.files:
            assert np.all(a == 0), n
            continue
        samp, ref = a[seeded.sample_indices(a.size)], fix["%s/%s/samp" % (prefix, n)]
        gkey = "%s/%s/samp" % (grad_prefix, n)
        if grad_prefix is not None and gkey in fix.files:
            g = np.abs(fix[gkey].astype(np.float64))
            keep = g >= TINY_GRAD * g.max()
            samp, ref = samp[keep], ref[keep]
        parity.close(case, prefix + "/" + n, samp, ref, tol=tol)
        parity.close(case, prefix + "/" + n + "/norm", np.sqrt((a * a).sum()), float(fix["%s/%s/norm" % (prefix, n)]), tol=tol)


# ---------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("shape", ["2s3z", "3s5z", "MMM2"])
def test_head_kernels_match_oracle(shape):
    """act and train forward, backward: B*T*N rows not a multiple of 16; o_next read from (T+1)-slot storage through an episode map
    with ragged lengths (steps t >= ep_len read as zeros)"""
    from marl_amd import ops
    from marl_amd.network.world_model import Agent
    args = seeded.make_args(shape, "qmix")
    N, O, A, H = args.n_agents, args.obs_shape, args.n_actions, 64
    B, T, E = 3, 7, 5
    R = B * T * N
    assert R % 16
    rng = np.random.default_rng(5)
    p = seeded.seeded_state(wo.world_param_shapes(args), seed=21)
    agent = Agent(O + A + N, args).to(DEV)
    agent.load_state_dict({**{k: v for k, v in agent.state_dict().items() if not k.startswith("world.")}, **_t(p)})
    w = agent.world_weights()
    h = rng.standard_normal((B, T, N, H)).astype(np.float32)
    store = rng.standard_normal((E, T + 1, N, O)).astype(np.float32)
    emap = np.array([4, 0, 2], dtype=np.int32)
    ep_len = np.array([7, 3, 5], dtype=np.int32)
    onext = np.zeros((B, T, N, O), np.float32)
    for b in range(B):
        onext[b, :ep_len[b]] = store[emap[b], 1:ep_len[b] + 1]
    r_ref, o_ref, t_ref = (x.numpy() for x in wo.head({k: torch.tensor(v, dtype=torch.float64) for k, v in p.items()},
                                                      torch.tensor(h, dtype=torch.float64)))
    hd = torch.tensor(h, device=DEV)
    q0 = rng.standard_normal((B, T, N, A)).astype(np.float32)
    q = torch.tensor(q0, device=DEV)
    r, oh, tau = (torch.full(s, 7.0, device=DEV) for s in ((B, T, N, A), (B, T, N, O), (B, T, N, 2)))
    ops.world_head_fwd(w, hd, q, B, T, N, O, A, r_out=r, ohat_out=oh, tau_out=tau)
    c = "world_head:%s" % shape
    parity.close(c, "r", r.cpu().numpy(), r_ref)
    parity.close(c, "o_hat", oh.cpu().numpy(), o_ref)
    parity.close(c, "tau", tau.cpu().numpy(), t_ref)
    parity.close(c, "q += r", q.cpu().numpy(), q0 + r_ref)
    loss = torch.full((2,), 1.5, device=DEV)
    sd = torch.tensor(store, device=DEV)
    kw = dict(obs=sd, obs_bs=(T + 1) * N, obs_t0=1, ep_len=torch.tensor(ep_len, device=DEV),
              ep_map=torch.tensor(emap, device=DEV))
    q1 = torch.tensor(q0, device=DEV)
    ops.world_head_fwd(w, hd, q1, B, T, N, O, A, loss=loss[0:1], **kw)
    parity.close(c, "train q", q1.cpu().numpy(), q0 + r_ref)
    parity.close(c, "loss", float(loss[0].item()) - 1.5, ((o_ref - onext) ** 2).sum())
    assert float(loss[1].item()) == 1.5
    # backward
    dq_idx = rng.integers(0, A, R).astype(np.int32)
    dq_val = rng.standard_normal(R).astype(np.float32)
    den, dscale = 3.0, 2.0 / (R * O)
    dr = np.zeros((R, A), np.float64)
    dr[np.arange(R), dq_idx] = dq_val
    dohat = dscale * den * (o_ref - onext)
    dh_ref, g_ref = wo.head_backward(p, h, dr.reshape(B, T, N, A), dohat)
    g = {k: torch.zeros_like(v) for k, v in agent.named_parameters() if k.startswith("world.")}
    dhs = torch.full((B, T, N, H), 7.0, device=DEV)
    ops.world_head_bwd(w, ops.world_grads(g), hd, torch.tensor(dq_idx, device=DEV), torch.tensor(dq_val, device=DEV),
                       sd, (T + 1) * N, 1, torch.tensor([den], device=DEV), dscale, dhs, B, T, N, O, A,
                       ep_len=kw["ep_len"], ep_map=kw["ep_map"])
    parity.close(c, "dhs", dhs.cpu().numpy(), dh_ref)
    for k, v in g.items():
        if k.startswith("world.terminate_out"):
            assert float(v.abs().max()) == 0.0
            continue
        parity.close(c, "grad " + k, v.cpu().numpy(), g_ref[k])
    # the reductions are reproducible: a second backward into fresh buffers gives the same bits
    g2 = {k: torch.zeros_like(v) for k, v in g.items()}
    dhs2 = torch.zeros_like(dhs)
    ops.world_head_bwd(w, ops.world_grads(g2), hd, torch.tensor(dq_idx, device=DEV), torch.tensor(dq_val, device=DEV),
                       sd, (T + 1) * N, 1, torch.tensor([den], device=DEV), dscale, dhs2, B, T, N, O, A,
                       ep_len=kw["ep_len"], ep_map=kw["ep_map"])
    assert torch.equal(dhs, dhs2) and all(torch.equal(g[k], g2[k]) for k in g)


# ---------------------------------------------------------------------------------------------------- the learner
@pytest.mark.parametrize("case", wo.CASES, ids=[c[0] for c in wo.CASES])
def test_forward_pieces_vs_reference(case, golden_dir, gemm_mode):
    name, shape, alg, B, T, lengths, over = case
    fix = np.load(os.path.join(golden_dir, name + ".npz"))
    args, mac, learner = build_product(case, gemm_mode)
    batch = seeded.make_batch(args, B, seed=100, lengths=lengths)
    mac.init_hidden(B)
    q, ret = mac.get_current_q_values(batch, T)
    c = "world_fwd:%s[%s]" % (name, gemm_mode)
    P = lambda key, t: parity.close(c, key, t.cpu().numpy(), fix[key])
    P("fwd/q_cur", q); P("fwd/h_cur", ret["ep_hidden_states"]); P("fwd/cur_r", ret["r"])
    P("fwd/cur_o_next", ret["o_next"]); P("fwd/cur_terminated", ret["terminated"])
    mac.init_hidden(B)
    q, ret = mac.get_next_q_values(batch, T)
    P("fwd/q_next", q); P("fwd/r_next", ret["r"])


@pytest.mark.parametrize("case", wo.CASES, ids=[c[0] for c in wo.CASES])
def test_train_steps_vs_reference_and_oracle(case, golden_dir, gemm_mode):
    name, shape, alg, B, T, lengths, over = case
    fix = np.load(os.path.join(golden_dir, name + ".npz"))
    args, mac, learner = build_product(case, gemm_mode)
    _, ost = wo.build_oracle_state(case)
    for i, ts in enumerate(wo.TRAIN_STEPS):
        batch = seeded.make_batch(args, B, seed=100 + i, lengths=lengths)
        loss = learner.train(learners.clone_batch(batch), ts)
        oloss, ograds, ointer = wo.train(ost, learners.clone_batch(batch), ts)
        rt = 1e-4 if i == 0 else 1e-3
        c = "world_train:%s[%s]/step%d" % (name, gemm_mode, ts)
        parity.close(c, "loss vs reference", loss, fix["losses"][i], tol=rt)
        parity.close(c, "loss vs oracle", loss, oloss, tol=rt)
        st = learner.last_stats.cpu().numpy()
        K = B * learner.max_episode_len * args.n_agents * args.obs_shape
        parity.close(c, "loss_pred", st[2] / K, fix["loss_pred"][i], tol=rt)
        assert learner.max_episode_len == ointer["T"]
        den = float(st[1])
        named = named_product_params(learner)
        if i <= 1:
            check_pins(fix, "step%d/grad" % i, [(n, p.grad) for n, p in named], rt, c, scale=1.0 / den)
            gn = float(torch.sqrt(learner.optimizer.sumsq[0]).item()) / den
            parity.close(c, "grad_norm", gn, float(fix["step%d/grad_norm" % i]), tol=rt)
            check_pins(fix, "step%d/param" % i, named, rt, c, grad_prefix="step%d/grad" % i)
        # the target network: synced to the eval network after step 200 (world.* included)
        check_pins(fix, "step%d/target_agent" % i,
                   [("agent." + k, p) for k, p in learner.target_net.agent.named_parameters()], 2e-3, c + "/target")


def test_get_q_and_q_tot_table(golden_dir):
    fix = np.load(os.path.join(golden_dir, "world_matrix_table.npz"))
    for alg in ("vdn", "qmix", "qplex"):
        args, mac, learner = build_product(("x", "matrix", alg, 1, 1, [1], {}))
        qt, qi, qj = learner.get_q_and_q_tot_table()
        np.testing.assert_allclose(qt, fix[alg + "/q_tot"], atol=1e-4, rtol=1e-4, err_msg=alg)
        np.testing.assert_allclose(qi, fix[alg + "/q_i"], atol=1e-4)
        np.testing.assert_allclose(qj, fix[alg + "/q_j"], atol=1e-4)


def test_large_shard_vs_oracle():
    """512 episodes x T = 120 of 2s3z (the fp32 unrolls' multi-tile and pair schedules): loss, loss_pred and gradient samples"""
    case = ("big", "2s3z", "qmix", 512, 120, None, {})
    args, mac, learner = build_product(case)
    _, ost = wo.build_oracle_state(case)
    rng = np.random.default_rng(1)
    lengths = [int(x) for x in rng.integers(60, 121, 512)]
    lengths[7] = -1
    batch = seeded.make_batch(args, 512, seed=400, lengths=lengths)
    loss = learner.train(learners.clone_batch(batch), 0)
    oloss, ograds, ointer = wo.train(ost, learners.clone_batch(batch), 0)
    c = "world_large"
    parity.close(c, "loss", loss, oloss)
    st = learner.last_stats.cpu().numpy()
    K = 512 * learner.max_episode_len * args.n_agents * args.obs_shape
    parity.close(c, "loss_pred", st[2] / K, float(ointer["loss_pred"].detach()))
    den = float(st[1])
    for n, p in named_product_params(learner):
        if n.startswith("agent.world.terminate_out"):
            continue
        a = p.grad.detach().cpu().numpy().ravel() / den
        ref = ograds[n].numpy().ravel()
        idx = seeded.sample_indices(a.size)
        parity.close(c, n, a[idx], ref[idx], scale=float(np.abs(ref).max()))


def _ring_learner(alg, mode, gemm_mode, E=96, T=12):
    import bench
    from marl_amd.controller.share_params import SharedMACWithState
    from marl_amd.algorithm.q_learner_state import QLearnerWithState
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    from marl_amd.common.replaybuffer import ReplayBuffer
    args = bench.make_args(alg, "2s3z", T)
    args.buffer_size, args.batch_size, args.hip_graph, args.gemm_mode = 2 * E, E, mode, gemm_mode
    torch.manual_seed(0)
    np.random.seed(7)
    mac = SharedMACWithState(args)
    learner = QLearnerWithState(mac, args)
    env = SyntheticSMACEnv(E, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, T, seed=3, fixed_length=True)
    w = RolloutWorker(env, mac, args)
    buf = ReplayBuffer(args)
    w.record_sink = buf
    return args, learner, w, buf


@pytest.mark.parametrize("alg,gemm_mode", [("qmix", "f32"), ("qplex", "f32"), ("qmix", "bf16x6")])
def test_graph_replay_and_repeats_give_the_same_bits(alg, gemm_mode):
    """eager vs hipGraph replay on the same ring samples: same losses and parameters bit for bit; terminate_out never moves"""
    E = 96
    out = {}
    for mode in (False, True):
        args, learner, w, buf = _ring_learner(alg, mode, gemm_mode, E)
        t0 = {k: v.detach().clone() for k, v in learner.eval_net.agent.world.terminate_out.named_parameters()}
        losses = []
        for i in range(8):
            buf.store_episode(w.generate_episodes(E)[0])
            losses.append(float(learner.train(buf.sample(E), i)))
        out[mode] = (losses, learner._flat.flat.detach().cpu().numpy().copy())
        for k, v in learner.eval_net.agent.world.terminate_out.named_parameters():
            assert torch.equal(v.detach(), t0[k]), k
        if mode:
            g = learner.graphs
            assert not g.disabled, getattr(g, "error", "")
            assert g.replays >= 3
    assert out[False][0] == out[True][0]
    np.testing.assert_array_equal(out[False][1], out[True][1])


def test_two_identical_updates_give_the_same_bits():
    case = wo.CASES[0]
    name, shape, alg, B, T, lengths, over = case
    res = []
    for _ in range(2):
        args, mac, learner = build_product(case)
        batch = seeded.make_batch(args, B, seed=100, lengths=lengths)
        loss = learner.train(learners.clone_batch(batch), 0)
        res.append((loss, learner._flat.flat.detach().cpu().numpy().copy(), learner._flat.gradx.detach().cpu().numpy().copy()))
    assert res[0][0] == res[1][0]
    np.testing.assert_array_equal(res[0][1], res[1][1])
    np.testing.assert_array_equal(res[0][2], res[1][2])


def test_save_load_roundtrip(tmp_path):
    case = wo.CASES[0]
    name, shape, alg, B, T, lengths, over = case
    args, mac, learner = build_product(case)
    args.model_dir = str(tmp_path)
    learner.model_dir = str(tmp_path) + "/" + args.alg + "/" + args.map
    batch = seeded.make_batch(args, B, seed=100, lengths=lengths)
    learner.train(learners.clone_batch(batch), 0)
    learner.save_models(0)
    sd = torch.load(learner.model_dir + "/0_rnn_net_params.pkl", map_location="cpu")
    assert len(sd) == 18 and "world.terminate_out.weight" in sd
    for kind in ("rnn_net", "mixer_net"):
        os.replace(learner.model_dir + "/0_%s_params.pkl" % kind, learner.model_dir + "/%s_params.pkl" % kind)
    args2, mac2, learner2 = build_product(case)
    learner2.model_dir = learner.model_dir
    learner2.load_models()
    assert torch.equal(learner2._flat.flat.cpu()[:learner.eval_net.agent._flat.n], learner.eval_net.agent._flat.flat.cpu())
    b2 = seeded.make_batch(args, B, seed=101, lengths=lengths)
    mac.init_hidden(B)
    mac2.init_hidden(B)
    assert torch.equal(mac.get_current_q_values(b2, T)[0], mac2.get_current_q_values(b2, T)[0])


@pytest.mark.parametrize("shape", ["2s3z", "MMM2"])
def test_batched_rollout_is_greedy_in_q_plus_r(shape):
    """a greedy batched rollout (per-step path with the act-mode head) picks argmax over the available actions of q + r as
    get_current_q_values computes it on the recorded episodes; the whole-rollout launch refuses the controller"""
    from marl_amd.controller.share_params import SharedMACWithState
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    T, E = 8, 37
    args = seeded.make_args(shape, "qmix", episode_limit=T)
    args.epsilon = 0.0
    agent = seeded.seeded_state(seeded.agent_param_shapes(args), seed=11, scale=3.0)
    agent.update(seeded.seeded_state(wo.world_param_shapes(args), seed=wo.WORLD_SEED, scale=3.0))
    mac = SharedMACWithState(args)
    mac.agent.load_state_dict(_t(agent))
    dims = (args.n_agents, args.obs_shape, args.state_shape, args.n_actions)
    for mode in ("whole", "fused_step", "unfused"):
        w = RolloutWorker(SyntheticSMACEnv(E, *dims, T, seed=5), mac, args)
        w.rollout_mode = mode
        ep = w.generate_episodes(E, evaluate=True)[0].numpy()
        mac.init_hidden(E)
        q, ret = mac.get_current_q_values(ep, T)
        q = q.cpu().numpy()
        q[np.asarray(ep["avail_u"]) == 0] = -np.inf
        live = np.asarray(ep["padded"])[..., 0] == 0
        u = np.asarray(ep["u"])[..., 0]
        assert np.array_equal(q.argmax(-1)[live], u[live]), mode
        with pytest.raises(RuntimeError):
            w.launch_episodes()


def _serial_mac(args):
    from marl_amd.controller.share_params import SharedMACWithState
    mac = SharedMACWithState(args)
    mac.agent.load_state_dict(_t(wo.serial_agent_state(args)))
    return mac


def test_serial_rollout_matches_reference_fixture(golden_dir):
    """the serial RolloutWorker loop with SharedMACWithState.choose_action (hidden state carried across steps, last action fed
    back, numpy draw order under epsilon) against the reference's own rollout"""
    from marl_amd.rollout import RolloutWorker
    from oracle import rollout as orl
    fx = np.load(os.path.join(golden_dir, "world_serial.npz"))
    for tag, eps, evaluate in (("greedy", 0.0, True), ("eps05", 0.5, False)):
        args = seeded.make_args("2s3z", "qmix", episode_limit=8)
        args.epsilon = eps
        w = RolloutWorker(orl.SerialSynthEnv(orl.SynthSMAC(5, 80, 120, 11, 8, seed=5)), _serial_mac(args), args)
        np.random.seed(9)
        ep, rew, wins, steps = w.generate_episodes(4, evaluate=evaluate)
        np.testing.assert_array_equal(np.asarray(ep["u"], dtype=np.float64), fx[tag + "/u"], err_msg=tag)
        for k in ("o", "r", "padded", "terminated", "avail_u", "avail_u_next"):
            np.testing.assert_allclose(np.asarray(ep[k], dtype=np.float64), fx[tag + "/" + k], atol=1e-6, err_msg=(tag, k))
        assert steps == int(fx[tag + "/steps"]) and list(wins) == list(fx[tag + "/wins"])
        np.testing.assert_allclose(rew, fx[tag + "/rewards"], atol=1e-5)
        np.testing.assert_allclose(w.epsilon, float(fx[tag + "/eps_after"]), rtol=1e-12)


@pytest.mark.parametrize("mode", ["whole", "fused_step", "unfused"])
def test_batched_rollout_matches_serial(mode):
    """greedy: the batched per-step rollout over E environments (act-mode head for every agent at once) plays the same
    episodes as E serial episodes of the reference-style loop (SerialSynthEnv's k-th reset is env slot k, episode 0)"""
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    from oracle import rollout as orl
    T, E = 8, 6
    args = seeded.make_args("2s3z", "qmix", episode_limit=T)
    args.epsilon = 0.0
    mac = _serial_mac(args)
    ws = RolloutWorker(orl.SerialSynthEnv(orl.SynthSMAC(5, 80, 120, 11, T, seed=5)), mac, args)
    np.random.seed(9)
    sep, srew, swins, ssteps = ws.generate_episodes(E, evaluate=True)
    wb = RolloutWorker(SyntheticSMACEnv(E, 5, 80, 120, 11, T, seed=5), mac, args)
    wb.rollout_mode = mode
    bep, brew, bwins, bsteps = wb.generate_episodes(E, evaluate=True)
    got = bep.numpy()
    np.testing.assert_array_equal(np.asarray(got["u"], dtype=np.float64), np.asarray(sep["u"], dtype=np.float64))
    for k in ("padded", "terminated", "avail_u"):
        np.testing.assert_array_equal(np.asarray(got[k], dtype=np.float64), np.asarray(sep[k], dtype=np.float64), err_msg=k)
    for k in ("o", "r"):
        np.testing.assert_allclose(np.asarray(got[k], dtype=np.float64), np.asarray(sep[k], dtype=np.float64), atol=1e-6, err_msg=k)
    assert bsteps == ssteps and list(bwins) == [bool(x) for x in swins]
    np.testing.assert_allclose(brew, srew, atol=1e-5)


def test_agent_forward_matches_oracle():
    """world_model.Agent.forward, the reference-shaped call (world_model.py:59-75): q = fc2(h) + r and the returns dict"""
    from marl_amd.network.world_model import Agent
    from oracle import nets
    args = seeded.make_args("MMM2", "qmix")
    I = args.obs_shape + args.n_actions + args.n_agents
    sd = seeded.seeded_state(seeded.agent_param_shapes(args), seed=11)
    sd.update(seeded.seeded_state(wo.world_param_shapes(args), seed=wo.WORLD_SEED))
    agent = Agent(I, args)
    agent.load_state_dict(_t(sd))
    rng = np.random.default_rng(3)
    rows = 37
    inp = rng.standard_normal((rows, I)).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((rows, 64))).astype(np.float32)
    q, ret = agent(torch.tensor(inp), torch.tensor(h0))
    p64 = {k: torch.tensor(v, dtype=torch.float64) for k, v in sd.items()}
    q_ref, h_ref = nets.agent_step(p64, torch.tensor(inp, dtype=torch.float64), torch.tensor(h0, dtype=torch.float64))
    r_ref, o_ref, t_ref = wo.head(p64, h_ref)
    c = "world_agent_forward"
    parity.close(c, "hidden_state", ret["hidden_state"].cpu().numpy(), h_ref.numpy())
    parity.close(c, "r", ret["r"].cpu().numpy(), r_ref.numpy())
    parity.close(c, "o_next", ret["o_next"].cpu().numpy(), o_ref.numpy())
    parity.close(c, "terminated", ret["terminated"].cpu().numpy(), t_ref.numpy())
    parity.close(c, "q", q.cpu().numpy(), (q_ref + r_ref).numpy())


def test_runner_trains_on_synthetic_env(tmp_path):
    from marl_amd.main import build
    from marl_amd.runner import Runner
    from marl_amd.utils.logging import Logger
    from marl_amd.controller.share_params import SharedMACWithState
    from marl_amd.algorithm.q_learner_state import QLearnerWithState
    args, env = build(["--alg", "qmix", "--map", "2s3z", "--n_envs", "16", "--world_model", "True", "--n_steps", "1200",
                       "--evaluate_cycle", "100000", "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "m")])
    runner = Runner(env, Logger(), args)
    assert isinstance(runner.mac, SharedMACWithState) and isinstance(runner.learner, QLearnerWithState)
    loss = runner.run(0)
    assert runner.train_steps > 0 and np.isfinite(float(loss))


def test_dropin_world_flow():
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin_world_flow.py")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MARL_N_ENVS="8")
    r = subprocess.run([sys.executable, "-m", "marl_amd.dropin", script], cwd=root, capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "world drop-in ok" in r.stdout
