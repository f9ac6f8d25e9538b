"""MAIC on the MI355X: the message head (csrc/maic_head.hip) against the float64 oracle and the reference fixtures, the gate's
zero pattern, bitwise repeatability, rollouts (greedy, serial, exploring), checkpoints, the Runner and the drop-in."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import parity
import maic_oracle as mo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
MODES = [(True, False), (True, True), (False, False), (False, True)]      # (test_mode, batch statistics)
MODE_IDS = ["test_eval", "test_batch", "samp_eval", "samp_batch"]


def _t(d):
    return {k: torch.tensor(np.asarray(v)) for k, v in d.items()}


def _agent(args, seed=mo.MAIC_SEED, scale=3.0):
    from marl_amd.network.maic import MAICAgent
    agent = MAICAgent(args.obs_shape + args.n_actions + args.n_agents, args)
    agent.load_state_dict(_t(mo.maic_state(args, seed=seed, scale=scale)), strict=True)
    return agent


def _mac(args, seed=mo.MAIC_SEED, train=False):
    from marl_amd.controller.share_params import MAICMAC
    mac = MAICMAC(args)
    mac.agent.load_state_dict(_t(mo.maic_state(args, seed=seed)), strict=True)
    mac.agent.train(train)
    return mac


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape,bs", [("2s3z", 37), ("3s5z", 37), ("MMM2", 37), ("matrix", 37), ("2s3z", 1), ("MMM2", 2)])
def test_head_kernel_matches_oracle(shape, bs, mode):
    """rows not a multiple of 16 and a last workgroup that is partly filled (2s3z: 3 envs per tile, 37 = 12 * 3 + 1; 3s5z: 2
    per tile; matrix: 8 per tile), every optional output, all four mode combinations"""
    from marl_amd import ops
    test_mode, bn_batch = mode
    args = mo.maic_args(shape)
    N, A, NL = args.n_agents, args.n_actions, args.n_agents * mo.L
    state = mo.maic_state(args, seed=5)
    rng = np.random.default_rng(3)
    R = bs * N
    h = rng.standard_normal((R, 64)).astype(np.float32) * 0.5
    q = rng.standard_normal((R, A)).astype(np.float32)
    eps = rng.standard_normal((R, NL)).astype(np.float32)
    dev = {k: v.to(DEV).contiguous() for k, v in _t(state).items()}
    w = ops.maic_weights(dev)
    qd = torch.tensor(q, device=DEV)
    outs = dict(mean_out=torch.full((R, NL), np.nan, device=DEV), var_out=torch.full((R, NL), np.nan, device=DEV),
                lat_out=torch.full((R, NL), np.nan, device=DEV), alpha_out=torch.full((R, N), np.nan, device=DEV),
                msg_out=torch.full((R * N, A), np.nan, device=DEV))
    ops.maic_head_fwd(w, torch.tensor(h, device=DEV), qd, bs, N, A, test_mode=test_mode, bn_batch=bn_batch,
                      eps=None if test_mode else torch.tensor(eps, device=DEV), **outs)
    ref = mo.head(mo.p64(state), torch.tensor(h, dtype=torch.float64), torch.tensor(q, dtype=torch.float64), bs, N, test_mode,
                  bn_batch, torch.tensor(eps, dtype=torch.float64))
    c = "maic_head_%s_bs%d_%s" % (shape, bs, MODE_IDS[MODES.index(mode)])
    parity.close(c, "mean", outs["mean_out"].cpu().numpy(), ref["mean"].numpy())
    parity.close(c, "var", outs["var_out"].cpu().numpy(), ref["var"].numpy())
    parity.close(c, "latent", outs["lat_out"].cpu().numpy(), ref["latent"].numpy())
    parity.close(c, "alpha", outs["alpha_out"].cpu().numpy().reshape(bs, N, N), ref["alpha"].numpy())
    parity.close(c, "msg", outs["msg_out"].cpu().numpy().reshape(bs, N, N, A), ref["msg"].numpy())
    parity.close(c, "return_q", qd.cpu().numpy(), ref["return_q"].numpy())
    rm, rv = dev[mo.BN + "running_mean"].cpu().numpy(), dev[mo.BN + "running_var"].cpu().numpy()
    parity.close(c, "running_mean", rm, ref["running_mean"].numpy())
    parity.close(c, "running_var", rv, ref["running_var"].numpy())
    assert int(dev[mo.BN + "num_batches_tracked"]) == ref["num_batches_tracked"]
    # without the optional outputs: the same q, bit for bit
    dev2 = {k: v.to(DEV).contiguous() for k, v in _t(state).items()}
    q2 = torch.tensor(q, device=DEV)
    ops.maic_head_fwd(ops.maic_weights(dev2), torch.tensor(h, device=DEV), q2, bs, N, A, test_mode=test_mode, bn_batch=bn_batch,
                      eps=None if test_mode else torch.tensor(eps, device=DEV))
    assert torch.equal(q2, qd)


def test_unsupported_shapes_raise_before_any_launch():
    from marl_amd import ops
    h, q = torch.zeros(17, 64, device=DEV), torch.zeros(17, 11, device=DEV)
    with pytest.raises(ValueError):
        ops.maic_head_fwd(None, h, q, 1, 17, 11)
    with pytest.raises(ValueError):
        ops.maic_head_fwd(None, h, q, 1, 5, 33)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", ["2s3z", "MMM2"])
def test_forward_vs_reference_fixture(shape, mode, golden_dir, gemm_mode):
    """MAICAgent.forward against what the reference computed, the gate's zero pattern and the running statistics"""
    test_mode, bn_batch = mode
    tag = MODE_IDS[MODES.index(mode)]
    fi = np.load(os.path.join(golden_dir, "maic_%s_inputs.npz" % shape))
    fx = np.load(os.path.join(golden_dir, "maic_%s_%s.npz" % (shape, tag)))
    args = mo.maic_args(shape)
    args.gemm_mode = gemm_mode
    N, A = args.n_agents, args.n_actions
    bs = fi["inputs"].shape[0] // N
    agent = _agent(args, seed=int(fi["seed"]))
    agent.train(bn_batch)
    kw = {} if test_mode else {"eps": torch.tensor(fx["eps"], device=DEV)}
    q, h, ret = agent(torch.tensor(fi["inputs"]), torch.tensor(fi["h0"]), bs, test_mode=test_mode, **kw)
    assert ret == {}
    c = "maic_forward_%s_%s_%s" % (shape, tag, gemm_mode)
    parity.close(c, "h", h.cpu().numpy(), fi["h"])
    parity.close(c, "return_q", q.cpu().numpy(), fx["return_q"])
    bn = agent.embed_net[1]
    parity.close(c, "running_mean", bn.running_mean.cpu().numpy(), fx["running_mean"])
    parity.close(c, "running_var", bn.running_var.cpu().numpy(), fx["running_var"])
    assert int(bn.num_batches_tracked) == int(fx["num_batches_tracked"])
    # the head's pieces from the agent's own h
    q0 = torch.zeros(bs * N, A, device=DEV)
    agent2 = _agent(args, seed=int(fi["seed"]))
    agent2.train(bn_batch)
    alpha, lat, msg = torch.empty(bs * N, N, device=DEV), torch.empty(bs * N, N * mo.L, device=DEV), torch.empty(bs * N * N, A, device=DEV)
    agent2.weights()
    agent2.head(h, q0, bs, test_mode, kw.get("eps"), alpha_out=alpha, lat_out=lat, msg_out=msg)
    parity.close(c, "latent", lat.cpu().numpy(), fx["latent"])
    parity.close(c, "alpha", alpha.cpu().numpy().reshape(bs, N, N), fx["alpha"])
    parity.close(c, "msg", msg.cpu().numpy().reshape(bs, N, N, A), fx["msg"])
    if test_mode:
        assert np.array_equal(alpha.cpu().numpy().reshape(bs, N, N) == 0, fx["alpha"] == 0)


def _episodes(args, B, T, seed=4):
    from oracle import seeded
    return seeded.make_batch(args, B, seed, dtype=np.float32, full_length=True)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "batch"])
@pytest.mark.parametrize("shape", ["2s3z", "MMM2"])
def test_get_current_q_values_vs_oracle(shape, train, gemm_mode):
    """the unroll then the head: one head call over all B*T environments in eval mode, one per transition index in
    batch-statistics mode (the running statistics move T times)"""
    from oracle import nets
    T, B = 4, 7
    args = mo.maic_args(shape, episode_limit=T)
    args.gemm_mode = gemm_mode
    N, A = args.n_agents, args.n_actions
    mac = _mac(args, train=train)
    batch = _episodes(args, B, T)
    mac.init_hidden(B)
    q, hs, ret = mac.get_current_q_values(batch, T, test_mode=True)
    p = mo.p64(mo.maic_state(args))
    h = torch.zeros(B * N, 64, dtype=torch.float64)
    o = torch.tensor(np.asarray(batch["o"]), dtype=torch.float64)
    uo = torch.tensor(np.asarray(batch["u_onehot"]), dtype=torch.float64)
    ref = np.zeros((B, T, N, A))
    for t in range(T):
        last = uo[:, t - 1] if t > 0 else torch.zeros_like(uo[:, 0])
        inp = torch.tensor(mo.step_inputs(args, o[:, t].numpy(), last.numpy()))
        out = mo.forward(p, inp, h, B, N, True, train)
        h = out["h"]
        if train:
            p[mo.BN + "running_mean"], p[mo.BN + "running_var"] = out["running_mean"], out["running_var"]
        ref[:, t] = out["return_q"].numpy().reshape(B, N, A)
    c = "maic_mac_q_%s_%s_%s" % (shape, "batch" if train else "eval", gemm_mode)
    parity.close(c, "q", q.cpu().numpy(), ref)
    bn = mac.agent.embed_net[1]
    parity.close(c, "running_mean", bn.running_mean.cpu().numpy(), p[mo.BN + "running_mean"].numpy())
    assert int(bn.num_batches_tracked) == 3 + (T if train else 0)
    qn, _, _ = mac.get_next_q_values(batch, T, test_mode=True)
    assert qn.shape == q.shape and torch.isfinite(qn).all()


@pytest.mark.parametrize("train", [False, True], ids=["eval", "batch"])
def test_two_identical_calls_give_the_same_bits(train):
    args = mo.maic_args("MMM2")
    N, A, bs = args.n_agents, args.n_actions, 333
    g = torch.Generator().manual_seed(1)
    x = torch.randn(bs * N, args.obs_shape + A + N, generator=g)
    h0 = torch.randn(bs * N, 64, generator=g) * 0.5
    eps = torch.randn(bs * N, N * mo.L, generator=g).to(DEV)
    res = []
    for _ in range(2):
        agent = _agent(args)
        agent.train(train)
        for test_mode in (True, False):
            q, h, _ = agent(x, h0, bs, test_mode=test_mode, eps=eps)
            res.append(q.clone())
        res.append(agent.embed_net[1].running_var.clone())
    for a, b in zip(res[:3], res[3:]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("shape", ["2s3z", "MMM2"])
def test_batched_rollout_is_greedy_in_the_message_q(shape):
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    T, E = 8, 37
    args = mo.maic_args(shape, episode_limit=T)
    args.epsilon = 0.0
    mac = _mac(args)
    dims = (args.n_agents, args.obs_shape, args.state_shape, args.n_actions)
    recs = []
    for mode in ("whole", "fused_step", "unfused"):
        w = RolloutWorker(SyntheticSMACEnv(E, *dims, T, seed=5), mac, args)
        w.rollout_mode = mode
        ep = w.generate_episodes(E, evaluate=True)[0].numpy()
        mac.init_hidden(E)
        q = mac.get_current_q_values(ep, T, test_mode=True)[0].cpu().numpy()
        q[np.asarray(ep["avail_u"]) == 0] = -np.inf
        live = np.asarray(ep["padded"])[..., 0] == 0
        u = np.asarray(ep["u"])[..., 0]
        assert np.array_equal(q.argmax(-1)[live], u[live]), mode
        with pytest.raises(RuntimeError):
            w.launch_episodes()
        recs.append(ep)
    for k in recs[0]:
        assert np.array_equal(recs[0][k], recs[1][k]) and np.array_equal(recs[0][k], recs[2][k]), k


def _serial_worker(args, mac, T):
    from marl_amd.rollout import RolloutWorker
    from oracle import rollout as orl
    return RolloutWorker(orl.SerialSynthEnv(orl.SynthSMAC(5, 80, 120, 11, T, seed=5)), mac, args)


def test_serial_rollout_matches_reference_fixture(golden_dir):
    fx = np.load(os.path.join(golden_dir, "maic_serial.npz"))
    args = mo.maic_args("2s3z", episode_limit=8)
    args.epsilon = 0.0
    mac = _mac(args, seed=int(fx["seed"]))
    np.random.seed(9)
    ep, rew, wins, steps = _serial_worker(args, mac, 8).generate_episodes(6, evaluate=True)
    np.testing.assert_array_equal(np.asarray(ep["u"], dtype=np.float64), fx["u"])
    for k in ("padded", "terminated", "avail_u"):
        np.testing.assert_array_equal(np.asarray(ep[k], dtype=np.float64), fx[k], err_msg=k)
    for k in ("o", "r"):
        np.testing.assert_allclose(np.asarray(ep[k], dtype=np.float64), fx[k], atol=1e-6, err_msg=k)
    assert steps == int(fx["steps"]) and list(wins) == list(fx["wins"])
    np.testing.assert_allclose(rew, fx["rewards"], atol=1e-5)


@pytest.mark.parametrize("mode", ["whole", "fused_step", "unfused"])
def test_batched_rollout_matches_serial_in_eval_mode(mode, golden_dir):
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    fx = np.load(os.path.join(golden_dir, "maic_serial.npz"))
    T, E = 8, 6
    args = mo.maic_args("2s3z", episode_limit=T)
    args.epsilon = 0.0
    mac = _mac(args, seed=int(fx["seed"]))
    wb = RolloutWorker(SyntheticSMACEnv(E, 5, 80, 120, 11, T, seed=5), mac, args)
    wb.rollout_mode = mode
    bep, brew, bwins, bsteps = wb.generate_episodes(E, evaluate=True)
    got = bep.numpy()
    np.testing.assert_array_equal(np.asarray(got["u"], dtype=np.float64), fx["u"])
    for k in ("padded", "terminated", "avail_u"):
        np.testing.assert_array_equal(np.asarray(got[k], dtype=np.float64), fx[k], err_msg=k)
    for k in ("o", "r"):
        np.testing.assert_allclose(np.asarray(got[k], dtype=np.float64), fx[k], atol=1e-6, err_msg=k)
    assert bsteps == int(fx["steps"]) and list(bwins) == [bool(x) for x in fx["wins"]]
    np.testing.assert_allclose(brew, fx["rewards"], atol=1e-5)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "batch"])
def test_exploring_rollout_reproduces_the_hash_noise(train):
    """epsilon 0.5, sampled latents: the actions of the batched rollout equal the oracle's, which restates the hash-drawn
    noise (stream 8, Box-Muller) and the epsilon-greedy draws"""
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    from oracle import rollout as orl
    T, E = 8, 23
    args = mo.maic_args("2s3z", episode_limit=T)
    args.epsilon, args.anneal_epsilon, args.seed = 0.5, 0.0, 77
    mac = _mac(args, train=train)
    w = RolloutWorker(SyntheticSMACEnv(E, 5, 80, 120, 11, T, seed=5), mac, args)
    w.rollout_mode = "fused_step"
    ep = w.generate_episodes(E, evaluate=False)[0].numpy()
    u_ref, pad_ref = mo.batched_rollout(mo.maic_state(args), args, orl.SynthSMAC(5, 80, 120, 11, T, seed=5), E, 0.5, False,
                                        rseed=77, bn_train=train)
    np.testing.assert_array_equal(np.asarray(ep["padded"])[..., 0], pad_ref)
    live = pad_ref == 0
    np.testing.assert_array_equal(np.asarray(ep["u"])[..., 0][live], u_ref[live])


def test_noise_kernel_matches_restatement():
    from marl_amd import ops
    E, N = 9, 10
    eps = torch.empty(E * N, N * mo.L, device=DEV)
    ops.maic_noise(77, 3, 1234, eps, E, N)
    ref = mo.hash_noise(77, 3 + np.arange(E), np.full(E, 1234), N).reshape(E * N, -1)
    np.testing.assert_allclose(eps.cpu().numpy(), ref, atol=2e-6, rtol=2e-6)


def test_save_load_roundtrip_deepcopy_and_load_state(tmp_path):
    T, B = 3, 5
    args = mo.maic_args("2s3z", episode_limit=T)
    mac = _mac(args, train=True)
    batch = _episodes(args, B, T)
    mac.init_hidden(B)
    mac.get_current_q_values(batch, T, test_mode=True)          # moves the running statistics
    mac.agent.eval()
    path = str(tmp_path / "rnn_net_params.pkl")
    mac.save_models(path)
    sd = torch.load(path, map_location="cpu")
    assert list(sd.keys()) == [k for k, _ in mo.key_shapes(args)]
    mac2 = _mac(args, seed=9)
    mac2.load_models(path)
    mac3 = copy.deepcopy(mac)
    mac4 = _mac(args, seed=10)
    mac4.cuda()
    mac4.load_state(mac)
    ref = None
    for m in (mac, mac2, mac3, mac4):
        m.agent.eval()
        m.init_hidden(B)
        q = m.get_current_q_values(batch, T, test_mode=True)[0]
        ref = q if ref is None else ref
        assert torch.equal(q, ref)


def test_runner_evaluates_a_saved_model_and_refuses_training(tmp_path):
    from marl_amd.main import build
    from marl_amd.runner import Runner
    from marl_amd.utils.logging import Logger
    from marl_amd.controller.share_params import MAICMAC
    from marl_amd.algorithm.maic_q_learner import MAICQLearner
    common = ["--alg", "qmix", "--map", "2s3z", "--n_envs", "16", "--MAIC", "True", "--evaluate_epoch", "1",
              "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "m")]
    args, env = build(common)
    runner = Runner(env, Logger(), args)
    assert isinstance(runner.mac, MAICMAC) and isinstance(runner.learner, MAICQLearner)
    before = runner.learner._flat.flat.clone()
    ep = runner.rolloutWorker.generate_episodes(16)[0]
    with pytest.raises(NotImplementedError):
        runner.learner.train(ep, 0)
    assert torch.equal(runner.learner._flat.flat, before)
    runner.learner.save_models(0)
    mdir = tmp_path / "m" / "qmix" / "2s3z"
    os.rename(mdir / "0_rnn_net_params.pkl", mdir / "rnn_net_params.pkl")
    os.rename(mdir / "0_mixer_net_params.pkl", mdir / "mixer_net_params.pkl")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "marl_amd.main"] + common + ["--load_model", "True", "--evaluate", "True"],
                       cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "The win rate of qmix is" in r.stdout


def test_dropin_maic_flow():
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin_maic_flow.py")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "marl_amd.dropin", script], cwd=root, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, MARL_N_ENVS="8"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "MAIC drop-in ok" in r.stdout
