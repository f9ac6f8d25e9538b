"""RTW inference on the MI355X: the reflection head kernels (csrc/rtw_head.hip) against the reference's outputs for the
shipped QMIX model and against the torch oracle (tests/rtw_oracle.py) at every configuration shape, the serial and batched
RTW rollouts, the Runner's evaluation of the shipped model, and RTWQLearner.train's TypeError."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import seeded, rollout as orl
import parity
import rtw_oracle

pytestmark = pytest.mark.gpu


def _args(shape, T, not_self=True, **over):
    a = seeded.make_args(shape, "qmix", episode_limit=T, **over)
    a.RTW = True
    a.world_loss_weight, a.teammate_loss_weight, a.hidden_dim, a.attn_dim = 1, 1, 64, 64
    a.not_self_model = not_self
    return a


def _model_dir(tmp_path, golden_dir):
    d = tmp_path / "model" / "qmix" / "2s3z"
    d.mkdir(parents=True)
    for f in ("rnn_net_params.pkl", "mixer_net_params.pkl"):
        shutil.copyfile(os.path.join(golden_dir, "ref_ckpt", "qmix_rtw", f), str(d / f))
    return str(tmp_path / "model")


def _learner(args, tmp_path, golden_dir):
    from marl_amd.controller.share_params import RTWMAC
    from marl_amd.algorithm.rtw_q_learner import RTWQLearner
    args.model_dir = _model_dir(tmp_path, golden_dir)
    mac = RTWMAC(args)
    learner = RTWQLearner(mac, None, args)
    learner.load_models()
    return mac, learner


def _act(agent, inp, h0, obs, avail, N, O, A, not_self):
    """unroll rows (as RNNQNet.forward) + act head with the optional outputs"""
    from marl_amd import ops
    dev = torch.device("cuda")
    G = avail.shape[0]
    from marl_amd.network.q_network import RNNQNet
    q, h = RNNQNet.forward(agent, torch.tensor(inp, device=dev).reshape(G * N, -1), torch.tensor(h0, device=dev).reshape(G * N, 64))
    a_out = torch.full((G * N, N), -7, dtype=torch.int32, device=dev)
    ohat = torch.zeros(G * N, O, device=dev)
    ops.rtw_head_act(agent.rtw_weights(), h, torch.tensor(obs, device=dev).reshape(G * N, O).contiguous(), N, 0,
                     torch.tensor(avail, device=dev).contiguous(), N, 0, q, G, N, O, A, not_self, a_out=a_out, ohat_out=ohat)
    return q.cpu().numpy(), h.cpu().numpy(), a_out.cpu().numpy(), ohat.cpu().numpy()


@pytest.mark.parametrize("tag,not_self", [("self0", True), ("self1", False)])
def test_shipped_model_matches_reference(tmp_path, golden_dir, tag, not_self):
    fx = np.load(os.path.join(golden_dir, "rtw_2s3z_ckpt.npz"))
    args = _args("2s3z", 5, not_self)
    mac, learner = _learner(args, tmp_path, golden_dir)
    case = "rtw_ckpt_" + tag
    pre = tag + "/act/"
    q, h, a, ohat = _act(mac.agent, fx[pre + "inp"], fx[pre + "h0"], fx[pre + "obs"], fx[pre + "avail"], 5, 80, 11, not_self)
    parity.close(case, "act/h", h, fx[pre + "h"])
    parity.close(case, "act/q", q, fx[pre + "q"])
    parity.close(case, "act/ohat", ohat, fx[pre + "ohat"])
    np.testing.assert_array_equal(a, fx[pre + "act"])
    # the controller's own act path, one row at a time (RTWAgent.forward test_mode=True)
    G = fx[pre + "inp"].shape[0]
    for g, i in ((0, 0), (G - 1, 4)):
        qq, hh = mac.agent(torch.tensor(fx[pre + "inp"][g, i:i + 1]), torch.tensor(fx[pre + "h0"][g, i:i + 1]),
                           torch.tensor(fx[pre + "obs"][g, i:i + 1]), None, None, torch.tensor(fx[pre + "avail"][g:g + 1]),
                           test_mode=True, agent_num=i)
        parity.close(case, "forward/q", qq.cpu().numpy()[0], fx[pre + "q"][g * 5 + i])
    pre = tag + "/given/"
    batch = seeded.make_batch(args, 3, seed=700, lengths=[5, 3, -1])
    mac.init_hidden(3)
    q, hs, l1, l2 = mac.get_current_q_values(batch, 5)
    parity.close(case, "given/q", q.cpu().numpy(), fx[pre + "q"])
    parity.close(case, "given/h", hs.cpu().numpy(), fx[pre + "h"])
    assert l1 == 0.0 and l2 == 0.0 and isinstance(l1, float)


@pytest.mark.parametrize("shape", ["2s3z", "3s5z", "MMM2", "matrix"])
@pytest.mark.parametrize("E", [37, 512, 4096])
@pytest.mark.parametrize("not_self", [True, False])
def test_head_kernels_match_oracle(shape, E, not_self):
    from marl_amd import ops
    from marl_amd.network.rtw import RTWAgent
    args = _args(shape, 4, not_self)
    N, O, A = args.n_agents, args.obs_shape, args.n_actions
    assert ops.rtw_supported(N, O, A)
    sd = rtw_oracle.random_rtw_params(args, 3)
    p = rtw_oracle.params_t(sd)
    agent = RTWAgent(O + A + N, args)
    agent.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    agent.cuda()
    w = agent.rtw_weights()
    rng = np.random.default_rng(E + N)
    dev = torch.device("cuda")
    case = "rtw_head_%s_%d_%s" % (shape, E, "ns" if not_self else "self")
    # act mode, reading slot t = 2 of (T+1)-slot storage as the rollout does
    T = 3
    h = torch.tensor(rng.standard_normal((E * N, 64)).astype(np.float32))
    obs = torch.tensor(rng.standard_normal((E, T + 1, N, O)).astype(np.float32))
    avail = torch.tensor((rng.random((E, T + 1, N, A)) < 0.6).astype(np.float32))
    avail[..., 0] = 1.0
    q0 = torch.tensor(rng.standard_normal((E * N, A)).astype(np.float32))
    qr, ohat, a, gap = rtw_oracle.act_head(p, h, obs[:, 2].reshape(E * N, O), avail[:, 2], N, not_self)
    q = q0.to(dev)
    a_out = torch.full((E * N, N), -7, dtype=torch.int32, device=dev)
    oh = torch.zeros(E * N, O, device=dev)
    ops.rtw_head_act(w, h.to(dev), obs.to(dev), (T + 1) * N, 2, avail.to(dev), (T + 1) * N, 2, q, E, N, O, A, not_self,
                     a_out=a_out, ohat_out=oh)
    sure = gap.numpy() > 1e-5
    np.testing.assert_array_equal(a_out.cpu().numpy()[sure], a.numpy()[sure])
    assert sure.mean() > 0.99
    rows = sure.all(1)          # rows whose teammate actions are all unambiguous feed the same one-hot blocks
    parity.close(case, "act/ohat", oh.cpu().numpy()[rows], ohat.numpy()[rows])
    parity.close(case, "act/q", q.cpu().numpy()[rows], (q0 + qr).numpy()[rows])
    # given mode over B episodes x T steps: o at t0 = 0 and o_next at t0 = 1 of the same storage, u with u_t0 = 0
    B = max(1, E // T)
    hs = torch.tensor(rng.standard_normal((B, T, N, 64)).astype(np.float32))
    ob = torch.tensor(rng.standard_normal((B, T + 1, N, O)).astype(np.float32))
    u = torch.tensor(rng.integers(-1, A, (B, T, N)).astype(np.int32))
    qg0 = torch.tensor(rng.standard_normal((B, T, N, A)).astype(np.float32))
    qgr = rtw_oracle.given_head(p, hs.reshape(-1, 64), ob[:, :T].reshape(-1, O), ob[:, 1:].reshape(-1, O), u.reshape(-1), N,
                                not_self)
    qg = qg0.to(dev)
    obd = ob.to(dev)
    ops.rtw_head_given(w, hs.to(dev), obd, (T + 1) * N, 0, obd, (T + 1) * N, 1, u.to(dev), T * N, 0, qg, B, T, N, O, A,
                       not_self)
    parity.close(case, "given/q", qg.cpu().numpy(), (qg0 + qgr.view(B, T, N, A)).numpy())


def test_serial_rollout_matches_reference_fixture(tmp_path, golden_dir):
    from marl_amd.rollout import RolloutWorker
    fx = np.load(os.path.join(golden_dir, "rtw_serial.npz"))
    for tag, eps, evaluate in (("greedy", 0.0, True), ("eps05", 0.5, False)):
        args = _args("2s3z", 8, epsilon=eps)
        mac, _ = _learner(args, tmp_path / tag, golden_dir)
        sy = orl.SynthSMAC(5, 80, 120, 11, 8, seed=5)
        w = RolloutWorker(orl.SerialSynthEnv(sy), mac, args)
        np.random.seed(9)
        ep, rew, wins, steps = w.generate_episodes(4, evaluate=evaluate)
        np.testing.assert_array_equal(np.asarray(ep["u"], dtype=np.float64), fx[tag + "/u"])
        for k in ("o", "r", "padded", "terminated", "avail_u", "avail_u_next"):
            np.testing.assert_allclose(np.asarray(ep[k], dtype=np.float64), fx[tag + "/" + k], atol=1e-6, err_msg=k)
        assert steps == int(fx[tag + "/steps"]) and list(wins) == list(fx[tag + "/wins"])
        np.testing.assert_allclose(rew, fx[tag + "/rewards"], atol=1e-5)
        np.testing.assert_allclose(w.epsilon, float(fx[tag + "/eps_after"]), rtol=1e-12)


def _seeded_rtw_mac(args, seed=11):
    from marl_amd.controller.share_params import RTWMAC
    sd = rtw_oracle.random_rtw_params(args, seed)
    mac = RTWMAC(args)
    mac.agent.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    mac.cuda()
    return mac, sd


@pytest.mark.parametrize("shape,E", [("2s3z", 37), ("MMM2", 29)])
@pytest.mark.parametrize("eps,evaluate", [(0.0, True), (0.5, False)])
def test_batched_rollout_matches_oracle(shape, E, eps, evaluate):
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    T = 8
    args = _args(shape, T, epsilon=eps, seed=77)
    args.anneal_epsilon = 0.01
    dims = (args.n_agents, args.obs_shape, args.state_shape, args.n_actions)
    mac, sd = _seeded_rtw_mac(args)
    sy = orl.SynthSMAC(*dims, T, seed=5)
    oep, orew, owins, osteps, oeps = rtw_oracle.batched_rtw_rollout(sd, args, sy, E, eps, evaluate=evaluate, rseed=77, env0=2)
    for mode in ("whole", "fused_step", "unfused"):      # "whole" is the default request: RTW takes the per-step path
        w = RolloutWorker(SyntheticSMACEnv(E, *dims, T, seed=5, env0=2), mac, args)
        w.rollout_mode = mode
        ep, rew, wins, steps = w.generate_episodes(E, evaluate=evaluate)
        got = ep.numpy()
        for k in ("u", "padded", "terminated", "avail_u", "avail_u_next", "u_onehot"):
            np.testing.assert_array_equal(got[k], np.asarray(oep[k], dtype=got[k].dtype), err_msg=(mode, k))
        for k in ("o", "o_next", "s", "s_next", "r"):
            np.testing.assert_allclose(got[k], oep[k], atol=1e-6, err_msg=(mode, k))
        assert steps == osteps and list(wins) == [bool(x) for x in owins]
        np.testing.assert_allclose(rew, orew, atol=1e-5)
        np.testing.assert_allclose(w.epsilon, oeps if not evaluate else eps, rtol=1e-12)
        with pytest.raises(RuntimeError):
            w.launch_episodes()


def test_host_vector_env_matches_device_env():
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    from marl_amd.env.host_vector import HostVectorEnv
    T, E, env0 = 8, 13, 2
    args = _args("2s3z", T, epsilon=0.5, seed=77)
    args.anneal_epsilon = 0.01
    mac, _ = _seeded_rtw_mac(args)
    sy = orl.SynthSMAC(5, 80, 120, 11, T, seed=5)
    wh = RolloutWorker(HostVectorEnv([orl.SerialSynthEnv(sy, env_id=env0 + i) for i in range(E)], seed=5, env0=env0), mac, args)
    wd = RolloutWorker(SyntheticSMACEnv(E, 5, 80, 120, 11, T, seed=5, env0=env0), mac, args)
    for evaluate in (True, False):
        eh, rh, winh, sh = wh.generate_episodes(E, evaluate=evaluate)
        ed, rd, wind, sd_ = wd.generate_episodes(E, evaluate=evaluate)
        for f in ("u", "r", "term", "padded", "length", "won", "avail"):
            assert torch.equal(getattr(eh.record, f), getattr(ed.record, f)), f
        assert sh == sd_ and list(winh) == list(wind)


def test_runner_evaluates_shipped_model(tmp_path, golden_dir):
    from marl_amd.main import build
    from marl_amd.runner import Runner
    from marl_amd.utils.logging import Logger
    from marl_amd.controller.share_params import RTWMAC
    from marl_amd.algorithm.rtw_q_learner import RTWQLearner
    model_dir = _model_dir(tmp_path, golden_dir)
    args, env = build(["--alg", "qmix", "--map", "2s3z", "--n_envs", "16", "--RTW", "True", "--load_model", "True",
                       "--evaluate_epoch", "16", "--result_dir", str(tmp_path / "res"), "--model_dir", model_dir])
    runner = Runner(env, Logger(), args)
    assert isinstance(runner.mac, RTWMAC) and isinstance(runner.learner, RTWQLearner)
    win_rate, reward = runner.evaluate()
    sd = torch.load(os.path.join(golden_dir, "ref_ckpt", "qmix_rtw", "rnn_net_params.pkl"), map_location="cpu")
    sy = orl.SynthSMAC(5, 80, 120, 11, args.episode_limit, seed=args.seed)
    _, orew, owins, _, _ = rtw_oracle.batched_rtw_rollout({k: v.numpy() for k, v in sd.items()}, args, sy, 16, 0.0,
                                                          evaluate=True, rseed=args.seed)
    assert win_rate == sum(owins) / 16
    np.testing.assert_allclose(reward, sum(orew) / 16, atol=1e-4)


def test_train_raises_and_changes_nothing(tmp_path, golden_dir):
    args = _args("2s3z", 5)
    mac, learner = _learner(args, tmp_path, golden_dir)
    flat = learner._flat.flat.clone()
    tgt = learner.target_net.agent._flat.flat.clone()
    s1 = learner.optimizer.s1.clone()
    batch = seeded.make_batch(args, 3, seed=700, lengths=[5, 3, -1])
    with pytest.raises(TypeError):
        learner.train(batch, 0)
    with pytest.raises(TypeError):
        mac.get_next_q_values(batch, 5)
    assert torch.equal(flat, learner._flat.flat) and torch.equal(tgt, learner.target_net.agent._flat.flat)
    assert torch.equal(s1, learner.optimizer.s1) and learner.optimizer.t == 0


def test_dropin_resolves_rtw_modules():
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin_rtw_flow.py")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "marl_amd.dropin", script], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "RTW drop-in ok" in r.stdout
