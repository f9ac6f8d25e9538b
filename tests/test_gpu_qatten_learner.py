"""QattenMixer and QLearner(alg='qatten') on the MI355X against tests/qatten_oracle.py.  Needs a real MI355X: ``pytest -m gpu``.

Module level: hip_forward / hip_backward and hip_loss_backward against autograd of the unfolded float64 ``mix`` - q_tot, dq and every
parameter's .grad, parity.close at 1e-4 * max|ref| - with ``no_fused`` set and without.  Learner level: three updates beside the
oracle learner at the batch shape of the IQL learner test, with the bounds of tests/test_gpu_learners.py (1e-4 for the loss, the
gradients and the parameters of the first update, 1e-3 for the later ones): with the loss fold and with no_loss_fold, with and without
double-Q, on TD(lambda) returns, in both gemm modes; the target sync, hipGraph replay from a replay ring, and the launcher."""
import numpy as np
import pytest
import torch

from oracle import seeded, learners
import qatten_oracle as qo
import parity

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _mixer(args, seed=5, no_fused=False):
    from marl_amd.network.mixer import QattenMixer
    from marl_amd.hostutil import flatten_module
    m = QattenMixer(args)
    P = seeded.seeded_state(qo.param_shapes(args), seed=seed)
    m.load_state_dict({k: torch.tensor(x) for k, x in P.items()})
    if no_fused:
        m.no_fused = True
    m.to(DEV)
    flatten_module(m, DEV, with_grad=True)
    return m, {k: torch.tensor(x, dtype=torch.float64, requires_grad=True) for k, x in P.items()}


@pytest.mark.parametrize("no_fused", [True, False])
@pytest.mark.parametrize("name, R", [("2s3z", 65), ("MMM2", 33)])
def test_module_against_autograd_of_the_unfolded_mix(name, R, no_fused):
    args = seeded.make_args(name, "qatten")
    m, P = _mixer(args, no_fused=no_fused)
    N, S = args.n_agents, args.state_shape
    g = np.random.default_rng(R)
    q, s, gin, q_tgt, r = (g.standard_normal(shape).astype(np.float32) for shape in ((R, N), (R, S), (R,), (R,), (R,)))
    rr = np.arange(R)
    padded, term = (rr % 5 == 4).astype(np.float32), (rr % 7 == 6).astype(np.float32)
    t64 = lambda x: torch.tensor(x, dtype=torch.float64)
    up = lambda x: torch.tensor(x, device=DEV)
    qd, sd = up(q), up(s)
    case = "qatten_module:%s[no_fused=%s]" % (name, no_fused)
    # forward + backward from a given gradient
    q64 = t64(q).requires_grad_(True)
    ref = qo.mix(P, q64, t64(s), args)
    names = list(P)
    grads = torch.autograd.grad((ref * t64(gin)).sum(), [q64] + [P[k] for k in names], retain_graph=True)
    ctx = {}
    m._flat.zero_grad()
    q_tot = m.hip_forward(qd, sd, R, ctx=ctx)
    parity.close(case, "q_tot", q_tot.cpu().numpy(), ref.detach().numpy())
    dq = m.hip_backward(ctx, up(gin), R)
    parity.close(case, "dq", dq.cpu().numpy(), grads[0].numpy())
    for k, gref in zip(names, grads[1:]):
        parity.close(case, "grad " + k, dict(m.named_parameters())[k].grad.cpu().numpy(), gref.numpy())
    # forward(): the nn.Module face
    parity.close(case, "forward", m(torch.tensor(q).view(1, R, N), torch.tensor(s).view(1, R, S)).cpu().numpy().reshape(R), ref.detach().numpy())
    # loss-folded
    mask = 1.0 - t64(padded)
    L = ((mask * (t64(r) + qo.GAMMA * t64(q_tgt) * (1 - t64(term)) - ref)) ** 2).sum()
    grads = torch.autograd.grad(L, [q64] + [P[k] for k in names])
    m._flat.zero_grad()
    loss2 = torch.zeros(2, device=DEV)
    q_tot2 = torch.empty(R, device=DEV)
    assert m.loss_backward_fused(sd)
    dq = m.hip_loss_backward(qd, sd, R, up(q_tgt), up(r), up(term), up(padded), qo.GAMMA, loss2, q_tot=q_tot2)
    assert torch.equal(q_tot2, q_tot)
    parity.close(case, "loss num", float(loss2[0]), float(L.detach()))
    assert float(loss2[1]) == float(mask.sum())
    parity.close(case, "loss dq", dq.cpu().numpy(), grads[0].numpy())
    for k, gref in zip(names, grads[1:]):
        parity.close(case, "loss grad " + k, dict(m.named_parameters())[k].grad.cpu().numpy(), gref.numpy())


def build_product(args, gemm_mode=None):
    from marl_amd.controller.share_params import SharedMAC
    from marl_amd.algorithm.q_learner import QLearner
    from marl_amd.network.mixer import QattenMixer
    args.cuda = True
    if gemm_mode is not None:
        args.gemm_mode = gemm_mode
    mac = SharedMAC(args)
    t = lambda d: {k: torch.tensor(x) for k, x in d.items()}
    mac.agent.load_state_dict(t(seeded.seeded_state(seeded.agent_param_shapes(args), seed=qo.AGENT_SEED)))
    learner = QLearner(mac, args)
    assert type(learner.mixer) is QattenMixer and type(learner.target_mixer) is QattenMixer
    mixer = t(seeded.seeded_state(qo.param_shapes(args), seed=qo.MIXER_SEED))
    learner.mixer.load_state_dict(mixer)
    learner.target_mixer.load_state_dict(mixer)
    return mac, learner


def three_updates(case, gemm_mode, **more):
    args, st, batch_of, lam = qo.learner_case(case, **more)
    _, learner = build_product(qo.learner_case(case, **more)[0], gemm_mode)
    for i, tol in enumerate(qo.LEARNER_TOL):
        batch = batch_of(i)
        loss = learner.train(learners.clone_batch(batch), i)
        oloss, ograds, ointer = qo.train(st, learners.clone_batch(batch), i, lam=lam)
        c = "qatten_train:%s%s[%s]/step%d" % (case, sorted(more.items()) or "", gemm_mode, i)
        assert learner.max_episode_len == ointer["T"]
        parity.close(c, "loss", loss, oloss, tol=tol)
        den = float(learner.last_stats[1].item())
        assert den == float(ointer["den"])
        got = [("agent." + k, p) for k, p in learner.eval_net.agent.named_parameters()] + \
              [("mixer." + k, p) for k, p in learner.mixer.named_parameters()]
        ref = dict(st.named_params())
        assert [k for k, _ in got] == list(ref)
        for n, p in got:
            if i == 0:
                parity.close(c, "grad " + n, p.grad.detach().cpu().numpy() / den, ograds[n].numpy(), tol=tol)
            parity.close(c, "param " + n, p.detach().cpu().numpy(), ref[n].detach().numpy(), tol=tol)
    return learner, st


def test_three_updates_vs_oracle(gemm_mode):
    three_updates("double_q", gemm_mode)


def test_three_updates_without_the_loss_fold(gemm_mode):
    learner, _ = three_updates("double_q", gemm_mode, no_loss_fold=True)
    folded, _ = three_updates("double_q", gemm_mode)
    # the fold gives the composition's gradients bit for bit; only the loss sums are added in another order
    for (n, a), (_, b) in zip(learner.mixer.named_parameters(), folded.mixer.named_parameters()):
        parity.close("qatten fold vs no fold[%s]" % gemm_mode, n, a.detach().cpu().numpy(), b.detach().cpu().numpy(), tol=1e-4)


def test_three_updates_without_double_q(gemm_mode):
    three_updates("max", gemm_mode)


def test_three_updates_on_lambda_returns(gemm_mode):
    three_updates("lam0.8", gemm_mode)


def test_target_sync_fires_at_target_update_cycle():
    args, _, batch_of, _ = qo.learner_case("double_q", target_update_cycle=2)
    _, learner = build_product(args)
    tgt = learner.target_mixer._flat.flat
    start = tgt.clone()
    now = lambda: torch.cat([p.detach().reshape(-1) for p in learner.mixer.parameters()])
    then = lambda: torch.cat([p.detach().reshape(-1) for p in learner.target_mixer.parameters()])
    assert torch.equal(now(), then())
    for i in range(3):
        assert np.isfinite(learner.train(learners.clone_batch(batch_of(i)), i))
        if i < 2:
            assert torch.equal(tgt, start) and not torch.equal(now(), then()), i
        else:
            assert torch.equal(now(), then()) and not torch.equal(tgt, start)


def _ring_run(mode, updates):
    """tests/test_gpu_edges.py:test_hip_graph_replay_equals_eager's loop with the Qatten mixer"""
    import bench
    from marl_amd.controller.share_params import SharedMAC
    from marl_amd.algorithm.q_learner import QLearner
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    from marl_amd.common.replaybuffer import ReplayBuffer
    args = bench.make_args("qatten", "2s3z", 12)
    E = 96
    args.buffer_size, args.batch_size, args.hip_graph = 2 * E, E, mode
    torch.manual_seed(0)
    np.random.seed(7)
    mac = SharedMAC(args)
    learner = QLearner(mac, args)
    env = SyntheticSMACEnv(E, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, 12, seed=3, fixed_length=True)
    w = RolloutWorker(env, mac, args)
    buf = ReplayBuffer(args)
    w.record_sink = buf
    losses = []
    for i in range(updates):
        buf.store_episode(w.generate_episodes(E)[0])
        losses.append(learner.train(buf.sample(E), i))
    return learner, losses, learner._flat.flat.detach().cpu().numpy().copy()


def test_hip_graph_replay_equals_eager():
    """the update replayed from a hipGraph, the states read in place from the replay ring through the episode map"""
    from marl_amd.algorithm.common import GraphedUpdate
    out = {}
    for mode in (False, True):
        learner, losses, flat = _ring_run(mode, GraphedUpdate.WARMUP + 2)
        out[mode] = (losses, flat)
        if mode:
            g = learner.graphs
            assert not g.disabled, getattr(g, "error", "")
            assert any(e["graph"] is not None for e in g.entries.values()), "no graph was captured"
            assert g.replays >= 2
    assert all(np.isfinite(x) for x in out[False][0])
    assert out[False][0] == out[True][0]
    np.testing.assert_array_equal(out[False][1], out[True][1])


def test_launcher_trains_two_steps(tmp_path):
    from marl_amd.main import build, make_runner
    from marl_amd.algorithm.q_learner import QLearner
    from marl_amd.network.mixer import QattenMixer
    from marl_amd.utils.logging import Logger
    args, env = build(["--alg", "qatten", "--map", "MMM2", "--n_envs", "8", "--n_steps", "1", "--evaluate_epoch", "0",
                       "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "model")])
    assert (args.qatten_heads, args.qatten_embed_dim, args.qatten_unit_dim) == (4, 32, 32)
    args.save_cycle = 10 ** 9
    torch.manual_seed(3)
    r = make_runner(args, env, Logger())
    assert type(r.learner) is QLearner and type(r.learner.mixer) is QattenMixer and r.buffer is not None
    before = r.learner._flat.flat.clone()
    for _ in range(2):
        r.args.n_steps = r.time_steps + 1
        r.run(0)
    assert r.train_steps == 2 == len(r.losses) and all(np.isfinite(float(x)) for x in r.losses)
    assert not torch.equal(before, r.learner._flat.flat)
