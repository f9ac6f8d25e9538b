"""CentralFFMixer and WQMIXLearner on the MI355X against tests/wqmix_oracle.py.  Needs a real MI355X: ``pytest -m gpu``.

Module level: hip_forward / hip_backward against autograd of the float64 ``central_mix`` - Qc, dq and every parameter's .grad,
parity.close at 1e-4 * max|ref|.  Learner level: three updates of ow_qmix and of cw_qmix beside the oracle learner at the batch shape
of the Qatten and IQL learner tests, in both gemm modes, with the bounds of tests/test_gpu_learners.py - the loss, ``den`` exactly, the
weights and the selected actions exactly, the first update's gradients, all parameters of both agents and both mixers (the tensors
wqmix_oracle.F32_EXCEPTIONS lists: four times their CPU figure); one TD(lambda) case; the target sync; a checkpoint round trip; the
launcher on the matrix game and on the battle environment."""
import os
import shutil

import numpy as np
import pytest
import torch

from oracle import seeded, learners
import wqmix_oracle as wo
import parity

pytestmark = pytest.mark.gpu

DEV = "cuda"
t32 = lambda d: {k: torch.tensor(x) for k, x in d.items()}


@pytest.mark.parametrize("name, R", [("2s3z", 65), ("MMM2", 33)])
def test_central_mixer_against_autograd(name, R):
    from marl_amd.network.mixer import CentralFFMixer
    from marl_amd.hostutil import flatten_module
    args = seeded.make_args(name, "ow_qmix")
    Pn = seeded.seeded_state(wo.central_param_shapes(args), seed=5)
    m = CentralFFMixer(args)
    assert [k for k, _ in m.state_dict().items()] == list(Pn)
    m.load_state_dict(t32(Pn))
    m.to(DEV)
    flatten_module(m, DEV, with_grad=True)
    P = {k: torch.tensor(x, dtype=torch.float64, requires_grad=True) for k, x in Pn.items()}
    N, S = args.n_agents, args.state_shape
    g = np.random.default_rng(R)
    q, s, gin = (g.standard_normal(shape).astype(np.float32) for shape in ((R, N), (R, S), (R,)))
    t64 = lambda x: torch.tensor(x, dtype=torch.float64)
    up = lambda x: torch.tensor(x, device=DEV)
    case = "central_mixer:%s" % name
    q64 = t64(q).requires_grad_(True)
    ref = wo.central_mix(P, q64, t64(s))
    names = list(P)
    grads = torch.autograd.grad((ref * t64(gin)).sum(), [q64] + [P[k] for k in names])
    ctx = {}
    m._flat.zero_grad()
    qd, sd = up(q), up(s)
    out = m.hip_forward(qd, sd, R, ctx=ctx)
    parity.close(case, "Qc", out.cpu().numpy(), ref.detach().numpy())
    # a second forward under another tag (the learner's greedy one) leaves the kept activations alone
    other = m.hip_forward(up(q[::-1].copy()), sd, R, tag="g")
    assert not torch.equal(other, out)
    dq = m.hip_backward(ctx, up(gin), R)
    parity.close(case, "dq", dq.cpu().numpy(), grads[0].numpy())
    for k, gref in zip(names, grads[1:]):
        parity.close(case, "grad " + k, dict(m.named_parameters())[k].grad.cpu().numpy(), gref.numpy())
    parity.close(case, "forward", m(torch.tensor(q).view(1, R, N), torch.tensor(s).view(1, R, S)).cpu().numpy().reshape(R), ref.detach().numpy())


def build_product(args, gemm_mode=None):
    from marl_amd.controller.share_params import SharedMAC
    from marl_amd.algorithm.wqmix import WQMIXLearner
    from marl_amd.network.mixer import QMixMixer, CentralFFMixer
    args.cuda = True
    if gemm_mode is not None:
        args.gemm_mode = gemm_mode
    mac = SharedMAC(args)
    mac.agent.load_state_dict(t32(seeded.seeded_state(seeded.agent_param_shapes(args), seed=wo.AGENT_SEED)))
    learner = WQMIXLearner(mac, args)
    assert type(learner.mixer) is QMixMixer and type(learner.central_mixer) is CentralFFMixer and learner.graphs is None
    for nets, state in (((learner.mixer, learner.target_mixer), seeded.seeded_state(seeded.qmix_param_shapes(args), seed=wo.MIXER_SEED)),
                        ((learner.central_net.agent, learner.target_central_net.agent),
                         seeded.seeded_state(seeded.agent_param_shapes(args), seed=wo.CENTRAL_AGENT_SEED)),
                        ((learner.central_mixer, learner.target_central_mixer),
                         seeded.seeded_state(wo.central_param_shapes(args), seed=wo.CENTRAL_MIXER_SEED))):
        for net in nets:
            net.load_state_dict(t32(state))
    return mac, learner


def named(learner):
    return [(p + "." + k, x) for p, net in (("agent", learner.eval_net.agent), ("mixer", learner.mixer),
                                            ("central_agent", learner.central_net.agent), ("central_mixer", learner.central_mixer))
            for k, x in net.named_parameters()]


def three_updates(case, gemm_mode, **more):
    args, st, batch_of, lam = wo.learner_case(case, **more)
    _, learner = build_product(wo.learner_case(case, **more)[0], gemm_mode)
    for i, tol in enumerate(wo.LEARNER_TOL):
        batch = batch_of(i, st)                              # (CW: planted with the oracle's state before this update)
        loss = learner.train(learners.clone_batch(batch), i)
        oloss, ograds, o = wo.train(st, learners.clone_batch(batch), i, lam=lam)
        c = "wqmix_train:%s[%s]/step%d" % (case, gemm_mode, i)
        assert learner.max_episode_len == o["T"]
        stats = learner.last_stats.cpu().numpy().astype(np.float64)
        print(c, "loss", loss, oloss, "stats", stats, "oracle", [float(o[k]) for k in ("num", "den", "num_c", "ones")])
        parity.close(c, "loss", loss, oloss, tol=tol)
        den = stats[1]
        assert den == float(o["den"]) and stats[3] == float(o["ones"]) <= den
        dbg, live = learner._dbg, o["live"]
        B, T = live.shape
        assert np.array_equal(dbg["w"].cpu().numpy().reshape(B, T), o["w"].numpy())
        assert np.array_equal(dbg["u_next"].cpu().numpy()[live.numpy()], o["u_next"].numpy()[live.numpy()])
        if o["u_greedy"] is not None:
            assert np.array_equal(dbg["u_greedy"].cpu().numpy()[live.numpy()], o["u_greedy"].numpy()[live.numpy()])
        parity.close(c, "y", dbg["y"].cpu().numpy().reshape(B, T) * live.numpy(), (o["y"] * live).numpy(), tol=tol)
        parity.close(c, "q_central", dbg["q_central"].cpu().numpy().reshape(B, T) * live.numpy(), (o["q_central"].detach() * live).numpy(), tol=tol)
        got, ref = named(learner), dict(st.named_params())
        assert [k for k, _ in got] == list(ref)
        for n, p in got:
            if i == 0:
                parity.close(c, "grad " + n, p.grad.detach().cpu().numpy() / den, ograds[n].numpy(), tol=tol)
            exc = wo.F32_EXCEPTIONS.get((case, i, "param " + n))
            if exc is None:
                parity.close(c, "param " + n, p.detach().cpu().numpy(), ref[n].detach().numpy(), tol=tol)
            else:
                err = float(np.abs(p.detach().cpu().numpy().astype(np.float64) - ref[n].detach().numpy()).max())
                print(c, "param", n, "err %.3e against the listed float32-oracle figure %.3e" % (err, exc))
                assert err <= 4.0 * exc, (c, n, err, exc)
    return learner, st


def test_three_updates_of_ow_qmix_vs_oracle(gemm_mode):
    three_updates("ow", gemm_mode)


def test_three_updates_of_cw_qmix_vs_oracle(gemm_mode):
    three_updates("cw", gemm_mode)


def test_three_updates_on_lambda_returns():
    three_updates("ow_lam0.8", "f32")


def test_target_sync_fires_at_target_update_cycle():
    args, st, batch_of, _ = wo.learner_case("ow", target_update_cycle=2)
    _, learner = build_product(args)
    pairs = [(learner.eval_net.agent, learner.target_net.agent), (learner.mixer, learner.target_mixer),
             (learner.central_net.agent, learner.target_central_net.agent), (learner.central_mixer, learner.target_central_mixer)]
    flat = lambda net: torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    start = [flat(t).clone() for _, t in pairs]
    assert all(torch.equal(flat(e), flat(t)) for e, t in pairs)
    for i in range(3):
        assert np.isfinite(learner.train(learners.clone_batch(batch_of(i, st)), i))
        for (e, t), s0 in zip(pairs, start):
            if i < 2:
                assert torch.equal(flat(t), s0) and not torch.equal(flat(e), flat(t)), i
            else:
                assert torch.equal(flat(e), flat(t)) and not torch.equal(flat(t), s0)


def test_checkpoint_and_resume_round_trip(tmp_path):
    args, st, batch_of, _ = wo.learner_case("cw", model_dir=str(tmp_path), save_cycle=1)
    _, a = build_product(args)
    a.train(learners.clone_batch(batch_of(0, st)), 0)
    a.save_models(7)
    d = a.model_dir
    assert sorted(os.listdir(d)) == ["7_central_mixer_net_params.pkl", "7_central_rnn_net_params.pkl", "7_mixer_net_params.pkl",
                                     "7_rnn_net_params.pkl"]
    for f in os.listdir(d):
        shutil.copy(os.path.join(d, f), os.path.join(d, f[2:]))           # load_models reads the un-numbered names
    a.save_resume(str(tmp_path / "resume.pt"))
    torch.manual_seed(99)
    _, b = build_product(wo.learner_case("cw", model_dir=str(tmp_path), save_cycle=1)[0])
    assert not torch.equal(a._flat.flat, b._flat.flat)
    b.load_models()
    assert torch.equal(a._flat.flat, b._flat.flat)                        # all four trained networks, to the same bits
    b.load_resume(str(tmp_path / "resume.pt"))
    assert set(a.resume_state()) >= {"target_agent", "target_mixer", "target_central_agent", "target_central_mixer"}
    for k, x in a.resume_state().items():
        y = b.resume_state()[k]
        assert torch.equal(x, y) if isinstance(x, torch.Tensor) else (k == "optimizer" or x == y), k
    assert torch.equal(a.optimizer.s1, b.optimizer.s1)
    # and the two go on to the same bits
    la = a.train(learners.clone_batch(batch_of(1, st)), 1)
    lb = b.train(learners.clone_batch(batch_of(1, st)), 1)
    assert la == lb and torch.equal(a._flat.flat, b._flat.flat)


@pytest.mark.parametrize("argv", [["--env", "matrix", "--alg", "ow_qmix", "--n_envs", "32"],
                                  ["--env", "battle", "--map", "3m", "--alg", "cw_qmix", "--n_envs", "8"]], ids=["matrix-ow", "battle-cw"])
def test_launcher_trains(argv, tmp_path):
    from marl_amd.main import build, make_runner
    from marl_amd.algorithm.wqmix import WQMIXLearner
    from marl_amd.utils.logging import Logger
    args, env = build(argv + ["--n_steps", "1", "--evaluate_epoch", "0", "--result_dir", str(tmp_path / "res"),
                              "--model_dir", str(tmp_path / "model")])
    assert (args.wqmix_alpha, args.central_mixing_embed_dim) == (0.5 if args.alg == "ow_qmix" else 0.75, 256)
    args.save_cycle = 10 ** 9
    torch.manual_seed(3)
    r = make_runner(args, env, Logger())
    assert type(r.learner) is WQMIXLearner and r.buffer is not None
    before = r.learner._flat.flat.clone()
    updates = 0
    while r.time_steps < 300 and updates < 40:               # a few hundred environment steps, one update after every rollout
        updates += 1
        r.args.n_steps = r.time_steps + 1
        r.run(0)
        s = r.learner.last_stats.cpu().numpy()
        assert np.isfinite(s).all() and 0 <= s[3] <= s[1] and s[1] > 0, s
    print(argv, "environment steps", r.time_steps, "updates", r.train_steps, "last stats", s)
    assert r.time_steps >= 300 and r.train_steps == updates == len(r.losses) and all(np.isfinite(float(x)) for x in r.losses)
    assert not torch.equal(before, r.learner._flat.flat)
    if args.env == "matrix":
        table, qi, qj = r.learner.get_q_and_q_tot_table()
        assert table.shape == (3, 3) and np.isfinite(table).all()
