"""The G2ANet kernels (csrc/g2anet.hip) and G2ANetMAC on the MI355X against tests/g2anet_oracle.py (float64).

Bounds: tests/parity.close, 1e-4 * max|ref| per tensor with its absolute floor; a tensor whose FLOAT32 ORACLE already misses a quarter
of that (tests/test_g2anet_cpu.py measures it: at tau = 0.01 the factor 1 / tau multiplies float32 rounding by 100) is bounded by 4 x
its float32-oracle error, g2anet_oracle.F32_EXCEPTIONS.  The head cases carry weights uniform in +-0.25 and a dlogits sized so that
every gradient is of order one (g2anet_oracle.head_case); each runs with hard on / off and tau 0.01 / 1."""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import learners
import parity
import g2anet_oracle as go

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
H = go.H


def _ops():
    from marl_amd import ops
    return ops


def _extra_groups(N):
    """one group more than two full workgroup tiles: marl_g2anet_groups_per_workgroup(N) = 16 / N whole groups share a 16-row tile"""
    return 2 * _ops().g2anet_groups_per_workgroup(N) + 1


@functools.lru_cache(maxsize=None)
def _content(G, N, A):
    return go.head_case(G, N, A, go.head_seed(G, N, A))


@functools.lru_cache(maxsize=None)
def _case(G, N, A, hard, tau):
    c = _content(G, N, A)
    return c, go.head_reference(c, N, hard, tau)


def _run_head(c, G, N, A, hard, tau, hs=None, noise="case", g=None):
    """(logits, dhs, grads) of one forward and one backward call on the case's content; ``g``: the gradient destinations (zeros)"""
    ops = _ops()
    t = lambda k: torch.tensor(c[k], device=DEV)
    w = {k: t(k) for k in go.HEAD_PARAMS}
    g = {k: torch.zeros_like(v) for k, v in w.items()} if g is None else g
    hs = t("hs") if hs is None else hs
    noise = t("noise") if isinstance(noise, str) else noise
    logits = torch.full((G * N, A), float("nan"), device=DEV)
    dhs = torch.full((G * N, H), float("nan"), device=DEV)
    ops.g2anet_head_fwd(ops.g2anet_weights(w), hs, noise, logits, G, N, A, hard, tau)
    ops.g2anet_head_bwd(ops.g2anet_weights(w), ops.g2anet_grads(g), hs, noise, t("dlogits"), dhs, G, N, A, hard, tau)
    return logits, dhs, g


def _close(name, key, tensor, got, ref):
    exc = go.F32_EXCEPTIONS.get(key + (tensor,))
    if exc is None:
        parity.close(name, tensor, got, ref)
    else:
        err = float(np.abs(np.asarray(got, dtype=np.float64) - ref).max())
        print("%s %s: err %.3e, bound 4 x %.2e" % (name, tensor, err, exc))
        assert err <= 4.0 * exc, (name, tensor, err, exc)


def _check_head(G, N, A, hard, tau):
    c, ref = _case(G, N, A, hard, tau)
    logits, dhs, g = _run_head(c, G, N, A, hard, tau)
    name = "g2anet head G=%d N=%d A=%d hard=%s tau=%g" % (G, N, A, hard, tau)
    key = ("head", G, N, A, hard, tau)
    _close(name, key, "logits", logits.cpu().numpy(), ref["logits"])
    _close(name, key, "dhs", dhs.cpu().numpy(), ref["dhs"])
    for k in go.HEAD_PARAMS:
        _close(name, key, k, g[k].cpu().numpy(), ref[k])
        if (not hard and k in go.HARD_PARAMS) or (N == 2 and k in go.ZERO_AT_N2):
            assert float(g[k].abs().max()) == 0.0 and float(np.abs(ref[k]).max()) == 0.0, k


@pytest.mark.parametrize("hard,tau", go.HEAD_MODES)
@pytest.mark.parametrize("G,N,A", go.HEAD_SHAPES)
def test_head_forward_and_backward_vs_float64(G, N, A, hard, tau):
    _check_head(G, N, A, hard, tau)


@pytest.mark.parametrize("hard,tau", go.HEAD_MODES)
@pytest.mark.parametrize("N,A", go.EXTRA_NA)
def test_head_one_group_past_full_tiles(N, A, hard, tau):
    _check_head(_extra_groups(N), N, A, hard, tau)


@pytest.mark.parametrize("hard,tau", go.HEAD_MODES)
@pytest.mark.parametrize("G,N,A", go.MANY_TILES)
def test_head_many_tiles(G, N, A, hard, tau):
    """more tiles than either kernel has workgroups (512 forward, 256 backward; 16 / N groups per tile): 667 and 600 tiles, so a
    workgroup walks two or three - LDS planes used again, gradient accumulators carried across tiles, slabs of several tiles"""
    _check_head(G, N, A, hard, tau)


@pytest.mark.parametrize("G,N,A", [(37, 5, 11), (2000, 5, 11)])
def test_null_noise_is_zero_noise(G, N, A):
    c = _content(G, N, A)
    l0, d0, g0 = _run_head(c, G, N, A, True, 0.01, noise=None)
    l1, d1, g1 = _run_head(c, G, N, A, True, 0.01, noise=torch.zeros(G * N, N - 1, device=DEV))
    assert torch.equal(l0, l1) and torch.equal(d0, d1) and all(torch.equal(g0[k], g1[k]) for k in go.HEAD_PARAMS)
    l2, _, _ = _run_head(c, G, N, A, True, 0.01)
    assert not torch.equal(l0, l2)


def test_head_refuses_what_it_does_not_cover():
    ops = _ops()
    from marl_amd._lib import MarlHipError
    assert all(ops.g2anet_supported(N, A, hard) for N in range(2, 11) for A in (1, 32) for hard in (True, False))
    c = go.head_case(2, 5, 11, seed=3)
    w = {k: torch.tensor(c[k], device=DEV) for k in go.HEAD_PARAMS}
    g = {k: torch.zeros_like(v) for k, v in w.items()}
    for N, A in ((1, 11), (11, 11), (5, 33)):
        assert not ops.g2anet_supported(N, A)
        rows = 2 * N
        hs, noise = torch.zeros(rows, H, device=DEV), torch.zeros(rows, max(N - 1, 1), device=DEV)
        logits, dhs = torch.zeros(rows, A, device=DEV), torch.zeros(rows, H, device=DEV)
        with pytest.raises(MarlHipError):
            ops.g2anet_head_fwd(ops.g2anet_weights(w), hs, noise, logits, 2, N, A, True, 0.01)
        with pytest.raises(MarlHipError):
            ops.g2anet_head_bwd(ops.g2anet_weights(w), ops.g2anet_grads(g), hs, noise, torch.ones(rows, A, device=DEV), dhs, 2, N, A, True, 0.01)
        if N != 5:
            buf = torch.zeros(2 * rows * max(N - 1, 1), device=DEV)
            with pytest.raises(MarlHipError):
                ops.g2anet_noise(1, 0, 0, buf, 2, 1, N)
            assert float(buf.abs().max()) == 0.0
        torch.cuda.synchronize()
        assert float(logits.abs().max()) == 0.0 and float(dhs.abs().max()) == 0.0 and all(float(v.abs().max()) == 0.0 for v in g.values())


@pytest.mark.parametrize("G,N,A,keep", [(37, 5, 11, 18), (2000, 5, 11, 18), (2000, 5, 11, 1700), (600, 10, 18, 599)])
def test_no_leakage_between_groups(G, N, A, keep):
    """every group's hs and noise but one overwritten: that group's logits and dhs keep their bits (at G = 2000 / 600 the group's tile
    is one of several its workgroup walks: 1700 / 3 = tile 566 is the second of forward workgroup 54 and the third of backward
    workgroup 54)"""
    c = _content(G, N, A)
    l0, d0, _ = _run_head(c, G, N, A, True, 0.01)
    hs = torch.tensor(c["hs"], device=DEV).view(G, N, H).clone()
    noise = torch.tensor(c["noise"], device=DEV).view(G, N, N - 1).clone()
    kept = hs[keep].clone(), noise[keep].clone()
    hs.copy_(torch.tanh(3.0 * hs + 0.5))
    noise.copy_(-noise)
    hs[keep], noise[keep] = kept
    l1, d1, _ = _run_head(c, G, N, A, True, 0.01, hs=hs.view(G * N, H), noise=noise.view(G * N, N - 1))
    assert torch.equal(l0.view(G, N, A)[keep], l1.view(G, N, A)[keep]) and torch.equal(d0.view(G, N, H)[keep], d1.view(G, N, H)[keep])
    assert not torch.equal(l0.view(G, N, A)[keep - 1], l1.view(G, N, A)[keep - 1])


@pytest.mark.parametrize("hard", [True, False])
@pytest.mark.parametrize("G,N,A", [(601, 5, 11)] + list(go.MANY_TILES))
def test_backward_is_deterministic(G, N, A, hard):
    c = _content(G, N, A)
    _, d0, g0 = _run_head(c, G, N, A, hard, 0.01)
    _, d1, g1 = _run_head(c, G, N, A, hard, 0.01)
    assert torch.equal(d0, d1) and all(torch.equal(g0[k], g1[k]) for k in go.HEAD_PARAMS)


@pytest.mark.parametrize("G,N,A", [(37, 5, 11), (2000, 5, 11)])
def test_backward_adds_into_its_gradient_destinations(G, N, A):
    """the sixteen gradients are ADDED: into destinations that hold other numbers, and a second call adds the same again; dhs is
    written.  tau = 1: the destinations' own float32 rounding, 6e-8 of values up to about 5, stays far inside 1e-4 max|ref|"""
    c, ref = _case(G, N, A, True, 1.0)
    rng = np.random.default_rng(G)
    init = {k: torch.tensor(rng.standard_normal(c[k].shape).astype(np.float32), device=DEV) for k in go.HEAD_PARAMS}
    g = {k: v.clone() for k, v in init.items()}
    _, d0, _ = _run_head(c, G, N, A, True, 1.0, g=g)
    name = "g2anet head adds G=%d" % G
    for k in go.HEAD_PARAMS:
        parity.close(name, "grad " + k, (g[k].double() - init[k].double()).cpu().numpy(), ref[k])
    once = {k: v.clone() for k, v in g.items()}
    _, d1, _ = _run_head(c, G, N, A, True, 1.0, g=g)
    for k in go.HEAD_PARAMS:
        parity.close(name, "grad twice " + k, (g[k].double() - init[k].double()).cpu().numpy(), 2.0 * ref[k])
        assert not torch.equal(g[k], once[k])
    assert torch.equal(d0, d1)


def test_noise_entry():
    ops = _ops()
    E, T, N = 3, 5, 5
    a = torch.full((E, T, N, N - 1), float("nan"), device=DEV)
    ops.g2anet_noise(123, 7, 1000, a, E, T, N)
    ref = go.noise(123, 7, 1000, E, T, N)
    assert torch.isfinite(a).all() and float(a.abs().max()) <= 17.4
    assert float(np.abs(a.cpu().numpy().astype(np.float64) - ref).max()) <= 2e-6
    steps = torch.empty_like(a)
    for t in range(T):
        one = torch.empty(E, 1, N, N - 1, device=DEV)
        ops.g2anet_noise(123, 7, 1000 + t, one, E, 1, N)
        steps[:, t] = one[:, 0]
    assert torch.equal(a, steps)
    b = torch.empty_like(a)
    for seed, env0, tg0 in ((123, 8, 1000), (123, 7, 1001), (124, 7, 1000)):
        ops.g2anet_noise(seed, env0, tg0, b, E, T, N)
        assert not torch.equal(a, b)
    ops.g2anet_noise(123, 8, 1000, b, E, T, N)
    assert torch.equal(a[1:], b[:-1])                  # environment env0 + e
    # a large draw count at the widest shape: finite everywhere, symmetric in the mean
    big = torch.empty(64, 120, 10, 9, device=DEV)
    ops.g2anet_noise(5, 0, 0, big, 64, 120, 10)
    assert torch.isfinite(big).all() and float(big.abs().max()) <= 17.4 and abs(float(big.mean())) < 0.02


def test_empty_launches():
    ops = _ops()
    c = go.head_case(1, 5, 11, seed=5)
    w = {k: torch.tensor(c[k], device=DEV) for k in go.HEAD_PARAMS}
    g = {k: torch.zeros_like(v) for k, v in w.items()}
    e = torch.empty(0, H, device=DEV)
    ops.g2anet_head_fwd(ops.g2anet_weights(w), e, torch.empty(0, 4, device=DEV), torch.empty(0, 11, device=DEV), 0, 5, 11, True, 0.01)
    ops.g2anet_head_bwd(ops.g2anet_weights(w), ops.g2anet_grads(g), e, None, torch.empty(0, 11, device=DEV), torch.empty(0, H, device=DEV),
                        0, 5, 11, True, 0.01)
    ops.g2anet_noise(1, 0, 0, torch.empty(0, device=DEV), 0, 4, 5)
    torch.cuda.synchronize()
    assert all(float(v.abs().max()) == 0.0 for v in g.values())


def test_controller_with_no_episodes_launches_nothing(monkeypatch):
    """B = 0 / E = 0: G2ANetMAC.unroll, planes, rollout_step, rollout_head and backward return before any launch"""
    ops = _ops()
    args, state, batch, mac = build_mac("2s3z")
    mac.cuda()
    N, A, O, T = args.n_agents, args.n_actions, args.obs_shape, 5

    def refuse(*a, **k):
        raise AssertionError("a kernel was launched for an empty batch")
    for f in ("linear", "linear_wgrad", "agent_unroll_fwd", "agent_unroll_bwd", "g2anet_head_fwd", "g2anet_head_bwd", "g2anet_noise"):
        monkeypatch.setattr(ops, f, refuse)
    e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=DEV)
    mac.unroll(e(0, T, N, O), T * N, 0, e(0, T, N, dt=torch.int32), T * N, -1, 0, T, e(0, T, N, A), None, e(0, H), None, h0=None)
    planes = mac.planes(lambda name, shape: e(*shape), (0, T, N, H))
    mac.unroll(e(0, T, N, O), T * N, 0, e(0, T, N, dt=torch.int32), T * N, -1, 0, T, e(0, T, N, A), planes, e(0, H), None, h0=None)
    rec = types.SimpleNamespace(T=T, obs=e(0, T + 1, N, O), u=e(0, T, N, dt=torch.int32))
    mac.rollout_step(mac.rollout_weights(), rec, 0, e(0, H), e(0, 1, N, A), 0)
    mac.rollout_head(e(0, H), e(0, 1, N, A), rec, 0, 0, False, 1, None)
    db = types.SimpleNamespace(B=0, T=T, N=N, A=A, O=O)
    mac.backward(db, None, planes, e(0, T, N, A), None)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- the controller
def build_mac(name, alg="reinforce", **over):
    """(args, oracle state, batch(i), G2ANetMAC with the state's weights)"""
    from marl_amd.controller.share_params import G2ANetMAC
    args, state, batch = go.learner_case(alg, name, **over)
    mac = G2ANetMAC(args)
    mac.agent.load_state_dict({k: x.detach().to(torch.float32) for k, x in state.agent.items()})
    return args, state, batch, mac


@pytest.mark.parametrize("name,flags", go.MAC_CASES)
def test_mac_unroll_and_backward_vs_oracle(name, flags):
    """G2ANetMAC.unroll (the unroll over encoding and h, then the head) and .backward on the ragged learner cases: logits and hs under
    m, all 22 parameter gradients in full, against autograd of the oracle fed the noise the device drew, read back"""
    from marl_amd.algorithm.reinforce import ReinforceLearner
    from marl_amd.hostutil import DeviceBatch
    args, state, batch, mac = build_mac(name, last_action=flags, reuse_network=flags)
    learner = ReinforceLearner(mac, args)
    b = batch(0)
    db = DeviceBatch.from_dict(learners.clone_batch(b), args, DEV, T=None)
    B, T, N, A = db.B, db.T, db.N, db.A
    oc, oc_bs, oc_t0 = db.o_cur
    mac.set_train_step(3)
    logits = torch.empty(B, T, N, A, device=DEV)
    planes = mac.planes(lambda name, shape: torch.empty(*shape, device=DEV), (B, T, N, H))
    drawn = planes.noise.cpu().numpy()
    assert float(np.abs(drawn - go.update_noise(args, 3, B, T, N)).max()) <= 2e-6
    saved, h_last = torch.empty(_ops().saved_shape(T, B, N), device=DEV), torch.empty(B * N, H, device=DEV)
    mac.unroll(oc, oc_bs, oc_t0, db.u_fed, db.u_bs, -1, B, T, logits, planes, h_last, saved, h0=None, ep_len=db.ep_len,
               ep_map=getattr(db, "o_map", None))
    # the oracle, on the noise the device drew
    _, _, b2, dl, ref = go.mac_reference(name, flags, lambda B_, T_, N_: drawn)
    assert all(np.array_equal(np.asarray(b[k]), np.asarray(b2[k])) for k in b)
    # an unroll that is not given the planes (other observations, the controller's own scratch) leaves them alone
    hs_before, noise_before = planes.hs.clone(), planes.noise.clone()
    mac.unroll(torch.randn_like(oc), oc_bs, oc_t0, db.u_fed, db.u_bs, -1, B, T, torch.empty_like(logits), None,
               torch.empty_like(h_last), None, h0=None)
    assert torch.equal(hs_before, planes.hs) and torch.equal(noise_before, planes.noise)
    dlg = dl.to(device=DEV, dtype=torch.float32).contiguous()
    with pytest.raises(TypeError):
        mac.backward(db, saved, planes.hs, dlg, learner._buf)
    learner._flat.zero_grad()
    mac.backward(db, saved, planes, dlg, learner._buf)
    c = "g2anet mac %s flags=%s" % (name, flags)
    key = ("mac", name, flags)
    m = (1.0 - torch.tensor(np.asarray(b["padded"])[:, :T], dtype=torch.float64)).reshape(B, T, 1, 1).numpy()
    assert torch.isfinite(logits).all()
    _close(c, key, "logits", logits.cpu().numpy() * m, ref["logits"])
    _close(c, key, "hs", planes.hs.cpu().numpy() * m, ref["hs"])
    got = dict(mac.agent.named_parameters())
    assert sorted("grad " + k for k in got) == sorted(k for k in ref if k.startswith("grad ")) and len(got) == 22
    for k, p in got.items():
        _close(c, key, "grad " + k, p.grad.cpu().numpy(), ref["grad " + k])


def test_serial_choose_action_is_refused_and_touches_nothing():
    args, state, batch, mac = build_mac("2s3z")
    mac.init_hidden(1)
    h = mac.hidden_states.clone()
    with pytest.raises(NotImplementedError, match="every agent's observation"):
        mac.choose_action(np.zeros(args.obs_shape), np.zeros(args.n_actions), 0, np.ones(args.n_actions), 0.1)
    assert torch.equal(h, mac.hidden_states)


# ---------------------------------------------------------------------------------------------------- rollouts
def _rollout(args, mac, E, env0, evaluate):
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    from marl_amd.rollout import RolloutWorker
    env = SyntheticSMACEnv(E, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, args.episode_limit, seed=args.seed,
                           env0=env0)
    w = RolloutWorker(env, mac, args)
    batch, _, _, _ = w.generate_episodes(evaluate=evaluate)
    return batch.record, env


def _rollout_args():
    from marl_amd.main import build
    args, _ = build(["--map", "2s3z", "--alg", "reinforce+g2anet", "--n_envs", "8"])
    args.episode_limit = 6
    return args


def test_evaluation_rollout_batched_equals_serial_environments():
    from marl_amd.controller.share_params import G2ANetMAC
    args = _rollout_args()
    torch.manual_seed(5)
    mac = G2ANetMAC(args)
    rec, _ = _rollout(args, mac, 8, 0, True)
    for e in range(8):
        one, _ = _rollout(args, mac, 1, e, True)
        for k in ("obs", "u", "r", "term", "padded"):
            assert torch.equal(getattr(rec, k)[e:e + 1], getattr(one, k)), (e, k)


def test_training_rollout_samples_available_actions_and_unroll_reproduces_it():
    from marl_amd.controller.share_params import G2ANetMAC, G2ANetPlanes
    from marl_amd.rollout import RolloutWorker
    args = _rollout_args()
    torch.manual_seed(6)
    mac = G2ANetMAC(args)
    ops = _ops()
    seen, calls = [], []
    real = ops.policy_sample
    head = mac.rollout_head

    def spy_head(h, q, rec, t, E, evaluate, rseed, env):
        q.fill_(float("nan"))                        # the head WRITES q
        head(h, q, rec, t, E, evaluate, rseed, env)
        seen.append(q.clone())
    mac.rollout_head = spy_head
    ops.policy_sample = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        rec, env = _rollout(args, mac, 8, 0, False)
    finally:
        ops.policy_sample = real
        del mac.rollout_head
    E, T, N, A = 8, rec.T, args.n_agents, args.n_actions
    assert len(calls) == T == len(seen) and all(torch.isfinite(q).all() for q in seen)
    live = (rec.padded.view(E, T) == 0)
    u = rec.u.view(E, T, N).long()
    av = torch.gather(rec.avail[:, :T].reshape(E, T, N, A), 3, u.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    assert bool(((av > 0) | ~live.unsqueeze(-1)).all()) and bool(live.any())
    # the T-step unroll over the record, on the noise one call regenerates from the episode's first global step, reproduces the
    # per-step logits at the real steps, bit for bit
    noise = torch.empty(E, T, N, N - 1, device=DEV)
    ops.g2anet_noise(args.seed, env.env0, env.global_step(0), noise, E, T, N)
    planes = G2ANetPlanes(torch.empty(E, T, N, H, device=DEV), noise)
    logits = torch.empty(E, T, N, A, device=DEV)
    mac.unroll(rec.obs, (T + 1) * N, 0, rec.u, T * N, -1, E, T, logits, planes, torch.empty(E * N, H, device=DEV), None, h0=None)
    per_step = torch.stack([q.view(E, N, A) for q in seen], 1)
    assert torch.equal(logits[live], per_step[live])
    # ... and the update's own draws are other numbers
    other = torch.empty(E, T, N, A, device=DEV)
    mac.unroll(rec.obs, (T + 1) * N, 0, rec.u, T * N, -1, E, T, other, None, torch.empty(E * N, H, device=DEV), None, h0=None)
    assert not torch.equal(other[live], per_step[live])
    # overlapped / whole-rollout launches refuse the head
    w = RolloutWorker(env, mac, args)
    with pytest.raises(RuntimeError, match="g2anet head"):
        w.launch_episodes()
