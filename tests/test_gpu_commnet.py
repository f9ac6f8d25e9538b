"""The CommNet kernels (csrc/commnet.hip) and CommNetMAC on the MI355X against tests/commnet_oracle.py (float64).

Bounds: tests/parity.close, 1e-4 * max|ref| per tensor with its absolute floor.  The head cases carry weights at twice torch's init
scale and a dlogits sized so that every gradient is of order one (commnet_oracle.head_case)."""
import functools

import numpy as np
import pytest
import torch

from oracle import learners, nets, seeded
import parity
import commnet_oracle as cn
import pg_oracle as pg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
H = cn.H


def _ops():
    from marl_amd import ops
    return ops


def _extra_groups(N):
    """one group more than two full workgroup tiles: marl_commnet_groups_per_workgroup(N) = 16 / N whole groups share a 16-row tile
    (csrc/commnet.hip), so this G leaves a tile with a single group in it"""
    return 2 * _ops().commnet_groups_per_workgroup(N) + 1


# more tiles than either kernel has workgroups (csrc/commnet.hip: 512 forward, 256 backward; 16 / N groups per tile): 667 and 600 tiles,
# so a workgroup walks two or three tiles - LDS planes used again, gradient accumulators carried across tiles, slabs of several tiles
MANY_TILES = ((2000, 5, 11), (600, 10, 18))
HEAD_CASES = [s + (K,) for s in cn.HEAD_SHAPES for K in cn.HEAD_KS] + [s + (3,) for s in MANY_TILES]
EXTRA_CASES = [(N, A, K) for (N, A) in ((2, 3), (3, 9), (5, 11), (8, 14), (10, 18)) for K in (3,)]


@functools.lru_cache(maxsize=None)
def _case(G, N, A, K):
    c = cn.head_case(G, N, A, seed=1000 + 7 * G + N)
    return c, cn.head_reference(c, N, K)


def _run_head(c, G, N, A, K, hs=None, g=None):
    """(logits, dhs, grads) of one forward and one backward call on the case's content; ``g``: the gradient destinations (zeros)"""
    ops = _ops()
    t = lambda k: torch.tensor(c[k], device=DEV)
    w = {k: t(k) for k in cn.HEAD_PARAMS}
    g = {k: torch.zeros_like(v) for k, v in w.items()} if g is None else g
    hs = t("hs") if hs is None else hs
    logits = torch.full((G * N, A), float("nan"), device=DEV)
    dhs = torch.full((G * N, H), float("nan"), device=DEV)
    ops.commnet_head_fwd(ops.commnet_weights(w), hs, logits, G, N, A, K)
    ops.commnet_head_bwd(ops.commnet_weights(w), ops.commnet_grads(g), hs, t("dlogits"), dhs, G, N, A, K)
    return logits, dhs, g


def _check_head(G, N, A, K):
    c, ref = _case(G, N, A, K)
    logits, dhs, g = _run_head(c, G, N, A, K)
    name = "commnet head G=%d N=%d A=%d K=%d" % (G, N, A, K)
    parity.close(name, "logits", logits.cpu().numpy(), ref["logits"])
    parity.close(name, "dhs", dhs.cpu().numpy(), ref["dhs"])
    for k in cn.HEAD_PARAMS:
        parity.close(name, "grad " + k, g[k].cpu().numpy(), ref[k])
        assert float(np.abs(ref[k]).max()) > 0.05 or (K == 1 and k == "f_comm.weight_ih"), (k, float(np.abs(ref[k]).max()))
    if K == 1:                                  # round 0 has a zero input: its W_ih never sees a gradient
        assert float(g["f_comm.weight_ih"].abs().max()) == 0.0


@pytest.mark.parametrize("G,N,A,K", HEAD_CASES)
def test_head_forward_and_backward_vs_float64(G, N, A, K):
    _check_head(G, N, A, K)


@pytest.mark.parametrize("N,A,K", EXTRA_CASES)
def test_head_one_group_past_full_tiles(N, A, K):
    _check_head(_extra_groups(N), N, A, K)


def test_head_refuses_what_it_does_not_cover():
    ops = _ops()
    from marl_amd._lib import MarlHipError
    assert all(ops.commnet_supported(N, A, K) for N in range(2, 11) for A in (1, 32) for K in (1, 4))
    assert not ops.commnet_supported(17, 5, 2) and not ops.commnet_supported(5, 33, 2) and not ops.commnet_supported(5, 5, 5)
    assert not ops.commnet_supported(5, 5, 0) and not ops.commnet_supported(0, 5, 1)
    c = cn.head_case(2, 5, 11, seed=3)
    w = {k: torch.tensor(c[k], device=DEV) for k in cn.HEAD_PARAMS}
    logits = torch.zeros(10, 11, device=DEV)
    with pytest.raises(MarlHipError):
        ops.commnet_head_fwd(ops.commnet_weights(w), torch.tensor(c["hs"], device=DEV), logits, 2, 5, 11, 5)
    assert float(logits.abs().max()) == 0.0


@pytest.mark.parametrize("G,N,A,keep", [(37, 5, 11, 18), (2000, 5, 11, 18), (2000, 5, 11, 1700), (600, 10, 18, 599)])
def test_no_leakage_between_groups(G, N, A, keep):
    """every group's hs but one overwritten: that group's logits and dhs keep their bits (at G = 2000 / 600 the group's tile is one of
    several its workgroup walks: 1700 / 3 = tile 566 is the second of forward workgroup 54 and the third of backward workgroup 54)"""
    K = 3
    c, _ = _case(G, N, A, K)
    l0, d0, _ = _run_head(c, G, N, A, K)
    hs = torch.tensor(c["hs"], device=DEV).view(G, N, H).clone()
    kept = hs[keep].clone()
    hs.copy_(torch.tanh(3.0 * hs + 0.5))
    hs[keep] = kept
    l1, d1, _ = _run_head(c, G, N, A, K, hs=hs.view(G * N, H))
    assert torch.equal(l0.view(G, N, A)[keep], l1.view(G, N, A)[keep]) and torch.equal(d0.view(G, N, H)[keep], d1.view(G, N, H)[keep])
    assert not torch.equal(l0.view(G, N, A)[keep - 1], l1.view(G, N, A)[keep - 1])


@pytest.mark.parametrize("G,N,A", [(601, 5, 11)] + list(MANY_TILES))
def test_backward_is_deterministic(G, N, A):
    K = 3
    c, _ = _case(G, N, A, K)
    _, d0, g0 = _run_head(c, G, N, A, K)
    _, d1, g1 = _run_head(c, G, N, A, K)
    assert torch.equal(d0, d1) and all(torch.equal(g0[k], g1[k]) for k in cn.HEAD_PARAMS)


@pytest.mark.parametrize("G,N,A", [(37, 5, 11), (2000, 5, 11)])
def test_backward_adds_into_its_gradient_destinations(G, N, A):
    """the six gradients are ADDED: into destinations that hold other numbers, and a second call adds the same again; dhs is written.
    (the destinations' own float32 rounding, 6e-8 of values up to about 5, is far inside 1e-4 max|ref|: the bound stays the head's)"""
    K = 3
    c, ref = _case(G, N, A, K)
    rng = np.random.default_rng(G)
    init = {k: torch.tensor(rng.standard_normal(c[k].shape).astype(np.float32), device=DEV) for k in cn.HEAD_PARAMS}
    g = {k: v.clone() for k, v in init.items()}
    _, d0, _ = _run_head(c, G, N, A, K, g=g)
    name = "commnet head adds G=%d" % G
    for k in cn.HEAD_PARAMS:
        parity.close(name, "grad " + k, (g[k].double() - init[k].double()).cpu().numpy(), ref[k])
    once = {k: v.clone() for k, v in g.items()}
    _, d1, _ = _run_head(c, G, N, A, K, g=g)
    for k in cn.HEAD_PARAMS:
        parity.close(name, "grad twice " + k, (g[k].double() - init[k].double()).cpu().numpy(), 2.0 * ref[k])
        assert not torch.equal(g[k], once[k])
    assert torch.equal(d0, d1)


@pytest.mark.parametrize("rows", [1, 63, 64, 1025])
def test_sigmoid_kernels(rows):
    ops = _ops()
    rng = np.random.default_rng(rows)
    x = (3.0 * rng.standard_normal((rows, H))).astype(np.float32)
    de = rng.standard_normal((rows, H)).astype(np.float32)
    e64 = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    e = torch.tensor(x, device=DEV)
    ops.commnet_sigmoid_fwd(e)
    parity.close("sigmoid rows=%d" % rows, "e", e.cpu().numpy(), e64)
    d = torch.empty_like(e)
    ops.commnet_sigmoid_bwd(torch.tensor(de, device=DEV), e, d)
    ef = e.cpu().numpy().astype(np.float64)
    parity.close("sigmoid rows=%d" % rows, "dxp", d.cpu().numpy(), de.astype(np.float64) * ef * (1.0 - ef))
    # views that start 4 bytes later: the same bits, element for element (in place for the backward as the controller runs it)
    n = rows * H
    buf = torch.zeros(n + 1, device=DEV)
    buf[1:] = torch.tensor(x, device=DEV).view(-1)
    ops.commnet_sigmoid_fwd(buf[1:])
    assert torch.equal(buf[1:], e.view(-1)) and float(buf[0]) == 0.0
    dbuf = torch.zeros(n + 1, device=DEV)
    dbuf[1:] = torch.tensor(de, device=DEV).view(-1)
    ops.commnet_sigmoid_bwd(dbuf[1:], buf[1:], dbuf[1:])
    assert torch.equal(dbuf[1:], d.view(-1)) and float(dbuf[0]) == 0.0
    dm = torch.tensor(de, device=DEV).view(-1)
    ops.commnet_sigmoid_bwd(dm, buf[1:], dm)                     # operands on different boundaries: the elementwise kernel
    assert torch.equal(dm, d.view(-1))


def test_empty_launches():
    ops = _ops()
    c = cn.head_case(1, 5, 11, seed=5)
    w = {k: torch.tensor(c[k], device=DEV) for k in cn.HEAD_PARAMS}
    g = {k: torch.zeros_like(v) for k, v in w.items()}
    e = torch.empty(0, H, device=DEV)
    ops.commnet_head_fwd(ops.commnet_weights(w), e, torch.empty(0, 11, device=DEV), 0, 5, 11, 3)
    ops.commnet_head_bwd(ops.commnet_weights(w), ops.commnet_grads(g), e, torch.empty(0, 11, device=DEV), torch.empty(0, H, device=DEV),
                         0, 5, 11, 3)
    ops.commnet_sigmoid_fwd(e)
    ops.commnet_sigmoid_bwd(e, e, torch.empty(0, H, device=DEV))
    torch.cuda.synchronize()
    assert all(float(v.abs().max()) == 0.0 for v in g.values())


def test_controller_with_no_episodes_launches_nothing(monkeypatch):
    """B = 0 / E = 0: CommNetMAC.unroll, rollout_step and backward return before any launch"""
    import types
    ops = _ops()
    args, state, batch, mac = build_mac("2s3z")
    mac.cuda()
    N, A, O, T = args.n_agents, args.n_actions, args.obs_shape, 5

    def refuse(*a, **k):
        raise AssertionError("a kernel was launched for an empty batch")
    for f in ("linear", "linear_wgrad", "agent_unroll_fwd", "agent_unroll_bwd", "commnet_head_fwd", "commnet_head_bwd",
              "commnet_sigmoid_fwd", "commnet_sigmoid_bwd"):
        monkeypatch.setattr(ops, f, refuse)
    e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=DEV)
    mac.unroll(e(0, T, N, O), T * N, 0, e(0, T, N, dt=torch.int32), T * N, -1, 0, T, e(0, T, N, A), None, e(0, H), None, h0=None)
    planes = mac.planes(lambda name, shape: e(*shape), (0, T, N, H))
    mac.unroll(e(0, T, N, O), T * N, 0, e(0, T, N, dt=torch.int32), T * N, -1, 0, T, e(0, T, N, A), planes, e(0, H), None, h0=None)
    rec = types.SimpleNamespace(T=T, obs=e(0, T + 1, N, O), u=e(0, T, N, dt=torch.int32))
    mac.rollout_step(mac.rollout_weights(), rec, 0, e(0, H), e(0, 1, N, A), 0)
    db = types.SimpleNamespace(B=0, T=T, N=N, A=A, O=O)
    mac.backward(db, None, planes, e(0, T, N, A), None)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- the controller
def build_mac(name, alg="reinforce", **over):
    """(args, oracle state, batch(i), CommNetMAC with the state's weights)"""
    from marl_amd.controller.share_params import CommNetMAC
    args, state, batch = cn.learner_case(alg, name, **over)
    mac = CommNetMAC(args)
    mac.agent.load_state_dict({k: x.detach().to(torch.float32) for k, x in state.agent.items()})
    return args, state, batch, mac


@pytest.mark.parametrize("flags", [True, False])
@pytest.mark.parametrize("name", ["2s3z", "MMM2"])
def test_mac_unroll_and_backward_vs_oracle(name, flags):
    """CommNetMAC.unroll (encoder, the unroll through the identity front, head) and .backward on the ragged learner cases: logits and
    hs under m, all twelve parameter gradients (ten weight / bias tensors of four layers, f_obs's and f_comm's biases twice) in full"""
    from marl_amd.algorithm.reinforce import ReinforceLearner
    from marl_amd.hostutil import DeviceBatch
    args, state, batch, mac = build_mac(name, last_action=flags, reuse_network=flags)
    learner = ReinforceLearner(mac, args)
    b = batch(0)
    db = DeviceBatch.from_dict(learners.clone_batch(b), args, DEV, T=None)
    B, T, N, A = db.B, db.T, db.N, db.A
    K = args.k
    # the oracle
    dt = torch.float64
    bt = {k: torch.tensor(np.asarray(v)[:, :T], dtype=torch.long if k == "u" else dt) for k, v in b.items()}
    fed = nets.shifted_onehot(bt["u_onehot"])
    z, hs_ref, _ = cn.unroll(state.agent, bt["o"], fed, torch.zeros(B * N, H, dtype=dt), args.last_action, args.reuse_network, K)
    m = (1.0 - bt["padded"]).reshape(B, T, 1, 1)
    rng = np.random.default_rng(11)
    dl = torch.tensor(rng.standard_normal((B, T, N, A)), dtype=dt) * m
    names = list(state.agent)
    gs = torch.autograd.grad((z * dl).sum(), [state.agent[k] for k in names])
    # the product
    oc, oc_bs, oc_t0 = db.o_cur
    logits = torch.empty(B, T, N, A, device=DEV)
    planes = mac.planes(lambda name, shape: torch.empty(*shape, device=DEV), (B, T, N, H))
    hs = planes.hs
    saved, h_last = torch.empty(_ops().saved_shape(T, B, N), device=DEV), torch.empty(B * N, H, device=DEV)
    mac.unroll(oc, oc_bs, oc_t0, db.u_fed, db.u_bs, -1, B, T, logits, planes, h_last, saved, h0=None, ep_len=db.ep_len,
               ep_map=getattr(db, "o_map", None))
    # an unroll that is not given the planes (other observations, the controller's own scratch) leaves them alone
    hs_before, e_before = planes.hs.clone(), planes.e.clone()
    mac.unroll(torch.randn_like(oc), oc_bs, oc_t0, db.u_fed, db.u_bs, -1, B, T, torch.empty_like(logits), None,
               torch.empty_like(h_last), None, h0=None)
    assert torch.equal(hs_before, planes.hs) and torch.equal(e_before, planes.e)
    with pytest.raises(TypeError):
        mac.backward(db, saved, hs, dl.to(device=DEV, dtype=torch.float32).contiguous(), learner._buf)
    learner._flat.zero_grad()
    mac.backward(db, saved, planes, dl.to(device=DEV, dtype=torch.float32).contiguous(), learner._buf)
    c = "commnet mac %s flags=%s" % (name, flags)
    mn = m.numpy()
    assert torch.isfinite(logits).all()
    parity.close(c, "logits", logits.cpu().numpy() * mn, z.detach().numpy() * mn)
    parity.close(c, "hs", hs.cpu().numpy() * mn, hs_ref.detach().numpy() * mn)
    got = dict(mac.agent.named_parameters())
    assert sorted(got) == sorted(names) and len(names) == 12
    for k, g in zip(names, gs):
        parity.close(c, "grad " + k, got[k].grad.cpu().numpy(), g.numpy())


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
    return batch.record


def _rollout_args():
    from marl_amd.main import build
    args, _ = build(["--map", "2s3z", "--alg", "reinforce+commnet", "--n_envs", "8"])
    args.episode_limit = 6
    return args


def test_evaluation_rollout_batched_equals_serial_environments():
    from marl_amd.controller.share_params import CommNetMAC
    args = _rollout_args()
    torch.manual_seed(5)
    mac = CommNetMAC(args)
    rec = _rollout(args, mac, 8, 0, True)
    for e in range(8):
        one = _rollout(args, mac, 1, e, True)
        for k in ("obs", "u", "r", "term", "padded"):
            assert torch.equal(getattr(rec, k)[e:e + 1], getattr(one, k)), (e, k)


def test_training_rollout_samples_available_actions_and_unroll_reproduces_it():
    from marl_amd.controller.share_params import CommNetMAC
    args = _rollout_args()
    torch.manual_seed(6)
    mac = CommNetMAC(args)
    ops = _ops()
    seen = []
    real = ops.policy_sample
    step = mac.rollout_step

    def spy_step(w, rec, t, h, q, E):
        step(w, rec, t, h, q, E)
        seen.append(q.clone())
    mac.rollout_step = spy_step
    calls = []
    ops.policy_sample = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        rec = _rollout(args, mac, 8, 0, False)
    finally:
        ops.policy_sample = real
        del mac.rollout_step
    E, T, N, A = 8, rec.T, args.n_agents, args.n_actions
    assert len(calls) == T == len(seen)
    live = (rec.padded.view(E, T) == 0)
    u = rec.u.view(E, T, N).long()
    av = torch.gather(rec.avail[:, :T].reshape(E, T, N, A), 3, u.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    assert bool(((av > 0) | ~live.unsqueeze(-1)).all()) and bool(live.any())
    # the T-step unroll over the record reproduces the per-step logits at the real steps, bit for bit
    logits = torch.empty(E, T, N, A, device=DEV)
    mac.unroll(rec.obs, (T + 1) * N, 0, rec.u, T * N, -1, E, T, logits, None, torch.empty(E * N, H, device=DEV), None, h0=None)
    per_step = torch.stack([q.view(E, N, A) for q in seen], 1)
    assert torch.equal(logits[live], per_step[live])
