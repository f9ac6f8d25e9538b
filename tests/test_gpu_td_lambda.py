"""TD(lambda) returns on the MI355X: csrc/td_lambda.hip against the float64 fixture of the reference's function, exact probes
across the 64-step chunk seams, the kernel's bitwise contracts, the learners on lambda-returns against tests/td_lambda_oracle.py in
both gemm modes, lambda = 0 against today's loss on all five learners, off-means-off, and graph replay.

Bounds: tests/parity.close at 1e-4 * max|ref| (+ 1e-7) for every tensor of a first update and for the kernel; 1e-3 for the
second update (RMSprop's first step amplifies rounding: tests/test_gpu_learners.py).  The probes and contracts compare bits."""
import numpy as np
import pytest
import torch

from oracle import seeded, learners
from golden_cases import CASES, build_oracle_state
import parity
import td_lambda_oracle as tl

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
LAM = 0.8


def _dev(*arrays):
    return [torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV) for a in arrays]


def run_kernel(q, r, term, padded, gamma, lam, tail=64):
    """ret as a (B, T) float32 array; the output buffer is `tail` floats longer and NaN-filled: the tail must stay NaN"""
    from marl_amd import ops
    B, T = q.shape
    out = torch.full((B * T + tail,), float("nan"), device=DEV)
    ops.td_lambda_returns(*_dev(q, r, term, padded), gamma, lam, out, B, T)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[B * T:]).all()), "the kernel wrote behind ret[0 : B*T]"
    assert not bool(torch.isnan(out[:B * T]).any())
    return out[:B * T].view(B, T).cpu().numpy()


@pytest.fixture(scope="module")
def cases(golden_dir):
    return tl.load_cases(golden_dir)


# ---------------------------------------------------------------------------------------------------- the kernel
def test_kernel_vs_reference_float64(cases):
    for key, lam, inputs, G, _ in cases:
        got = run_kernel(*inputs, tl.GAMMA, lam)
        parity.close("td_lambda:%s" % key, "G lam=%g" % lam, got, G, tol=1e-4)


def _integer_case(B, T, seed):
    """integer r in [-3, 3] and integer q everywhere (padded rows included), ragged lengths, one unterminated episode"""
    rng = np.random.default_rng(seed)
    q = rng.integers(-5, 6, size=(B, T)).astype(np.float32)
    r = rng.integers(-3, 4, size=(B, T)).astype(np.float32)
    term, padded = np.zeros((B, T), np.float32), np.zeros((B, T), np.float32)
    lengths = [int(x) for x in rng.integers(1, T + 1, size=B)]
    lengths[0] = T
    lengths[-1] = -1
    for b, L in enumerate(lengths):
        if L >= 0:
            term[b, L - 1:] = 1.0
            padded[b, L:] = 1.0
    return q, r, term, padded


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 128, 129])
def test_integer_sums_are_exact(T):
    """gamma = lambda = 1: every partial sum is an integer fp32 holds exactly, so a dropped, doubled or shifted step at a chunk
    seam shows as a wrong integer"""
    for B in (1, 3, 5, 9):
        inputs = _integer_case(B, T, seed=10 * T + B)
        ref = tl.returns(*inputs, 1.0, 1.0)
        assert np.abs(ref).max() < 2 ** 24
        np.testing.assert_array_equal(run_kernel(*inputs, 1.0, 1.0).astype(np.float64), ref, err_msg="B %d T %d" % (B, T))


@pytest.mark.parametrize("T", [64, 65, 129])
def test_single_reward_decays_by_exact_powers_of_two(T):
    """gamma = 1, lambda = 0.5, q = 0, r = 1 at one step k: ret[t] = 2^-(k - t) up to k, 0 behind it"""
    L = T - T // 4                                     # the ragged episode: k is its last real step
    ks = [0, T - 1, 63] + ([64] if T > 64 else []) + [L - 1]
    B = len(ks)
    q, r = np.zeros((B, T), np.float32), np.zeros((B, T), np.float32)
    term, padded = np.zeros((B, T), np.float32), np.zeros((B, T), np.float32)
    for b, k in enumerate(ks):
        r[b, k] = 1.0
    term[B - 1, L - 1:] = 1.0
    padded[B - 1, L:] = 1.0
    got = run_kernel(q, r, term, padded, 1.0, 0.5).astype(np.float64)
    t = np.arange(T)
    for b, k in enumerate(ks):
        d = k - t
        want = np.where(d >= 0, 2.0 ** -np.maximum(d, 0).astype(np.float64), 0.0)
        check = d <= 100
        np.testing.assert_array_equal(got[b][check], want[check], err_msg="T %d k %d" % (T, k))


def test_padded_rows_contribute_nothing(cases):
    rng = np.random.default_rng(1)
    for key, lam, (q, r, term, padded), _, _ in cases:
        base = run_kernel(q, r, term, padded, tl.GAMMA, lam)
        junk = lambda: tl.JUNK * np.where(rng.random(q.shape) < 0.5, -1.0, 1.0).astype(np.float32)
        q2, r2 = np.where(padded == 1, junk(), q), np.where(padded == 1, junk(), r)
        other = run_kernel(q2, r2, term, padded, tl.GAMMA, lam)
        assert base.tobytes() == other.tobytes(), (key, lam)


def test_two_calls_and_split_rows_give_the_same_bits(cases):
    for key, lam, (q, r, term, padded), _, _ in cases:
        one = run_kernel(q, r, term, padded, tl.GAMMA, lam)
        assert one.tobytes() == run_kernel(q, r, term, padded, tl.GAMMA, lam).tobytes(), (key, lam)
        a = run_kernel(q[:3], r[:3], term[:3], padded[:3], tl.GAMMA, lam)
        b = run_kernel(q[3:], r[3:], term[3:], padded[3:], tl.GAMMA, lam)
        assert one.tobytes() == np.concatenate([a, b]).tobytes(), (key, lam)


def test_more_episodes_than_resident_waves():
    """the grid-stride path: more episodes than one pass of the grid holds"""
    B, T = 8192 + 37, 5
    inputs = _integer_case(B, T, seed=4)
    np.testing.assert_array_equal(run_kernel(*inputs, 1.0, 1.0).astype(np.float64), tl.returns(*inputs, 1.0, 1.0))


def test_no_episodes_launch_nothing():
    from marl_amd import _lib, ops
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    assert lib.marl_td_lambda_returns(None, None, None, None, 0.99, 0.8, None, 0, 5, s) == 0      # null pointers: never looked at
    assert lib.marl_td_lambda_returns(None, None, None, None, 0.99, 0.8, None, 5, 0, s) == 0
    x = torch.ones(8, device=DEV)
    assert lib.marl_td_lambda_returns(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 0.99, 0.8, x.data_ptr(), 2, 4, s) != 0
    out = torch.full((4,), 3.0, device=DEV)
    e = torch.zeros(0, device=DEV)
    ops.td_lambda_returns(e, e, e, e, 0.99, 0.8, out, 0, 7)
    torch.cuda.synchronize()
    assert float(out.min()) == 3.0 and float(x.min()) == 1.0


# ---------------------------------------------------------------------------------------------------- the learners
def _case(name, **over):
    c = next(c for c in CASES if c[0] == name)
    return c[:6] + (dict(c[6], **over),)


@pytest.mark.parametrize("name", ["qmix_2s3z", "vdn_2s3z_nodq", "qplex_2s3z", "qmix_MMM2", "qtran_3s5z"])
def test_two_updates_on_lambda_returns_vs_oracle(name, gemm_mode):
    """qmix_2s3z: the fused loss fold, with an unterminated episode cut at max_episode_len (quirk Q2); vdn_2s3z_nodq: the
    marl_td_loss branch; qmix_MMM2: the wide fold; qtran_3s5z: the returns of joint_q_targets"""
    from test_gpu_learners import build_product, named_product_params
    case = _case(name, td_lambda=LAM)
    _, shape, alg, B, T, lengths, over = case
    args, mac, learner = build_product(case, gemm_mode)
    assert learner.td_lambda == LAM
    _, ost = build_oracle_state(case)
    for i, ts in enumerate((0, 1)):
        batch = seeded.make_batch(args, B, seed=100 + i, lengths=lengths)
        loss = learner.train(learners.clone_batch(batch), ts)
        oloss, ograds, ointer = tl.train(ost, learners.clone_batch(batch), ts, LAM)
        tol = 1e-4 if i == 0 else 1e-3
        c = "td_lambda_train:%s[%s]/step%d" % (name, gemm_mode, ts)
        assert learner.max_episode_len == ointer["T"]
        parity.close(c, "loss", loss, oloss, tol=tol)
        G = learner._dbg["td_targets"].view(B, -1).cpu().numpy()
        parity.close(c, "td_targets", G, ointer["td_targets"].numpy(), tol=tol)
        den = float(learner.last_stats[-1 if alg.startswith("qtran") else 1].item())
        assert den == float(ointer["den"])
        for n, p in named_product_params(learner):
            og = ograds.get(n)
            g = p.grad.detach().cpu().numpy() / den
            if og is None:
                assert not g.any(), n
                continue
            parity.close(c, "grad " + n, g, og.detach().numpy(), tol=tol)
        gn = float(torch.sqrt(learner.optimizer.sumsq[0]).item()) / den
        parity.close(c, "grad_norm", gn, ointer["grad_norm"], tol=tol)


def _q_learner(name):
    def make(lam):
        from test_gpu_learners import build_product
        case = _case(name) if lam is None else _case(name, td_lambda=lam)
        args, _, learner = build_product(case)
        batch = seeded.make_batch(args, case[3], seed=100, lengths=case[5])
        return learner, lambda: learner.train(learners.clone_batch(batch), 0)
    return make


def _world_learner(lam):
    import test_gpu_world as tw
    import world_oracle as wo
    c = wo.CASES[0]
    case = c if lam is None else c[:6] + (dict(c[6], td_lambda=lam),)
    args, _, learner = tw.build_product(case)
    batch = seeded.make_batch(args, case[3], seed=100, lengths=case[5])
    return learner, lambda: learner.train(learners.clone_batch(batch), 0)


def _maic_learner(aux):
    def make(lam):
        if aux:
            import test_gpu_maic_aux as tm
            import maic_aux_oracle as mo
        else:
            import test_gpu_maic_train as tm
            import maic_train_oracle as mo
        case = mo.UPDATE_CASES[0]
        args, _, learner = tm.build_product(case)
        assert learner.aux == aux
        if lam is not None:
            args.td_lambda = lam              # the seeded namespaces of these cases have no such field: set on the live learner
        batch, eps = mo.update_case_data(case)
        return learner, lambda: learner.train(learners.clone_batch(batch), 0, eps=eps)
    return make


FIVE = {"QLearner": _q_learner("qmix_2s3z"), "QTRANLearner": _q_learner("qtran_3s5z"), "QLearnerWithState": _world_learner,
        "MAICTDLearner": _maic_learner(False), "MAICTDLearner_aux": _maic_learner(True)}


def _one_update(make, lam):
    learner, step = make(lam)
    loss = float(step())
    stats = learner.last_stats[:learner.n_stats].cpu().numpy().astype(np.float64)
    grads = {n: p.grad.detach().cpu().numpy().copy() for n, p in enumerate(learner.params)}
    return loss, stats, grads


@pytest.mark.parametrize("kind", list(FIVE))
def test_lambda_zero_is_todays_loss(kind):
    """td_lambda 0.0 against td_lambda unset, two learners from the same seeds on the same batch: the statistics to 1e-6, every
    gradient to 1e-4 of its own scale (not the parameters: RMSprop's first step moves one by 10 lr sign(g), and a zero gradient's
    sign is rounding).  0.8 on the same batch is another loss."""
    loss_n, stats_n, grads_n = _one_update(FIVE[kind], None)
    loss_0, stats_0, grads_0 = _one_update(FIVE[kind], 0.0)
    np.testing.assert_allclose(stats_0, stats_n, rtol=1e-6, atol=0)
    assert abs(loss_0 - loss_n) <= 1e-6 * abs(loss_n)
    for n in grads_n:
        parity.close("td_lambda_zero:" + kind, "grad %d" % n, grads_0[n], grads_n[n], tol=1e-4)
    loss_8, _, _ = _one_update(FIVE[kind], LAM)
    assert abs(loss_8 - loss_n) > 1e-3 * abs(loss_n)


@pytest.mark.parametrize("kind", list(FIVE))
def test_off_means_off(kind, monkeypatch):
    from marl_amd import ops

    def boom(*a, **k):
        raise AssertionError("td_lambda_returns was called with td_lambda unset")
    monkeypatch.setattr(ops, "td_lambda_returns", boom)
    learner, step = FIVE[kind](None)
    assert learner.td_lambda is None
    assert np.isfinite(float(step()))
    assert "td_targets" not in learner._dbg
    if kind == "QLearner":                   # and the patch does sit on the path
        learner, step = FIVE[kind](LAM)
        with pytest.raises(AssertionError):
            step()


@pytest.mark.parametrize("bad", [1.5, -0.1])
def test_out_of_range_raises_at_construction(bad):
    from test_gpu_learners import build_product
    for name in ("qmix_2s3z", "qtran_3s5z"):
        with pytest.raises(ValueError):
            build_product(_case(name, td_lambda=bad))


# ---------------------------------------------------------------------------------------------------- graph replay
def _ring_run(alg, gemm_mode, mode, updates, flips=None):
    """tests/test_gpu_edges.py:test_hip_graph_replay_equals_eager's loop with args.td_lambda set; flips: {update: td_lambda}"""
    import bench
    from marl_amd.controller.share_params import SharedMAC
    from marl_amd.algorithm.q_learner import QLearner
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    from marl_amd.common.replaybuffer import ReplayBuffer
    args = bench.make_args(alg, "2s3z", 12)
    E = 96
    args.buffer_size, args.batch_size, args.hip_graph, args.gemm_mode = 2 * E, E, mode, gemm_mode
    args.td_lambda = LAM
    torch.manual_seed(0)
    np.random.seed(7)
    mac = SharedMAC(args)
    learner = QLearner(mac, args)
    env = SyntheticSMACEnv(E, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, 12, seed=3, fixed_length=True)
    w = RolloutWorker(env, mac, args)
    buf = ReplayBuffer(args)
    w.record_sink = buf
    losses, captured = [], []
    for i in range(updates):
        if flips and i in flips:
            args.td_lambda = flips[i]
        ep = w.generate_episodes(E)[0]
        buf.store_episode(ep)
        losses.append(learner.train(buf.sample(E), i))
        if mode:
            captured.append(any(e["graph"] is not None for e in learner.graphs.entries.values()))
    return learner, losses, captured, learner._flat.flat.detach().cpu().numpy().copy()


@pytest.mark.parametrize("alg,gemm_mode", [("qmix", "bf16x6"), ("qplex", "f32")])
def test_hip_graph_replay_equals_eager_on_lambda_returns(alg, gemm_mode):
    out = {}
    for mode in (False, True):
        learner, losses, captured, flat = _ring_run(alg, gemm_mode, mode, 8)
        out[mode] = (losses, flat)
        assert "td_targets" in learner._dbg
        if mode:
            g = learner.graphs
            assert not g.disabled, getattr(g, "error", "")
            assert captured[-1], "no graph was captured"
            assert g.replays >= 5
        else:
            assert learner.graphs is None
    assert out[False][0] == out[True][0]
    np.testing.assert_array_equal(out[False][1], out[True][1])


def test_flipping_td_lambda_drops_the_captured_graph():
    """td_lambda is one of GraphedUpdate.SCHEDULE_ARGS: a graph captured with one value is not replayed with another"""
    flips = {5: 0.3}
    _, eager, _, flat_e = _ring_run("qmix", "f32", False, 9, flips)
    learner, graphed, captured, flat_g = _ring_run("qmix", "f32", True, 9, flips)
    assert not learner.graphs.disabled, getattr(learner.graphs, "error", "")
    assert captured[4] and not captured[5] and captured[8], captured
    assert learner.td_lambda == 0.3
    assert eager == graphed
    np.testing.assert_array_equal(flat_e, flat_g)
