"""Sampled training rollouts on the MI355X: the whole-rollout kernel and the fused step drawing their actions from the stochastic
policy (csrc/rollout_fused.hip synth_rollout_kernel<AC, true>, csrc/rollout.hip synth_fused_step_kernel<true>).

Bounds.  Against float64 (tests/sample_rollout_cases.step_check) a live cell whose draw lies at least policy_oracle.SAMPLER_EXCLUDE
= 1e-5 from every float64 CDF boundary must carry the float64 action; the excluded share stays below SAMPLER_CAP = 0.5 % (the
kernel test's rule, tests/test_gpu_policy.py).  Between the device paths the record fields that do not depend on the actions are
equal bit for bit; the fused step and the unfused path see the same logits tensor and call the same function, so u and r are equal
everywhere; the whole-rollout kernel's logits come from its own fc2 tile, so u is held equal on every cell whose row made no
near-boundary draw so far (prefix-clean), r where all N cells of the step are, and fewer than 5 % of the live cells may be left out
(tests/test_sample_rollout_cpu.py holds the float64 rollout alone to half of both caps)."""
import numpy as np
import pytest
import torch

import policy_oracle as po
import sample_rollout_cases as src

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("obs", "state", "avail", "u", "r", "term", "padded", "length", "won")
INVALID = 1          # hipErrorInvalidValue


def _setup(c, gemm_mode="f32"):
    from marl_amd.controller.share_params import PolicyMAC
    args = src.make_args(c)
    args.gemm_mode = gemm_mode
    agent = src.agent_weights(c, args)
    mac = PolicyMAC(args)
    mac.agent.load_state_dict({k: torch.tensor(v) for k, v in agent.items()})
    mac.cuda()
    return args, {k: torch.tensor(v, dtype=torch.float64) for k, v in agent.items()}, mac


def _env(c, args):
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    return SyntheticSMACEnv(c["E"], args.n_agents, args.obs_shape, args.state_shape, args.n_actions, c["T"], seed=src.ENV_SEED,
                            env0=src.ENV0)


def _worker(c, args, mac, mode=None):
    from marl_amd.rollout import RolloutWorker
    env = _env(c, args)
    w = RolloutWorker(env, mac, args)
    if mode is not None:
        w.rollout_mode = mode
    return w, env


def _check_against_float64(c, args, p64, w, env):
    """one training rollout of ``w``, held to the float64 policy step by step"""
    E, T, N, A = c["E"], c["T"], args.n_agents, args.n_actions
    eps_of_t, eps_after = src.eps_schedule(args, w.epsilon, T)
    ep, rew, wins, steps = w.generate_episodes(E)
    # the whole-rollout kernel ran: it wrote the per-episode statistics itself
    assert getattr(env, "_stats_ring", None) and ep.record.kernel_stats is None
    rec = ep.record
    np.testing.assert_allclose(rew, rec.r.sum(1).cpu().numpy(), atol=1e-5)
    assert steps == int(rec.length.sum().item()) and list(wins) == [bool(x) for x in rec.won.cpu().tolist()]
    np.testing.assert_allclose(w.epsilon, eps_after, rtol=1e-12)
    want, margin, live = src.step_check(rec, p64, args, eps_of_t, src.RSEED, env)
    u = rec.u.cpu().numpy().astype(np.int64)
    avail = rec.avail.cpu().numpy()[:, :T]
    live3 = np.broadcast_to(live[..., None], u.shape)
    assert (u[~live3] == -1).all() and (u[live3] >= 0).all() and (u[live3] < A).all()
    assert bool((rec.padded.cpu().numpy() == ~live).all())
    assert (np.take_along_axis(avail, np.maximum(u, 0)[..., None], -1)[..., 0][live3] == 1).all()
    far = live3 & (margin >= po.SAMPLER_EXCLUDE)
    n_live, n_near = int(live3.sum()), int((live3 & ~far).sum())
    wrong = int((u[far] != want[far]).sum())
    print(c["name"], "episode", env.episode, "live", n_live, "near", n_near, "wrong", wrong)
    assert wrong == 0
    assert n_near < po.SAMPLER_CAP * n_live
    return rec


@pytest.mark.parametrize("c", src.CASES, ids=src.CASE_IDS)
def test_whole_rollout_samples_the_float64_policy(c):
    args, p64, mac = _setup(c)
    w, env = _worker(c, args, mac)
    _check_against_float64(c, args, p64, w, env)
    assert env.episode == 0
    _check_against_float64(c, args, p64, w, env)        # the second rollout continues the episode counter and the schedule
    assert env.episode == 1


@pytest.mark.parametrize("c", src.CASES, ids=src.CASE_IDS)
def test_three_paths_one_record(c):
    args, p64, mac = _setup(c)
    E, T = c["E"], c["T"]
    recs, envs = {}, {}
    for mode in ("whole", "fused_step", "unfused"):
        w, env = _worker(c, args, mac, mode)
        eps_of_t, _ = src.eps_schedule(args, w.epsilon, T)
        recs[mode] = w.generate_episodes(E)[0].record
        envs[mode] = env
    assert getattr(envs["whole"], "_stats_ring", None) and not getattr(envs["fused_step"], "_stats_ring", None)
    for mode in ("whole", "fused_step"):
        for f in ("obs", "state", "avail", "length", "won", "term", "padded"):
            assert torch.equal(getattr(recs[mode], f), getattr(recs["unfused"], f)), (mode, f)
    for f in ("u", "r"):
        assert torch.equal(getattr(recs["fused_step"], f), getattr(recs["unfused"], f)), f
    _, margin, live = src.step_check(recs["unfused"], p64, args, eps_of_t, src.RSEED, envs["unfused"])
    clean = src.prefix_clean(margin, live)
    live3 = np.broadcast_to(live[..., None], clean.shape)
    uw, uu = recs["whole"].u.cpu().numpy(), recs["unfused"].u.cpu().numpy()
    rw, ru = recs["whole"].r.cpu().numpy(), recs["unfused"].r.cpu().numpy()
    n_live, left_out = int(live3.sum()), int((live3 & ~clean).sum())
    print(c["name"], "live", n_live, "left out", left_out, "cells that disagree anywhere", int((uw != uu).sum()),
          "rewards that disagree", int((rw != ru).sum()))
    assert (uw[live3 & clean] == uu[live3 & clean]).all() and (uw[~live3] == uu[~live3]).all()
    step_clean = clean.all(-1) & live
    assert (rw[step_clean].view(np.uint32) == ru[step_clean].view(np.uint32)).all() and (rw[~live] == ru[~live]).all()
    assert left_out < 0.05 * n_live


def _record(E, T, N, O, S, A, state_ld=0, **tensors):
    """a MarlRecord by reference: the sizes, and the data pointers of `tensors` (the other fields NULL)"""
    import ctypes
    from marl_amd import _lib
    return ctypes.byref(_lib.MarlRecord(state_ld=state_ld, E=E, T=T, N=N, O=O, S=S, A=A, **{k: t.data_ptr() for k, t in tensors.items()}))


def test_entry_points_zero_sizes_and_invalid_shapes():
    from marl_amd import _lib
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    roll = lambda E, T, N, A: lib.marl_synth_rollout_sample(None, _record(E, T, N, 80, 120, A), 1, 2, 0, 0, 0, None, None, None,
                                                            0.3, 0.0, 0.0, 1, 1, s)
    step = lambda E, N, A: lib.marl_synth_fused_step_sample(1, 2, 0, 0, 0, 0.3, None, _record(E, 8, N, 80, 120, A, state_ld=120), s)
    assert roll(0, 8, 5, 11) == 0 and roll(4, 0, 5, 11) == 0 and step(0, 5, 11) == 0        # nothing to do: nothing launched
    assert roll(4, 8, 5, 33) == INVALID and roll(4, 8, 65, 11) == INVALID and roll(4, 8, 0, 11) == INVALID
    assert step(4, 65, 11) == INVALID          # (the fused step has no bound on A: marl_synth_fused_step's checks)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["2s3z-e03", "MMM2"])
def test_entry_points_are_deterministic(name):
    c = next(x for x in src.CASES if x["name"] == name)
    args, _, mac = _setup(c)
    E, T, N, A, H = c["E"], c["T"], args.n_agents, args.n_actions, args.rnn_hidden_dim
    out = []
    for _ in range(2):
        env = _env(c, args)
        rec = env.new_record()
        h = torch.empty(E * N, H, device=DEV)
        env.whole_rollout(mac.agent.weights(), None, src.RSEED, rec, args.last_action, args.reuse_network, h_out=h,
                          eps_sched=(0.3, 0.03, 0.02), sample=True)
        torch.cuda.synchronize()
        out.append([getattr(rec, f).cpu().numpy().tobytes() for f in FIELDS] + [h.cpu().numpy().tobytes(),
                                                                                rec.kernel_stats.cpu().numpy().tobytes()])
    assert out[0] == out[1]
    # the fused step on fixed logits
    q = torch.tensor(np.random.default_rng(3).standard_normal((E, 1, N, A)).astype(np.float32) * 2.0, device=DEV)
    out = []
    for _ in range(2):
        env = _env(c, args)
        rec = env.new_record()
        env.begin_episode(rec)
        env.observe(0, rec)
        env.fused_step(0, q, 0.3, src.RSEED, rec, sample=True)
        torch.cuda.synchronize()
        out.append([getattr(rec, f).cpu().numpy().tobytes() for f in FIELDS])
    assert out[0] == out[1]
    u0 = np.frombuffer(out[0][3], np.int32).reshape(E, T, N)[:, 0]
    av0 = rec.avail.cpu().numpy()[:, 0]
    want, margin, _ = po.sample(q.view(E, N, A).cpu().numpy(), av0, None, 0.3, src.RSEED, env.env0, env.global_step(0))
    far = margin >= po.SAMPLER_EXCLUDE
    assert (u0[far] == want[far]).all() and float((~far).mean()) < po.SAMPLER_CAP
    assert (np.take_along_axis(av0, u0[..., None].astype(np.int64), -1) == 1).all()


def test_bf16x6_mode_samples_with_the_same_kernel():
    c = next(x for x in src.CASES if x["name"] == "2s3z-e03")
    recs = []
    for mode in ("f32", "bf16x6"):
        args, _, mac = _setup(c, mode)
        w, env = _worker(c, args, mac)
        recs.append(w.generate_episodes(c["E"])[0].record)
        assert getattr(env, "_stats_ring", None)
    for f in FIELDS:
        assert torch.equal(getattr(recs[0], f), getattr(recs[1], f)), f


# ---------------------------------------------------------------------------------------------------- controllers with a head
@pytest.mark.parametrize("alg,cls", [("reinforce+commnet", "CommNetMAC"), ("reinforce+g2anet", "G2ANetMAC")])
def test_head_controllers_fused_sampled_step_equals_the_unfused_path(alg, cls):
    """the default training rollout of a controller with a head and the one with rollout_mode = "fused_step" (the sampling fused
    step: two launches fewer per lock-step) against the three-launch reference path, bit for bit"""
    from marl_amd.controller import share_params
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    from marl_amd.main import build
    from marl_amd.rollout import RolloutWorker
    from marl_amd import ops
    args, _ = build(["--map", "2s3z", "--alg", alg, "--n_envs", "8"])
    args.episode_limit = 8
    torch.manual_seed(6)
    mac = getattr(share_params, cls)(args)
    recs, sampled = {}, {}
    real = ops.synth_fused_step
    for mode in (None, "fused_step", "unfused"):
        env = SyntheticSMACEnv(8, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, 8, seed=args.seed)
        w = RolloutWorker(env, mac, args)
        if mode is not None:
            w.rollout_mode = mode
        calls = []
        ops.synth_fused_step = lambda *a, **k: (calls.append(k.get("sample", False)), real(*a, **k))[1]
        try:
            recs[mode] = w.generate_episodes(8)[0].record
        finally:
            ops.synth_fused_step = real
        sampled[mode] = calls
        with pytest.raises(RuntimeError):
            w.launch_episodes()
    assert sampled["fused_step"] == [True] * 8 and sampled["unfused"] == []
    assert bool((recs["unfused"].u >= 0).any())
    for mode in (None, "fused_step"):
        for f in FIELDS:
            assert torch.equal(getattr(recs[mode], f), getattr(recs["unfused"], f)), (mode, f)


# ---------------------------------------------------------------------------------------------------- the runner
@pytest.mark.parametrize("alg", ["central_v", "reinforce", "coma", "mappo"])
def test_runner_trains_on_whole_sampled_rollouts(alg, tmp_path):
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    from marl_amd.main import build, make_runner
    from marl_amd.utils.logging import Logger
    args, _ = build(["--map", "2s3z", "--alg", alg, "--n_envs", "8", "--n_steps", "1", "--evaluate_epoch", "8",
                     "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "model")])
    args.episode_limit = 8
    env = SyntheticSMACEnv(8, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, 8, seed=args.seed)
    torch.manual_seed(3)
    r = make_runner(args, env, Logger())
    seen = []
    whole = env.whole_rollout
    env.whole_rollout = lambda *a, **k: (seen.append(bool(k.get("sample", False))), whole(*a, **k))[1]
    p0 = r.learner._flat.flat.clone()
    loss = r.run(0)                     # one training rollout + update, then the closing evaluation
    assert r.train_steps == 1 and np.isfinite(float(loss)) and not torch.equal(p0, r.learner._flat.flat)
    assert seen.count(True) == 1 and len(seen) >= 2               # the training rollout sampled in the kernel; evaluation is greedy
    assert getattr(env, "_stats_ring", None)


def test_null_record_is_refused_and_unread_fields_may_be_absent():
    """the record struct's two rules at the smallest shape that reaches them: every synthetic entry refuses rec = NULL before it looks
    at anything else (the weights are NULL too), and marl_synth_step runs with obs / state / avail absent, to the same bits"""
    from marl_amd import _lib, ops
    from marl_amd.env.synthetic_smac import EpisodeRecord
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    for fn in (lib.marl_synth_rollout, lib.marl_synth_rollout_sample, lib.marl_synth_rollout_x6):
        assert fn(None, None, 1, 2, 0, 0, 0, None, None, None, 0.3, 0.0, 0.0, 1, 1, s) == INVALID
    for fn in (lib.marl_synth_fused_step, lib.marl_synth_fused_step_sample):
        assert fn(1, 2, 0, 0, 0, 0.3, None, None, s) == INVALID
    assert lib.marl_synth_observe(1, 0, 0, 0, None, s) == INVALID and lib.marl_synth_step(1, 0, 0, 0, None, None, None, s) == INVALID
    E, T, N, O, S, A = 3, 4, 2, 4, 5, 3
    full, bare = EpisodeRecord(E, T, N, O, S, A, DEV), EpisodeRecord(E, T, N, O, S, A, DEV)
    assert full.state.stride(-2) == 8
    bare.obs = bare.state_store = bare.avail = None
    act = torch.tensor([[0, 2], [1, 1], [2, 0]], dtype=torch.int32, device=DEV)
    alive = {}
    for rec in (full, bare):
        ops.synth_lengths(src.ENV_SEED, 0, 0, rec.length, rec.won, E, T)
        alive[rec] = torch.full((T, E), -9, dtype=torch.int32, device=DEV)
        for t in range(T):
            ops.synth_step(src.ENV_SEED, 0, 0, t, act, rec, alive[rec][t])
    torch.cuda.synchronize()
    assert (full.u >= 0).any().item()                    # (the steps ran: u starts at -1)
    for f in ("u", "r", "term", "padded", "length", "won"):
        assert torch.equal(getattr(full, f), getattr(bare, f)), f
    assert torch.equal(alive[full], alive[bare])
