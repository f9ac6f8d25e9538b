"""The battle environment's fused step (csrc/battle.hip) and whole-rollout kernel (csrc/battle_rollout.hip) on the MI355X.

Every comparison is exact.  The three rollout paths of a RolloutWorker over FusedBattleEnv - the persistent kernel, the agent step +
fused step, and agent step + select / policy_sample + step - see the same q bit for bit (the kernel issues the T = 1 unroll's MFMA
sequences) and make the same draws, and the rules are integer arithmetic with one correctly rounded fp32 operation per feature, so
``torch.equal`` holds on every field and on the unit state.  The rules are then checked independently of the agent: the numpy oracle
(tests/battle_oracle.py) replays the actions the kernel recorded and must reproduce every other field."""
import types

import numpy as np
import pytest
import torch

import battle_oracle as bo
from oracle import seeded

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
MODES = ("whole", "fused_step", "unfused")
RSEED = 77
_cache = {}


def _fields():
    from marl_amd.env.synthetic_smac import EpisodeRecord
    return EpisodeRecord.FIELDS          # the nine: obs, state_store, avail, u, r, term, padded, length, won


def _args(name, T=None, eps=0.5, alg="qmix", last_action=True, reuse_network=True):
    from marl_amd.env.battle import battle_shapes
    N, O, S, A, T0 = battle_shapes(name)
    a = seeded.make_args("2s3z", alg, episode_limit=T or T0, n_agents=N, obs_shape=O, state_shape=S, n_actions=A, map=name,
                         epsilon=eps, seed=RSEED, last_action=last_action, reuse_network=reuse_network, env="battle")
    a.anneal_epsilon = 0.01
    a.gemm_mode = "f32"
    return a


def _mac(args, policy=False, scale=3.0, bias=None):
    from marl_amd.controller.share_params import PolicyMAC, SharedMAC
    agent = seeded.seeded_state(seeded.agent_param_shapes(args), seed=11, scale=scale)
    if bias is not None:
        agent["fc2.bias"] = (agent["fc2.bias"] + bias).astype(np.float32)
    mac = (PolicyMAC if policy else SharedMAC)(args)
    mac.agent.load_state_dict({k: torch.tensor(v) for k, v in agent.items()})
    mac.cuda()
    return mac


def _scribble(rec):
    """every field a kernel must write holds garbage first (the state's pad columns are allocated zero and left alone)"""
    for k in ("obs", "avail", "r", "term", "padded"):
        getattr(rec, k).fill_(float("nan"))
    rec.state.fill_(float("nan"))
    for k in ("u", "length", "won"):
        getattr(rec, k).fill_(-7)


def _clean(rec):
    for k in ("obs", "state", "avail", "r", "term", "padded"):
        assert not torch.isnan(getattr(rec, k)).any().item(), k
    for k in ("u", "length", "won"):
        assert not (getattr(rec, k) == -7).any().item(), k


def _play(name, E, mode, *, seed=5, env0=0, T=None, eps=0.5, evaluate=False, policy=False, last_action=True, reuse_network=True,
          rollouts=2, plain=False, scale=3.0, bias=None, scribble=False):
    """`rollouts` rollouts of one worker; per rollout the record, the unit state, the hidden state, the worker's epsilon and the
    kernel's statistics (whole path)"""
    from marl_amd.env.battle import BattleEnv, FusedBattleEnv
    from marl_amd.rollout import RolloutWorker
    args = _args(name, T, eps, "central_v" if policy else "qmix", last_action, reuse_network)
    mac = _mac(args, policy, scale, bias)
    env = BattleEnv(E, name, seed=seed, env0=env0) if plain else FusedBattleEnv(E, name, seed=seed, env0=env0, episode_limit=T)
    if scribble:
        fresh = env.new_record

        def new_record():
            rec = fresh()
            _scribble(rec)
            return rec
        env.new_record = new_record
    w = RolloutWorker(env, mac, args)
    w.rollout_mode = mode
    out = []
    for k in range(rollouts):
        ep, rew, wins, steps = w.generate_episodes(E, evaluate=evaluate)
        assert env.episode == k
        ring = getattr(env, "_stats_ring", None)
        assert bool(ring) == (mode == "whole" and not plain), "the path that ran is not the one asked for"
        rec = ep.record
        assert steps == int(rec.length.sum().item()) and list(wins) == [bool(x) for x in rec.won.cpu().tolist()]
        np.testing.assert_allclose(rew, rec.r.sum(1).cpu().numpy(), rtol=1e-6, atol=1e-6)
        out.append(types.SimpleNamespace(rec=rec, units=env.units.clone(), h=mac.hidden_states.clone(), eps=w.epsilon,
                                         stats=ring[env._stats_i].clone() if ring else None, env=env))
    return out


def _three(name, E, **kw):
    """the three paths of a case, played once and shared: read-only"""
    key = (name, E, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = {mode: _play(name, E, mode, **kw) for mode in MODES}
    return _cache[key]


def _same(a, b, what):
    for f in _fields():
        assert torch.equal(getattr(a.rec, f), getattr(b.rec, f)), (what, f)
    assert torch.equal(a.units, b.units), (what, "units")
    assert a.eps == b.eps, (what, "epsilon")


CASES = [("3m", 3, {}),                                # a partly filled tile
         ("3m", 65, {}),
         ("3m", 65, dict(eps=0.0, evaluate=True)),
         ("3m", 65, dict(eps=1.0)),
         ("3m", 65, dict(last_action=False)),
         ("3m", 65, dict(reuse_network=False)),
         ("3m", 257, {}),                              # two environments per workgroup, a ragged last workgroup
         ("3m", 1281, {}),                             # six: 18 rows, an environment across two row tiles, a last workgroup of three
         ("2s3z", 65, dict(env0=7)),
         ("3s5z", 3, {}),
         ("3s5z", 37, {})]


@pytest.mark.parametrize("name,E,kw", CASES, ids=["%s-E%d%s" % (n, e, "".join("-%s=%s" % i for i in sorted(k.items()))) for n, e, k in CASES])
def test_three_paths_one_record(name, E, kw):
    from marl_amd import ops
    from marl_amd.env.battle import battle_shapes
    N, O, S, A, T = battle_shapes(name)
    assert ops.battle_rollout_plan(E, N, O, A, kw.get("last_action", True), kw.get("reuse_network", True))[1] == (E + 255) // 256
    runs = _three(name, E, **kw)
    for k in range(2):                                 # the second rollout: the episode counter and the continued epsilon
        _clean(runs["whole"][k].rec)
        for mode in ("fused_step", "unfused"):
            _same(runs["whole"][k], runs[mode][k], (mode, k))
    assert not torch.equal(runs["whole"][0].rec.obs[:, 0], runs["whole"][1].rec.obs[:, 0])       # another episode's start
    u = runs["whole"][0].rec.u
    if not kw.get("evaluate"):
        assert len({tuple(x) for x in u[:, 0].cpu().tolist()}) > 1 or E < 4


def test_a_plain_battle_env_records_the_same():
    runs = _three("3m", 65)
    plain = _play("3m", 65, "whole", plain=True)       # BattleEnv has neither attribute: the three-launch path
    assert not hasattr(plain[0].env, "fused_step") and not hasattr(plain[0].env, "whole_rollout")
    for k in range(2):
        _same(runs["whole"][k], plain[k], ("plain", k))


@pytest.mark.parametrize("name,E", [("3m", 65), ("3s5z", 37)])
def test_sampling_three_paths_one_record(name, E):
    """PolicyMAC's training rollouts: the whole kernel's SAMPLE block, the sampling fused step, policy_sample + step"""
    runs = _three(name, E, policy=True)
    for k in range(2):
        _clean(runs["whole"][k].rec)
        for mode in ("fused_step", "unfused"):
            a, b = runs["whole"][k].rec.u, runs[mode][k].rec.u
            print(name, E, mode, k, "actions that differ:", int((a != b).sum().item()), "of", a.numel())
            _same(runs["whole"][k], runs[mode][k], (mode, k))
    greedy = _three(name, E, eps=0.0, evaluate=True)["whole"][0]
    assert not torch.equal(runs["whole"][0].rec.u, greedy.rec.u)                 # the draws are not the argmax


def test_an_evaluation_rollout_of_the_policy_is_the_greedy_one():
    ev = {mode: _play("3m", 65, mode, policy=True, eps=0.3, evaluate=True, rollouts=1)[0] for mode in MODES}
    q = _three("3m", 65, eps=0.0, evaluate=True)["whole"][0]
    for mode in MODES:
        for f in _fields():
            assert torch.equal(getattr(ev[mode].rec, f), getattr(q.rec, f)), (mode, f)
        assert torch.equal(ev[mode].units, q.units), mode


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


@pytest.mark.parametrize("name,E,kw", [("3m", 1281, {}), ("2s3z", 65, dict(env0=7)), ("3s5z", 37, {})])
def test_the_oracle_replays_the_recorded_actions(name, E, kw):
    """the rules, independently of the agent: the recorded u as a script"""
    runs = _three(name, E, **kw)["whole"]
    for episode in (0, 1) if E < 100 else (1,):
        got = runs[episode]
        u = got.rec.u.cpu().numpy()
        want = bo.play(name, E, 5, script=u, env0=kw.get("env0", 0), episode=episode)
        for f in ("obs", "state", "avail", "u", "r", "term", "padded", "length", "won"):
            g = getattr(got.rec, f).cpu().numpy()
            assert g.dtype == want[f].dtype and g.shape == want[f].shape, f
            bad = _bits(g) != _bits(want[f])
            assert not bad.any(), (name, episode, f, int(bad.sum()), np.argwhere(bad)[0])
        np.testing.assert_array_equal(got.units.cpu().numpy(), want["units"])


def _endings(run):
    rec = run.rec
    return bo.endings(dict(u=rec.u.cpu().numpy(), units=run.units.cpu().numpy(), won=rec.won.cpu().numpy(),
                           length=rec.length.cpu().numpy()))


def _attack_bias(A):
    b = np.zeros(A, np.float32)
    b[6:] = 10.0           # the attacks first,
    b[4] = 5.0             # then "move east"
    return b


def test_endings_a_win_a_loss_and_a_time_limit():
    # random weights lose: the enemies walk up and fire
    lost = _endings(_three("3m", 65)["whole"][0])
    assert lost[1] > 0
    # attack whoever is in range, else walk east: wins occur
    won = {mode: _play("3m", 65, mode, eps=0.0, evaluate=True, scale=1.0, bias=_attack_bias(9), rollouts=1) for mode in MODES}
    for mode in ("fused_step", "unfused"):
        _same(won["whole"][0], won[mode][0], ("biased", mode))
    ends = _endings(won["whole"][0])
    print("biased 3m E65 (wins, losses, limits):", ends, "random:", lost)
    assert ends[0] > 0
    assert int(won["whole"][0].rec.won.sum().item()) == ends[0]
    r = won["whole"][0].rec.r.sum(1)[won["whole"][0].rec.won == 1]
    assert torch.allclose(r, torch.full_like(r, 20.0), atol=1e-3)           # a won episode's rewards sum to 20 (env/battle.py)
    # a time limit below the shortest fight: every episode ends at it
    lim = _three("3m", 65, T=8)
    for mode in MODES:
        rec = lim[mode][0].rec
        assert (rec.length == 8).all().item() and (rec.term[:, 7] == 1).all().item() and not rec.won.any().item()
        assert not rec.term[:, :7].any().item() and not rec.padded.any().item()
    assert _endings(lim["whole"][0])[2] == 65
    for k in range(2):
        for mode in ("fused_step", "unfused"):
            _same(lim["whole"][k], lim[mode][k], ("limit", mode, k))


def test_statistics_and_the_final_hidden_state():
    for key, kw in ((("3m", 1281), {}), (("3s5z", 37), {}), (("3m", 65), dict(T=8))):
        runs = _three(*key, **kw)
        for k in range(2):
            w = runs["whole"][k]
            r = w.rec.r.cpu().numpy()
            want = np.cumsum(r, axis=1, dtype=np.float32)[:, -1]
            stats = w.stats.cpu().numpy()
            assert (_bits(stats[0]) == _bits(want)).all(), key
            np.testing.assert_array_equal(stats[1], w.rec.won.cpu().numpy().astype(np.float32))
            np.testing.assert_array_equal(stats[2], w.rec.length.cpu().numpy().astype(np.float32))
    lim = _three("3m", 65, T=8)                        # every episode runs to T: the hidden state is the per-step path's everywhere
    for k in range(2):
        assert (lim["whole"][k].rec.length == 8).all().item()
        for mode in ("fused_step", "unfused"):
            assert torch.equal(lim["whole"][k].h, lim[mode][k].h), (mode, k)
    # episodes that end early: the kernel feeds the input tile what the record holds (the final observation, then zeros), as the
    # per-step path reads it, so the hidden state is equal there as well
    full = _three("3m", 65)
    assert (full["whole"][0].rec.length < full["whole"][0].rec.T).any().item()
    for k in range(2):
        for mode in ("fused_step", "unfused"):
            assert torch.equal(full["whole"][k].h, full[mode][k].h), (mode, k)


@pytest.mark.parametrize("policy", [False, True])
def test_every_element_is_written_over_garbage(policy):
    want = _three("3m", 65, policy=policy)
    for mode in MODES:
        got = _play("3m", 65, mode, policy=policy, scribble=True, rollouts=1)[0]
        _clean(got.rec)
        _same(got, want[mode][0], ("scribbled", mode))


def test_a_rollout_into_the_replay_ring_leaves_the_other_slots_alone():
    from marl_amd.common.replaybuffer import ReplayBuffer
    from marl_amd.env.battle import FusedBattleEnv
    from marl_amd.env.synthetic_smac import EpisodeRecord
    from marl_amd.rollout import RolloutWorker
    want = _three("3m", 3)["whole"][0]
    args = _args("3m")
    env = FusedBattleEnv(3, "3m", seed=5)
    buf = ReplayBuffer(types.SimpleNamespace(buffer_size=8, **env.get_env_info()))
    buf.current_idx = buf.current_size = 3
    probe = buf.next_slot_record(3, env.episode_limit, env.n_agents, env.obs_shape, env.state_shape, env.n_actions, DEV)
    ring = buf.record
    assert probe is not None and probe.sink_slot == 3 and probe.obs.data_ptr() % 16 == 8      # a view that starts off a 16-byte line
    _scribble(ring)
    before = ring.clone()
    w = RolloutWorker(env, _mac(args), args)
    w.record_sink = buf
    ep = w.generate_episodes(3)[0]
    rec = ep.record
    assert getattr(rec, "sink_slot", None) == 3 and rec.obs.data_ptr() == ring.obs[3].data_ptr()
    _clean(rec)
    for f in EpisodeRecord.FIELDS:
        assert torch.equal(getattr(rec, f), getattr(want.rec, f)), f
        for sl in (slice(0, 3), slice(6, 8)):
            a, b = getattr(ring, f)[sl], getattr(before, f)[sl]
            assert torch.equal(torch.nan_to_num(a.float(), nan=-3.0), torch.nan_to_num(b.float(), nan=-3.0)), f
    assert torch.equal(env.units, want.units)


def test_refusals_write_nothing():
    import ctypes as C
    from marl_amd import _lib, ops
    lib = _lib.load()
    E, T, N, M, A, O, S = 2, 3, 3, 3, 9, 30, 48
    args = _args("3m")
    mac = _mac(args)                                   # (held: the struct points into its tensors)
    wts = mac.agent.weights()
    f = lambda *s: torch.full(s, 5.0, device=DEV)
    i = lambda *s: torch.full(s, 5, dtype=torch.int32, device=DEV)
    obs, state, avail, units, u = f(E, T + 1, N, O), f(E, T + 1, S), f(E, T + 1, N, A), i(E, N + M, 5), i(E, T, N)
    r, term, padded, length, won, h, stats, q = f(E, T), f(E, T), f(E, T), i(E), i(E), f(E * N, 64), f(3, E), f(E, 1, N, A)
    p = lambda t: C.c_void_p(t.data_ptr())
    INVALID = 1

    fields = dict(obs=obs, state=state, avail=avail, u=u, r=r, term=term, padded=padded, length=length, won=won)

    def record(sl, n, a):
        """the MarlRecord of the tensors above with these sizes, by reference"""
        return C.byref(_lib.MarlRecord(state_ld=sl, E=E, T=T, N=n, O=O, S=S, A=a, **{k: t.data_ptr() for k, t in fields.items()}))

    def whole(fn, types_=0, sl=S, n=N, m=M, a=A, tb=0):
        return fn(C.byref(wts), record(sl, n, a), 1, 2, 0, 0, types_, 0, tb, 0.1, p(units), p(h), p(stats), 0.5, 0.0, 0.05, m, 1, 1,
                  None)

    def step(fn, t=0, sl=S, n=N, m=M, a=A):
        return fn(0, 0, 0, 0.1, 2, 0, 0, t, 0.5, p(q), p(units), record(sl, n, a), m, None)
    for fn in (lib.marl_battle_rollout, lib.marl_battle_rollout_sample):
        assert whole(fn, sl=S - 1) == INVALID                   # battle_cfg's checks: the state's row stride,
        assert whole(fn, n=10, m=12, a=18) == INVALID           # MMM2's unit counts,
        assert whole(fn, types_=0b100101) == INVALID            # a type without a type bit
    for fn in (lib.marl_battle_fused_step, lib.marl_battle_fused_step_sample):
        assert step(fn, sl=S - 1) == INVALID and step(fn, t=T) == INVALID and step(fn, t=-1) == INVALID
        assert step(fn, n=10, m=12, a=18) == INVALID
    assert not ops.battle_rollout_supported(3, 30, 10) and not ops.battle_rollout_supported(17, 300, 23)
    torch.cuda.synchronize()
    for t in (obs, state, avail, units, u, r, term, padded, length, won, h, stats):
        assert (t == 5).all().item()


def test_record_struct_null_wrong_widths_and_absent_fields():
    """what only the record struct can express, on 3m with E = 3, T = 4: rec = NULL, and a record whose O or S is not the map's, are
    refused by all six battle entries and nothing is written; marl_battle_reset runs with u / r / term / padded absent, to the same
    bits"""
    import ctypes as C
    from marl_amd import _lib, ops
    from marl_amd.env.battle import battle_shapes
    from marl_amd.env.synthetic_smac import EpisodeRecord
    lib = _lib.load()
    E, T, M = 3, 4, 3
    N, O, S, A, _ = battle_shapes("3m")
    mac = _mac(_args("3m"))                            # (held: the struct points into its tensors)
    wts = mac.agent.weights()
    f = lambda *s: torch.full(s, 5.0, device=DEV)
    i = lambda *s: torch.full(s, 5, dtype=torch.int32, device=DEV)
    SL = S + 4                                         # a row stride that also holds S + 1 columns: only the width check can refuse
    fields = dict(obs=f(E, T + 1, N, O + 1), state=f(E, T + 1, SL), avail=f(E, T + 1, N, A), u=i(E, T, N), r=f(E, T), term=f(E, T),
                  padded=f(E, T), length=i(E), won=i(E))
    units, h, stats, q, act, alive = i(E, N + M, 5), f(E * N, 64), f(3, E), f(E, 1, N, A), i(E, N), i(E)
    p = lambda t: C.c_void_p(t.data_ptr())
    INVALID = 1

    def calls(rec):
        """the return codes of the six entries on `rec` (by reference, or None)"""
        return [lib.marl_battle_reset(1, 0, 0, 0, 0, 0, p(units), rec, M, None),
                lib.marl_battle_step(0, 0, 0, 0.1, 0, p(act), p(units), rec, p(alive), M, None)] + \
               [fn(0, 0, 0, 0.1, 2, 0, 0, 0, 0.5, p(q), p(units), rec, M, None)
                for fn in (lib.marl_battle_fused_step, lib.marl_battle_fused_step_sample)] + \
               [fn(C.byref(wts), rec, 1, 2, 0, 0, 0, 0, 0, 0.1, p(units), p(h), p(stats), 0.5, 0.0, 0.05, M, 1, 1, None)
                for fn in (lib.marl_battle_rollout, lib.marl_battle_rollout_sample)]
    record = lambda o, s_: C.byref(_lib.MarlRecord(state_ld=SL, E=E, T=T, N=N, O=o, S=s_, A=A,
                                                   **{k: t.data_ptr() for k, t in fields.items()}))
    assert calls(None) == [INVALID] * 6
    assert calls(record(O + 1, S)) == [INVALID] * 6 and calls(record(O, S + 1)) == [INVALID] * 6
    torch.cuda.synchronize()
    for t in list(fields.values()) + [units, h, stats, alive]:
        assert (t.cpu() == 5).all().item()
    # reset reads length / won / obs / state / avail only
    full, bare = EpisodeRecord(E, T, N, O, S, A, DEV), EpisodeRecord(E, T, N, O, S, A, DEV)
    bare.u = bare.r = bare.term = bare.padded = None
    un = {}
    for rec in (full, bare):
        for k in ("obs", "state", "avail"):             # (a sentinel that compares equal to itself: slots 1 .. T keep it)
            getattr(rec, k).fill_(-3.0)
        rec.length.fill_(-7)
        rec.won.fill_(-7)
        un[rec] = torch.full((E, N + M, 5), -7, dtype=torch.int32, device=DEV)
        ops.battle_reset(5, 0, 0, 0, False, 0, un[rec], rec, M)
    torch.cuda.synchronize()
    assert (full.length == T).all().item() and (full.won == 0).all().item() and not (full.obs[:, 0] == -3).all().item()
    for k in ("obs", "state_store", "avail", "length", "won"):
        assert torch.equal(getattr(full, k), getattr(bare, k)), k
    assert torch.equal(un[full], un[bare]) and (full.u == -1).all().item()      # (u: as allocated)


def _build(tmp_path, *more):
    from marl_amd.main import build
    args, env = build(["--env", "battle", "--map", "3m", "--alg", "qmix", "--n_envs", "8", "--seed", "5", "--evaluate_epoch", "1",
                       "--n_steps", "400", "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "model")] + list(more))
    args.save_cycle = 10 ** 9
    return args, env


@pytest.mark.parametrize("overlap", [False, True])
def test_the_launcher_with_the_switch(tmp_path, overlap):
    from marl_amd.env.battle import BattleEnv, FusedBattleEnv
    from marl_amd.main import make_runner
    from marl_amd.utils.logging import Logger
    args, env = _build(tmp_path, "--battle_fused", "True")
    assert type(env) is FusedBattleEnv and isinstance(env, BattleEnv) and args.episode_limit == 60
    args.overlap_rollout = overlap
    r = make_runner(args, env, Logger())
    r.run(0)
    assert r.time_steps >= 400 and env.episode >= 1 and getattr(env, "_stats_ring", None)       # the whole-rollout kernel played
    assert r.buffer.record is not None and r.buffer.current_size >= 8
    rec = r.buffer.record.slice(0, 8)
    assert (rec.length >= 1).all().item() and torch.isfinite(rec.obs).all().item()


def test_without_the_switch_the_refusal_stands(tmp_path):
    from marl_amd.env.battle import BattleEnv
    from marl_amd.main import make_runner
    from marl_amd.utils.logging import Logger
    args, env = _build(tmp_path)
    assert type(env) is BattleEnv and args.battle_fused is False
    args.overlap_rollout = True
    with pytest.raises(RuntimeError, match="whole-rollout kernel"):
        make_runner(args, env, Logger()).run(0)


def test_a_shape_the_whole_kernel_refuses_takes_the_fused_step(monkeypatch):
    from marl_amd import ops
    want = _three("3m", 3)["fused_step"][0]
    monkeypatch.setattr(ops, "battle_rollout_supported", lambda N, O, A: False)
    monkeypatch.setattr(ops, "battle_rollout", lambda *a, **k: pytest.fail("the whole-rollout kernel was launched"))
    monkeypatch.setattr(ops, "battle_step", lambda *a, **k: pytest.fail("the unfused step was launched"))
    from marl_amd.env.battle import FusedBattleEnv
    from marl_amd.rollout import RolloutWorker
    args = _args("3m")
    env = FusedBattleEnv(3, "3m", seed=5)
    assert not env.supports_whole_rollout()
    w = RolloutWorker(env, _mac(args), args)           # rollout_mode is the default, "whole"
    rec = w.generate_episodes(3)[0].record
    assert not getattr(env, "_stats_ring", None)
    for f in _fields():
        assert torch.equal(getattr(rec, f), getattr(want.rec, f)), f
