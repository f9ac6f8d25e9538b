"""The hunt environment's kernels (csrc/hunt.hip) against tests/hunt_oracle.py on the MI355X.  The oracle plays full episodes and
records its actions, the device replays the script step by step, then every record field, length, won, alive_next of every step and
the unit state are compared: integers are equal, floats are equal bit for bit (every feature is 0, 1 or one correctly rounded fp32
division of integers).  Then the fused choice + step against select_actions / policy_sample + step, the RolloutWorker's paths, and the
launcher end to end."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import hunt_oracle as ho
from oracle import seeded

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FLOATS, INTS = ("obs", "state", "avail", "r", "term", "padded"), ("u", "length", "won")
RSEED = 77


def scribble(rec):
    """every field a kernel must write holds garbage first (the state's pad columns stay zero: they are allocated so and left alone)"""
    for k in ("obs", "avail", "r", "term", "padded"):
        getattr(rec, k).fill_(float("nan"))
    rec.state.fill_(float("nan"))
    rec.u.fill_(-9)
    rec.length.fill_(-9)
    rec.won.fill_(-9)


def replay(env, script, rec=None):
    """one episode of `env` from the (E, T, N) script; (record, alive_next of every step (T, E))"""
    rec = env.new_record() if rec is None else rec
    scribble(rec)
    T = env.episode_limit
    steps = torch.from_numpy(np.ascontiguousarray(script.transpose(1, 0, 2))).to(DEV)
    alive = torch.full((T, env.n_envs), -9, dtype=torch.int32, device=DEV)
    env.units.fill_(-9)
    env.begin_episode(rec)
    units0 = env.units.clone()
    for t in range(T):
        env.observe(t, rec)
        env.step(t, steps[t], rec, alive[t])
    env.observe(T, rec)
    return rec, alive, units0


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def compare(c, want, rec, alive, units, units0):
    got = {k: getattr(rec, k).cpu().numpy() for k in FLOATS + INTS}
    got["alive_next"], got["units"], got["units0"] = alive.cpu().numpy(), units.cpu().numpy(), units0.cpu().numpy()
    for k in FLOATS + INTS + ("alive_next", "units", "units0"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (c, k)
        bad = bits(got[k]) != bits(want[k])
        assert not bad.any(), (c, k, int(bad.sum()), np.argwhere(bad)[0], got[k][tuple(np.argwhere(bad)[0])],
                               want[k][tuple(np.argwhere(bad)[0])])
    assert not rec.state_store[..., rec.S:].any().item(), (c, "state pad columns")


def make_env(name):
    from marl_amd.env.hunt import HuntEnv
    m, E, seed, env0, _, _, limit = ho.CASES[name]
    return HuntEnv(E, m, seed=seed, env0=env0, episode_limit=limit)


@pytest.mark.parametrize("name", sorted(ho.CASES))
def test_replay_equals_the_oracle(name):
    want = ho.case_record(name)
    env = make_env(name)
    assert env.batched and env.get_env_info() == dict(n_actions=6, n_agents=want["u"].shape[2], state_shape=want["state"].shape[2],
                                                      obs_shape=77, episode_limit=want["u"].shape[1])
    rec, alive, units0 = replay(env, want["script"])
    compare(name, want, rec, alive, env.units, units0)
    assert env.observe(0, rec) is None and env.global_step(3) == 3


def test_second_episode_on_the_same_env_object():
    name = "2v1_p2-uniform-E65-env7"
    env = make_env(name)
    for episode in range(2):
        want = ho.case_record(name, episode)
        rec, alive, units0 = replay(env, want["script"])
        assert env.episode == episode and env.global_step(2) == episode * 31 + 2
        compare((name, episode), want, rec, alive, env.units, units0)
    assert (ho.case_record(name, 0)["units0"] != ho.case_record(name, 1)["units0"]).any()


def test_record_is_a_view_into_a_larger_ring():
    """the view ReplayBuffer.next_slot_record hands out: episodes [3, 6) of an 8-episode ring whose state rows are padded
    (2v1: S = 7 in rows of 8 floats; an environment is 31 slots of 154 observation floats, so the view starts 8 bytes off a 16-byte
    line and its slots take both phases); the ring's other episodes stay as they were"""
    from marl_amd.common.replaybuffer import ReplayBuffer
    from marl_amd.env.synthetic_smac import EpisodeRecord
    name = "2v1-team-E3"
    want = ho.case_record(name)
    env = make_env(name)
    buf = ReplayBuffer(types.SimpleNamespace(buffer_size=8, **env.get_env_info()))
    buf.current_idx = buf.current_size = 3
    view = buf.next_slot_record(3, env.episode_limit, env.n_agents, env.obs_shape, env.state_shape, env.n_actions, DEV)
    ring = buf.record
    assert view is not None and view.sink_slot == 3 and ring.E == 8 and view.obs.data_ptr() == ring.obs[3].data_ptr()
    assert view.obs.data_ptr() % 16 == 8 and view.state.stride(-2) > view.S
    for k in ("obs", "avail", "r", "term", "padded"):
        getattr(ring, k).fill_(7.0)
    ring.state.fill_(7.0)
    before = ring.clone()
    rec, alive, units0 = replay(env, want["script"], rec=view)
    compare(name, want, rec, alive, env.units, units0)
    for k in EpisodeRecord.FIELDS:
        for sl in (slice(0, 3), slice(6, 8)):
            assert torch.equal(getattr(ring, k)[sl], getattr(before, k)[sl]), k


def test_refused_shapes_write_nothing():
    from marl_amd import _lib
    lib = _lib.load()
    E, T, N, M, G, A, O = 2, 3, 4, 2, 8, 6, 77
    S = 2 * N + 3 * M
    f = lambda *s: torch.full(s, 5.0, device=DEV)
    i = lambda *s: torch.full(s, 5, dtype=torch.int32, device=DEV)
    fields = dict(obs=f(E, T + 1, 17, O + 1), state=f(E, T + 1, 2 * 17 + 3 * 17 + 4), avail=f(E, T + 1, 17, A + 1), u=i(E, T, 17),
                  r=f(E, T), term=f(E, T), padded=f(E, T), length=i(E), won=i(E))
    units, q, act, alive = i(E, 34, 3), f(E, 1, 17, A + 1), i(E, 17), i(E)
    p = lambda t: C.c_void_p(t.data_ptr())
    INVALID = 1                                                                            # hipErrorInvalidValue

    def calls(rec, m=M, g=G, pen4=8, t=0, reset=True):
        """the return codes of the four launchers; reset = False: of the three that take pen4 and t (reset would run)"""
        return ([lib.marl_hunt_reset(1, 0, 0, g, m, p(units), rec, None)] if reset else []) + [
                lib.marl_hunt_step(1, 0, 0, g, pen4, t, p(act), p(units), rec, p(alive), m, None),
                lib.marl_hunt_fused_step(1, 2, 0, 0, g, pen4, t, 0.5, p(q), p(units), rec, m, None),
                lib.marl_hunt_fused_step_sample(1, 2, 0, 0, g, pen4, t, 0.5, p(q), p(units), rec, m, None)]

    def record(**kw):
        v = dict(state_ld=fields["state"].shape[2], E=E, T=T, N=N, O=O, S=S, A=A)     # (a row stride no width here exceeds)
        v.update(kw)
        return C.byref(_lib.MarlRecord(**v, **{k: t.data_ptr() for k, t in fields.items()}))
    assert calls(None) == [INVALID] * 4
    assert calls(record(O=O + 1)) == [INVALID] * 4 and calls(record(S=S + 1)) == [INVALID] * 4
    assert calls(record(state_ld=S - 1)) == [INVALID] * 4
    assert calls(record(N=17, S=2 * 17 + 3 * M)) == [INVALID] * 4 and calls(record(N=1, S=2 + 3 * M)) == [INVALID] * 4
    assert calls(record(S=2 * N + 3 * 17), m=17) == [INVALID] * 4 and calls(record(S=2 * N), m=0) == [INVALID] * 4
    assert calls(record(), g=33) == [INVALID] * 4 and calls(record(), g=2) == [INVALID] * 4
    assert calls(record(A=A + 1)) == [INVALID] * 4
    assert calls(record(), t=T, reset=False) == [INVALID] * 3 and calls(record(), t=-1, reset=False) == [INVALID] * 3
    assert calls(record(), pen4=65, reset=False) == [INVALID] * 3 and calls(record(), pen4=-1, reset=False) == [INVALID] * 3
    torch.cuda.synchronize()
    for t in list(fields.values()) + [units, q, act, alive]:
        assert (t == 5).all().item()


def _same_records(a, b, what):
    from marl_amd.env.synthetic_smac import EpisodeRecord
    for k in EpisodeRecord.FIELDS:              # the nine: obs, state_store, avail, u, r, term, padded, length, won
        x, y = getattr(a, k), getattr(b, k)
        same = torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, y)
        assert same, (what, k)


@pytest.mark.parametrize("sample,eps", [(False, 0.0), (False, 0.3), (True, 0.1)], ids=["greedy", "eps0.3", "sample-eps0.1"])
@pytest.mark.parametrize("E", [3, 65])
@pytest.mark.parametrize("name", ["2v1_p2", "8v8_p1.5"])
def test_fused_step_equals_choice_then_step(name, E, sample, eps):
    """a whole episode: fused_step against select_actions (sample: policy_sample) + step on random q, garbage in the record first"""
    from marl_amd import ops
    from marl_amd.env.hunt import HuntEnv
    envs = [HuntEnv(E, name, seed=4, env0=2) for _ in range(2)]
    N, A, T = envs[0].n_agents, envs[0].n_actions, envs[0].episode_limit
    g = torch.Generator().manual_seed(E + 31 * int(sample))
    q = torch.randn(T, E, 1, N, A, generator=g).to(DEV)          # continuous draws: no ties among a row's actions
    assert all(len(set(row)) == A for row in q[0].reshape(-1, A).cpu().tolist())
    recs = [env.new_record() for env in envs]
    for env, rec in zip(envs, recs):
        scribble(rec)
        env.begin_episode(rec)
    act = torch.full((E, N), -9, dtype=torch.int32, device=DEV)
    alive = torch.ones(E, dtype=torch.int32, device=DEV)
    choose = ops.policy_sample if sample else ops.select_actions
    for t in range(T):
        envs[0].fused_step(t, q[t], eps, RSEED, recs[0], sample=sample)
        choose(q[t], recs[1].avail[:, t], (T + 1) * N * A, alive, eps, RSEED, envs[1].env0, None, envs[1].global_step(t), act, N, E, N, A)
        envs[1].step(t, act, recs[1], alive)
    _same_records(recs[0], recs[1], (name, E, sample, eps))
    assert torch.equal(envs[0].units, envs[1].units)
    u = recs[0].u
    assert not torch.isnan(recs[0].obs).any().item() and not (u == -9).any().item()
    live = recs[0].padded == 0
    assert ((u >= 0) & (u < A))[live].all().item() and (u[~live] == -1).all().item()
    assert (torch.gather(recs[0].avail[:, :T], 3, u.clamp(min=0).long().unsqueeze(-1)).squeeze(-1)[live] == 1).all().item()
    if eps == 0.0:
        masked = q.permute(1, 0, 2, 3, 4).squeeze(2).masked_fill(recs[0].avail[:, :T] == 0, float("-inf"))
        assert torch.equal(masked.argmax(dim=3)[live], u[live].long())


def _args(name, T=None, eps=0.5, alg="qmix"):
    from marl_amd.env.hunt import hunt_shapes
    N, O, S, A, T0 = hunt_shapes(name)
    a = seeded.make_args("2s3z", alg, episode_limit=T or T0, n_agents=N, obs_shape=O, state_shape=S, n_actions=A, map=name,
                         epsilon=eps, seed=RSEED, env="hunt")
    a.anneal_epsilon = 0.01
    a.gemm_mode = "f32"
    return a


def _mac(args, policy=False):
    from marl_amd.controller.share_params import PolicyMAC, SharedMAC
    agent = seeded.seeded_state(seeded.agent_param_shapes(args), seed=11, scale=3.0)
    mac = (PolicyMAC if policy else SharedMAC)(args)
    mac.agent.load_state_dict({k: torch.tensor(v) for k, v in agent.items()})
    mac.cuda()
    return mac


def _worker(name, E, mode, policy=False):
    from marl_amd.env.hunt import HuntEnv
    from marl_amd.rollout import RolloutWorker
    args = _args(name, alg="central_v" if policy else "qmix")
    env = HuntEnv(E, name, seed=5)
    w = RolloutWorker(env, _mac(args, policy), args)
    if mode is not None:
        w.rollout_mode = mode
    return w, env


def _count(monkeypatch):
    """how often each of the environment's two step launches is made"""
    from marl_amd import ops
    n = dict(hunt_step=0, hunt_fused_step=0)
    for k in n:
        def counted(*a, _f=getattr(ops, k), _k=k, **kw):
            n[_k] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, k, counted)
    return n


@pytest.mark.parametrize("policy", [False, True], ids=["SharedMAC", "PolicyMAC-sampling"])
def test_worker_paths_give_one_episode_batch(policy, monkeypatch):
    """the three-launch path (rollout_mode "unfused") against the worker's default (SharedMAC: the fused step) or against
    rollout_mode "fused_step" (a sampling PolicyMAC), two rollouts each"""
    name, E = "4v2_p2", 37
    n = _count(monkeypatch)
    a, env_a = _worker(name, E, "unfused", policy)
    b, env_b = _worker(name, E, "fused_step" if policy else None, policy)
    T = env_a.episode_limit
    for k in range(2):
        ea, ra, wa, sa = a.generate_episodes(E)
        assert n == dict(hunt_step=(k + 1) * T, hunt_fused_step=k * T)
        eb, rb, wb, sb = b.generate_episodes(E)
        assert n == dict(hunt_step=(k + 1) * T, hunt_fused_step=(k + 1) * T)
        _same_records(ea.record, eb.record, ("worker", policy, k))
        assert torch.equal(env_a.units, env_b.units) and (ra, wa, sa) == (rb, wb, sb) and a.epsilon == b.epsilon
        assert sa == int(ea.record.length.sum().item()) and env_a.episode == k
    with pytest.raises(RuntimeError, match="launch_episodes"):
        b.launch_episodes()


@pytest.mark.parametrize("alg", ["qmix", "cw_qmix"])
def test_the_launcher_end_to_end(tmp_path, alg):
    """a smoke test of build + make_runner + run, not a learning claim"""
    from marl_amd.env.hunt import HuntEnv
    from marl_amd.main import build, make_runner
    from marl_amd.utils.logging import Logger
    args, env = build(["--env", "hunt", "--map", "2v1_p2", "--alg", alg, "--n_envs", "8", "--seed", "5", "--evaluate_epoch", "1",
                       "--n_steps", "400", "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "model")])
    args.save_cycle = 10 ** 9
    assert type(env) is HuntEnv and env.pen4 == 8
    assert (args.n_agents, args.obs_shape, args.state_shape, args.n_actions, args.episode_limit) == (2, 77, 7, 6, 30)
    r = make_runner(args, env, Logger())
    loss = r.run(0)
    assert r.time_steps >= 400 and r.train_steps >= 1 and env.episode >= 1
    assert np.isfinite(float(loss)) and all(np.isfinite(float(x)) for x in r.losses)
    win_rate, reward = r.evaluate()
    assert 0.0 <= win_rate <= 1.0 and np.isfinite(reward)
