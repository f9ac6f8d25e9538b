"""The battle environment's kernels (csrc/battle.hip) against tests/battle_oracle.py: the oracle plays full episodes and records its
actions, the device replays the script step by step (no host read-back inside the loop), then every record field, length, won,
alive_next of every step and the final unit state are compared.  Integer fields are equal; float fields are equal bit for bit: every
feature is one correctly rounded fp32 operation on integers."""
import ctypes as C

import numpy as np
import pytest
import torch

import battle_oracle as bo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FLOATS, INTS = ("obs", "state", "avail", "r", "term", "padded"), ("u", "length", "won")


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
    env.begin_episode(rec)
    for t in range(T):
        env.observe(t, rec)
        env.step(t, steps[t], rec, alive[t])
    env.observe(T, rec)
    return rec, alive


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def compare(c, want, rec, alive, units):
    got = {k: getattr(rec, k).cpu().numpy() for k in FLOATS + INTS}
    got["alive_next"], got["units"] = alive.cpu().numpy(), units.cpu().numpy()
    for k in FLOATS + INTS + ("alive_next", "units"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (c, k)
        bad = bits(got[k]) != bits(want[k])
        assert not bad.any(), (c, k, int(bad.sum()), np.argwhere(bad)[0], got[k][tuple(np.argwhere(bad)[0])],
                               want[k][tuple(np.argwhere(bad)[0])])
    assert not rec.state_store[..., rec.S:].any().item(), (c, "state pad columns")


def make_env(name):
    from marl_amd.env.battle import BattleEnv
    m, E, seed, env0, _, _ = bo.CASES[name]
    return BattleEnv(E, m, seed=seed, env0=env0)


@pytest.mark.parametrize("name", sorted(bo.CASES))
def test_replay_equals_the_oracle(name):
    want = bo.case_record(name)
    env = make_env(name)
    rec, alive = replay(env, want["script"])
    compare(name, want, rec, alive, env.units)
    assert env.observe(0, rec) is None and env.global_step(3) == 3


def test_second_episode_on_the_same_env_object():
    name = "3m-uniform-E65-env7"
    env = make_env(name)
    for episode in range(2):
        want = bo.case_record(name, episode)
        rec, alive = replay(env, want["script"])
        assert env.episode == episode and env.global_step(2) == episode * 61 + 2
        compare((name, episode), want, rec, alive, env.units)
    assert (bo.case_record(name, 0)["units0"] != bo.case_record(name, 1)["units0"]).any()


def test_record_is_a_view_into_a_larger_ring():
    """the view ReplayBuffer.next_slot_record hands out: episodes [3, 6) of an 8-episode ring (on 3m an environment is 5490 observation
    floats, so the view starts 8 bytes off a 16-byte line and its slots take both phases); the ring's other episodes stay as they were"""
    import types
    from marl_amd.common.replaybuffer import ReplayBuffer
    from marl_amd.env.synthetic_smac import EpisodeRecord
    name = "3m-attack-E3"
    want = bo.case_record(name)
    env = make_env(name)
    buf = ReplayBuffer(types.SimpleNamespace(buffer_size=8, **env.get_env_info()))
    buf.current_idx = buf.current_size = 3
    view = buf.next_slot_record(3, env.episode_limit, env.n_agents, env.obs_shape, env.state_shape, env.n_actions, DEV)
    ring = buf.record
    assert view is not None and view.sink_slot == 3 and ring.E == 8 and view.obs.data_ptr() == ring.obs[3].data_ptr()
    assert view.obs.data_ptr() % 16 == 8
    for k in ("obs", "avail", "r", "term", "padded"):
        getattr(ring, k).fill_(7.0)
    ring.state.fill_(7.0)
    before = ring.clone()
    rec, alive = replay(env, want["script"], rec=view)
    compare(name, want, rec, alive, env.units)
    for k in EpisodeRecord.FIELDS:
        for sl in (slice(0, 3), slice(6, 8)):
            assert torch.equal(getattr(ring, k)[sl], getattr(before, k)[sl]), k


def test_mmm2_sized_unit_counts_are_refused_without_writing():
    from marl_amd import _lib, ops
    lib = _lib.load()
    assert not ops.battle_supported(10, 12, 18) and not ops.battle_supported(17, 17, 23) and not ops.battle_supported(3, 3, 10)
    assert ops.battle_supported(3, 3, 9) and ops.battle_supported(16, 16, 22) and ops.battle_supported(1, 1, 7)
    E, T, N, M, A, O, S = 2, 3, 10, 12, 18, 176, 322
    f = lambda *s: torch.full(s, 5.0, device=DEV)
    i = lambda *s: torch.full(s, 5, dtype=torch.int32, device=DEV)
    obs, state, avail, units, u = f(E, T + 1, N, O), f(E, T + 1, 324), f(E, T + 1, N, A), i(E, N + M, 5), i(E, T, N)
    r, term, padded, length, won, alive, act = f(E, T), f(E, T), f(E, T), i(E), i(E), i(E), i(E, N)
    p = lambda t: C.c_void_p(t.data_ptr())

    def record(state_ld, N, O, S, A):
        """the MarlRecord of the tensors above with these sizes, by reference"""
        return C.byref(_lib.MarlRecord(state_ld=state_ld, E=E, T=T, N=N, O=O, S=S, A=A, **{k: t.data_ptr() for k, t in dict(
            obs=obs, state=state, avail=avail, u=u, r=r, term=term, padded=padded, length=length, won=won).items()}))
    INVALID = 1                                                                            # hipErrorInvalidValue
    assert lib.marl_battle_reset(1, 0, 0, 0, 1, 2, p(units), record(324, N, O, S, A), M, None) == INVALID
    assert lib.marl_battle_step(0, 1, 2, 0.1, 0, p(act), p(units), record(324, N, O, S, A), p(alive), M, None) == INVALID
    # a supported shape (3m: O = 30, S = 48) with a state row stride below S, a step outside the episode, a type without a type bit
    assert lib.marl_battle_step(0, 0, 0, 0.1, 0, p(act), p(units), record(47, 3, 30, 48, 9), p(alive), 3, None) == INVALID
    assert lib.marl_battle_step(0, 0, 0, 0.1, T, p(act), p(units), record(48, 3, 30, 48, 9), p(alive), 3, None) == INVALID
    assert lib.marl_battle_reset(1, 0, 0, 0b100101, 0, 0, p(units), record(48, 3, 30, 48, 9), 3, None) == INVALID
    torch.cuda.synchronize()
    for t in (obs, state, avail, units, u, r, term, padded, length, won, alive, act):
        assert (t == 5).all().item()
