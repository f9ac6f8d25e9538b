"""bench.py --dump-outputs: the outputs of the last timed step as DIR/<name>.npy (float32 / float64), a fixed seeded sample of the
episodes, never more than the byte budget.  The writer is fed a CPU episode record here (no GPU needed)."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _last_step(E=40, T=6, N=3, O=7, S=5, A=4):
    from marl_amd.env.synthetic_smac import EpisodeRecord
    from marl_amd.rollout import EpisodeBatch
    g = torch.Generator().manual_seed(3)
    rec = EpisodeRecord(E, T, N, O, S, A, "cpu")
    rec.obs.copy_(torch.rand(rec.obs.shape, generator=g))
    rec.state_store[..., :S] = torch.rand(E, T + 1, S, generator=g)
    rec.avail.fill_(1)
    rec.length.copy_(torch.randint(1, T + 1, (E,), generator=g, dtype=torch.int32))
    live = torch.arange(T)[None, :] < rec.length[:, None]
    rec.u.copy_(torch.where(live[..., None], torch.randint(0, A, (E, T, N), generator=g, dtype=torch.int32), -1))
    rec.r.copy_(torch.rand(E, T, generator=g) * live)
    rec.padded.copy_((~live).float())
    rec.term[torch.arange(E), rec.length.long() - 1] = 1
    learner = types.SimpleNamespace(_flat=types.SimpleNamespace(flat=torch.arange(50, dtype=torch.float32)))
    stats = (rec.r.sum(1).tolist(), [bool(i % 3 == 0) for i in range(E)])
    return (EpisodeBatch(rec), stats, 0.375), learner, rec


def test_dump_writes_the_steps_outputs_within_the_budget(tmp_path):
    import bench
    from marl_amd.rollout import EpisodeBatch
    last, learner, rec = _last_step()
    limit = 60000                                         # room for some of the 40 episodes, not all
    state = np.random.get_state()[1].copy()
    names = bench.dump_outputs(str(tmp_path), last, learner, limit=limit)
    assert np.array_equal(np.random.get_state()[1], state)      # the bench's own draws are not disturbed
    assert set(names) == ({"loss", "params", "episode_reward", "episode_won", "episode_index"} |
                          {"episode_" + k for k in EpisodeBatch.KEYS})
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in names)
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= limit
    got = {n: np.load(tmp_path / (n + ".npy")) for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert got["loss"].tolist() == [0.375] and np.array_equal(got["params"], np.arange(50, dtype=np.float32))
    assert got["episode_reward"].shape == (40,) and got["episode_won"].sum() == 14
    idx = got["episode_index"].astype(np.int64)
    assert 0 < len(idx) < 40 and np.all(np.diff(idx) > 0)
    full = EpisodeBatch(rec)
    for k in EpisodeBatch.KEYS:                           # the sampled rows of exactly what the caller received
        np.testing.assert_array_equal(got["episode_" + k], full[k][torch.as_tensor(idx)].float().numpy())


def test_dump_sample_is_fixed_and_whole_when_it_fits(tmp_path):
    import bench
    last, learner, _ = _last_step()
    bench.dump_outputs(str(tmp_path / "a"), last, learner, limit=60000)
    bench.dump_outputs(str(tmp_path / "b"), last, learner, limit=60000)
    for f in os.listdir(tmp_path / "a"):
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    bench.dump_outputs(str(tmp_path / "c"), last, learner)      # 64 MB: every episode
    assert np.array_equal(np.load(tmp_path / "c" / "episode_index.npy"), np.arange(40))
