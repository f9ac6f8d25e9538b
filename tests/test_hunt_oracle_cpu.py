"""The hunt environment's rules in tests/hunt_oracle.py, on the CPU: the shapes of the map table and the map
names, hand-written scenarios number by number, the invariants of full episodes, determinism, that the environment has something to
learn, and what the scripts of the GPU tests cover."""
import numpy as np
import pytest

import hunt_oracle as ho

F32 = np.float32
TABLE = {"2v1": (2, 77, 7, 6, 30), "4v2": (4, 77, 14, 6, 50), "8v8": (8, 77, 40, 6, 100)}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_shapes_equal_the_table(name):
    from marl_amd.env.hunt import HUNT_MAPS, hunt_shapes
    N, O, S, A, T = TABLE[name]
    assert hunt_shapes(name) == TABLE[name] and hunt_shapes(name + "_p2") == TABLE[name]
    assert HUNT_MAPS[name] == ho.MAPS[name]
    M = ho.MAPS[name][2]
    rec = ho.play(name, 2, 1, ho.stay_policy, episode_limit=3)
    assert rec["obs"].shape == (2, 4, N, O) and rec["state"].shape == (2, 4, S) and rec["avail"].shape == (2, 4, N, A)
    assert rec["u"].shape == (2, 3, N) and rec["r"].shape == rec["term"].shape == rec["padded"].shape == (2, 3)
    assert rec["units"].shape == (2, N + M, 3) and rec["alive_next"].shape == (3, 2)
    assert all(rec[k].dtype == F32 for k in ("obs", "state", "avail", "r", "term", "padded"))


def test_map_names_and_their_penalty_suffix():
    from marl_amd.env.hunt import hunt_map
    assert hunt_map("2v1") == (6, 2, 1, 30, 0) and hunt_map("4v2") == (8, 4, 2, 50, 0) and hunt_map("8v8") == (10, 8, 8, 100, 0)
    assert hunt_map("4v2_p2") == (8, 4, 2, 50, 8) and hunt_map("8v8_p1.5") == (10, 8, 8, 100, 6)
    assert hunt_map("2v1_p0") == (6, 2, 1, 30, 0) and hunt_map("2v1_p16")[4] == 64 and hunt_map("2v1_p0.25")[4] == 1
    for name in ("4v2_p2", "8v8_p1.5", "2v1"):
        assert ho.shape_of(name) == hunt_map(name)
    for bad in ("4v2_p0.3", "4v2_p17", "3m", "8v8_", "8v8_p", "4v2_p-1", "4v2_p1e1", "4v2_p2.", "4v2_p.5", "4v2_p2_p2", "4v2p2", "",
                "4v2_p16.25", "4V2"):
        with pytest.raises(ValueError, match="maps: 2v1, 4v2, 8v8"):
            hunt_map(bad)


def test_launcher_refuses_unknown_hunt_maps_before_anything_is_built(monkeypatch):
    from marl_amd import main
    monkeypatch.setattr(main, "HuntEnv", lambda *a, **k: pytest.fail("an environment was made"))
    with pytest.raises(ValueError, match="no map '3m'"):
        main.build(["--env", "hunt", "--map", "3m"])
    with pytest.raises(ValueError, match="multiple of 0.25"):
        main.build(["--env", "hunt", "--map", "4v2_p0.3"])


def _hunt(name, units, **kw):
    h = ho.Hunt(name, 1, 1, **kw)
    h.un[0] = np.array(units, dtype=np.int32)
    return h


def _window(o):
    """the (5, 5, 3) window of an observation row, indexed [dy + 2, dx + 2]"""
    return o[:75].reshape(5, 5, 3)


def test_hand_written_2v1_scenario():
    # a predator in the grid's corner, the other beside it, the prey on the first one's cell
    h = _hunt("2v1_p2", [[0, 0, 1], [1, 0, 1], [0, 0, 1]])
    av = h.avail()[0]
    np.testing.assert_array_equal(av[0], [1, 1, 0, 1, 0, 1])          # (0,+1) and (+1,0) stay on the grid, (0,-1) and (-1,0) do not
    np.testing.assert_array_equal(av[1], [1, 1, 0, 1, 1, 1])
    o = h.obs()[0]
    w = _window(o[0])
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            off = dx < 0 or dy < 0
            want = [0, 0, 1] if off else [1 if (dx, dy) == (1, 0) else 0, 1 if (dx, dy) == (0, 0) else 0, 0]
            np.testing.assert_array_equal(w[dy + 2, dx + 2], want, err_msg=str((dx, dy)))
    assert int(w[..., 2].sum()) == 16                                 # two columns and two rows of the window lie off the grid
    np.testing.assert_array_equal(o[0, 75:], [0, 0])
    np.testing.assert_array_equal(o[1, 75:], [F32(1) / F32(5), 0])
    w1 = _window(o[1])
    np.testing.assert_array_equal(w1[2, 1], [1, 1, 0])                # the other predator and the prey, one cell to the west
    np.testing.assert_array_equal(w1[2, 2], [0, 0, 0])                # its own cell: itself is not "another predator"
    np.testing.assert_array_equal(h.state()[0], [0, 0, F32(1) / F32(5), 0, 1, 0, 0])
    # a lone attempt at penalty 2: r = -2 exactly, the prey lives on
    r, term, padded, alive, u = h.step(0, [[5, 0]])
    assert r[0] == F32(-2) and term[0] == 0 and padded[0] == 0 and alive[0] == 1 and h.un[0, 2, 2] == 1
    np.testing.assert_array_equal(u[0], [5, 0])
    # a capture by two: +10, the episode is won, the prey's state row is zeros and nobody sees it
    h = _hunt("2v1_p2", [[0, 0, 1], [1, 0, 1], [0, 0, 1]])
    r, term, padded, alive, u = h.step(0, [[5, 5]])
    assert r[0] == F32(10) and term[0] == 1 and alive[0] == 0 and h.won[0] == 1 and h.length[0] == 1
    np.testing.assert_array_equal(h.un[0], [[0, 0, 1], [1, 0, 1], [0, 0, 0]])
    np.testing.assert_array_equal(h.state()[0], [0, 0, F32(1) / F32(5), 0, 0, 0, 0])
    assert not h.obs()[0, :, :75].reshape(2, 25, 3)[:, :, 1].any() and not h.avail()[0, :, 5].any()
    # a catch given with no prey near, a move off the grid and an action outside 0 .. 5: all stay, and the record keeps them
    h = _hunt("2v1_p2", [[0, 0, 1], [5, 5, 1], [3, 3, 1]])
    assert not h.avail()[0, :, 5].any()
    r, term, padded, alive, u = h.step(0, [[5, 1]])
    assert r[0] == 0 and h.events["bad_catch"] == 1 and h.events["off_grid"] == 1 and h.events["lone"] == 0
    np.testing.assert_array_equal(u[0], [5, 1])
    np.testing.assert_array_equal(h.un[0, :2], [[0, 0, 1], [5, 5, 1]])
    r, term, padded, alive, u = h.step(1, [[4, 9]])
    np.testing.assert_array_equal(u[0], [4, 9])
    np.testing.assert_array_equal(h.un[0, :2], [[0, 0, 1], [5, 5, 1]])
    assert h.events["off_grid"] == 2 and h.events["outside"] == 1
    r, term, padded, alive, u = h.step(2, [[1, 2]])
    np.testing.assert_array_equal(h.un[0, :2], [[0, 1, 1], [5, 4, 1]])                    # (0,+1) and (0,-1)
    r, term, padded, alive, u = h.step(3, [[3, 4]])
    np.testing.assert_array_equal(h.un[0, :2], [[1, 1, 1], [4, 4, 1]])                    # (+1,0) and (-1,0)


def test_hand_written_4v2_scenario():
    # predators 0 .. 2 around prey 0 at (3, 3); predator 3 between the two prey at equal distance 1
    units = [[3, 3, 1], [3, 4, 1], [2, 3, 1], [5, 3, 1], [3, 3, 1], [6, 3, 1]]
    h = _hunt("4v2_p2", units)
    d = h.dist()[0]
    np.testing.assert_array_equal(d, [[0, 3], [1, 4], [1, 4], [2, 1]])
    np.testing.assert_array_equal(h.avail()[0, :, 5], [1, 1, 1, 1])
    # a capture by three (+10), and predator 3 catches prey 1 alone (-2): r = 8
    r, term, padded, alive, u = h.step(0, [[5, 5, 5, 5]])
    assert r[0] == F32(8) and term[0] == 0 and h.events["capture3"] == 1 and h.events["lone"] == 1
    np.testing.assert_array_equal(h.un[0, 4], [3, 3, 0])                                  # a captured prey stays where it was
    np.testing.assert_array_equal(h.state()[0, 8:11], [0, 0, 0])
    assert h.state()[0, 11] == 1
    # the tie: predator 3 at (5, 3) with prey 0 at (4, 3) and prey 1 at (6, 3) - the catch goes to prey 0, the lower index
    h = _hunt("4v2_p2", [[4, 4, 1], [0, 0, 1], [0, 7, 1], [5, 3, 1], [4, 3, 1], [6, 3, 1]])
    r, term, padded, alive, u = h.step(0, [[5, 0, 0, 5]])
    assert r[0] == F32(10) and h.events["tie"] == 1 and h.events["capture2"] == 1 and h.un[0, 4, 2] == 0 and h.un[0, 5, 2] == 1
    # two captures in one step: r = 20, both prey gone, won
    h = _hunt("4v2_p2", [[1, 1, 1], [1, 2, 1], [6, 6, 1], [6, 5, 1], [1, 1, 1], [6, 6, 1]])
    r, term, padded, alive, u = h.step(0, [[5, 5, 5, 5]])
    assert r[0] == F32(20) and term[0] == 1 and h.won[0] == 1 and h.events["double"] == 1
    np.testing.assert_array_equal(h.state()[0, 8:], np.zeros(6, F32))
    # no penalty on the plain map: the same lone attempt is worth 0
    h = _hunt("4v2", units)
    assert h.step(0, [[0, 0, 0, 5]])[0][0] == 0 and h.events["lone"] == 1
    # penalty 1.5, two lone attempts: -3
    h = _hunt("4v2_p1.5", units)
    assert h.step(0, [[5, 0, 0, 5]])[0][0] == F32(-3)


@pytest.mark.parametrize("name", sorted(ho.CASES))
def test_episode_invariants(name):
    rec = ho.case_record(name)
    G, N, M, T, pen4 = ho.shape_of(ho.CASES[name][0])
    T = ho.CASES[name][6] or T
    E = rec["u"].shape[0]
    L, t = rec["length"], np.arange(T)[None, :]
    assert rec["u"].shape[1] == T and ((L >= 1) & (L <= T)).all()
    np.testing.assert_array_equal(rec["padded"], (t >= L[:, None]).astype(F32))
    np.testing.assert_array_equal(rec["term"], (t >= L[:, None] - 1).astype(F32))
    np.testing.assert_array_equal(rec["alive_next"].T, (t < L[:, None] - 1).astype(np.int32))
    after = t >= L[:, None]
    assert (rec["u"][after] == -1).all() and (rec["r"][after] == 0).all()
    np.testing.assert_array_equal(rec["u"][~after], rec["script"][~after])
    slot_after = np.arange(T + 1)[None, :] > L[:, None]
    for k in ("obs", "state", "avail"):
        assert not rec[k][slot_after].any(), k
    # the unit state seen through the state rows: inside the grid, the live flag never rises
    st = rec["state"]
    pos = np.rint(st[:, :, :2 * N] * F32(G - 1)).astype(int)
    assert ((pos >= 0) & (pos < G)).all()
    prey = st[:, :, 2 * N:].reshape(E, T + 1, M, 3)
    live = prey[..., 0]
    assert set(np.unique(live)) <= {0.0, 1.0} and (np.diff(live, axis=1) <= 0).all()
    qpos = np.rint(prey[..., 1:] * F32(G - 1)).astype(int)
    assert ((qpos >= 0) & (qpos < G)).all() and not prey[live == 0].any()
    # availability recomputed from the state rows, at every slot up to the final observation
    px, py = pos[..., 0::2], pos[..., 1::2]                                               # (E, T + 1, N)
    dist = np.abs(qpos[:, :, None, :, 0] - px[..., None]) + np.abs(qpos[:, :, None, :, 1] - py[..., None])
    near = ((dist <= 1) & (live[:, :, None, :] > 0)).any(axis=3)
    want = np.stack([np.ones_like(px), py + 1 < G, py - 1 >= 0, px + 1 < G, px - 1 >= 0, near], axis=-1).astype(F32)
    want[slot_after] = 0
    np.testing.assert_array_equal(rec["avail"], want)
    # the observation's own block is the state's, and a window cell says "prey" only where a live prey is
    np.testing.assert_array_equal(rec["obs"][..., 75:], st[:, :, :2 * N].reshape(E, T + 1, N, 2))
    seen = rec["obs"][..., :75].reshape(E, T + 1, N, 25, 3)[..., 1].sum(axis=3)           # cells with a prey in each window
    cells = ((np.abs(qpos[:, :, None, :, 0] - px[..., None]) <= 2) & (np.abs(qpos[:, :, None, :, 1] - py[..., None]) <= 2) &
             (live[:, :, None, :] > 0))
    assert (seen <= cells.sum(axis=3)).all() and ((seen > 0) == cells.any(axis=3)).all()
    # endings: won exactly where no prey is left, and then within the time limit; the final unit state is the last live slot's
    left = rec["units"][:, N:, 2].any(axis=1)
    np.testing.assert_array_equal(rec["won"], (~left).astype(np.int32))
    assert (L[left] == T).all()
    rows = np.arange(E)
    np.testing.assert_array_equal(rec["units"][:, :N, :2].reshape(E, -1), pos[rows, L])
    np.testing.assert_array_equal(rec["units"][:, N:, 2], live[rows, L].astype(np.int32))
    assert (rec["units"][:, :N, 2] == 1).all() and (rec["units0"][:, :, 2] == 1).all()
    total = rec["r"].sum(axis=1)
    if pen4 == 0:
        assert (rec["r"] >= 0).all() and (total[rec["won"] == 1] == 10 * M).all()
    captures = M - rec["units"][:, N:, 2].sum(axis=1)
    assert (total <= 10 * captures).all() and ((4 * rec["r"]) == np.rint(4 * rec["r"])).all()


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("obs", "state", "avail", "u", "r", "term", "padded", "length", "won", "units",
                                                     "units0", "alive_next"))


def test_determinism_env0_and_episode():
    a = ho.play("4v2_p2", 9, 3, ho.uniform_policy(1))
    assert _same(a, ho.play("4v2_p2", 9, 3, ho.uniform_policy(1)))
    assert _same(a, ho.play("4v2_p2", 9, 3, script=a["script"]))
    shifted = ho.play("4v2_p2", 9, 3, ho.uniform_policy(1), env0=2)
    np.testing.assert_array_equal(shifted["units0"][:7], a["units0"][2:])             # environment e of env0 = 2 is environment e + 2
    np.testing.assert_array_equal(shifted["obs"][:7, 0], a["obs"][2:, 0])
    assert (ho.play("4v2_p2", 9, 3, ho.stay_policy, episode=1)["units0"] != a["units0"]).any()
    assert (ho.play("4v2_p2", 9, 4, ho.stay_policy)["units0"] != a["units0"]).any()
    # the prey's walk is keyed by the environment and the step, not by what the predators do
    s0, s1 = ho.play("4v2", 9, 3, ho.stay_policy), ho.play("4v2", 9, 3, ho.stay_policy, env0=2)
    np.testing.assert_array_equal(s1["state"][:7], s0["state"][2:])


def test_there_is_something_to_learn():
    E, seed = 64, 1
    ret = lambda rec: float(rec["r"].sum(axis=1).mean())
    team, lone, uni = (ho.play("4v2_p2", E, seed, ho.POLICIES[p](seed)) for p in ("team", "lone", "uniform"))
    print("4v2_p2 won / mean return: team %.3f / %.2f, lone %.3f / %.2f, uniform %.3f / %.2f"
          % (team["won"].mean(), ret(team), lone["won"].mean(), ret(lone), uni["won"].mean(), ret(uni)))
    assert team["won"].mean() >= 0.9
    assert ret(uni) < 0 and uni["won"].mean() < team["won"].mean()
    assert ret(lone) < ret(team)
    for p in ("team", "lone", "uniform"):
        assert (ho.play("4v2", E, seed, ho.POLICIES[p](seed))["r"] >= 0).all(), p


def test_the_scripts_cover_what_the_gpu_tests_replay():
    recs = {name: ho.case_record(name) for name in ho.CASES}
    total = {k: sum(r["events"][k] for r in recs.values()) for k in ho.EVENTS}
    print(total)
    for k in ho.EVENTS:           # a capture by exactly 2 and by >= 3, a lone attempt, two captures in one step, an equal-distance
        assert total[k] > 0, k    # tie, an unavailable catch, an off-grid move and an outside action given, a prey stopped at the border
    T = {name: r["u"].shape[1] for name, r in recs.items()}
    assert any((r["won"] == 1).any() for r in recs.values())
    assert any(((r["won"] == 0) & (r["length"] == T[name])).any() for name, r in recs.items())
    shapes = [ho.shape_of(c[0]) for c in ho.CASES.values()]
    assert {s[:3] for s in shapes} == {(6, 2, 1), (8, 4, 2), (10, 8, 8), (32, 16, 16)}
    assert {s[4] for s in shapes} >= {0, 6, 8} and {c[1] for c in ho.CASES.values()} == {3, 65}
    assert any(c[3] == 7 for c in ho.CASES.values()) and any(c[6] is not None for c in ho.CASES.values())
    assert {c[4] for c in ho.CASES.values()} == set(ho.POLICIES)
