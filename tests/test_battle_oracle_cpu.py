"""The battle environment's rules in tests/battle_oracle.py, on the CPU: the shapes of the map table, a
hand-written scenario number by number, the invariants of full episodes, and that the environment has something to learn."""
import numpy as np
import pytest

import battle_oracle as bo

F32 = np.float32
TABLE = {"3m": (3, 30, 48, 9, 60), "2s3z": (5, 80, 120, 11, 120), "3s5z": (8, 128, 216, 14, 150)}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_shapes_equal_the_table(name):
    from marl_amd import main
    from marl_amd.env.battle import battle_shapes
    N, O, S, A, T = TABLE[name]
    assert battle_shapes(name) == TABLE[name]
    if name in main.MAPS:
        assert main.MAPS[name] == TABLE[name]
    rec = bo.play(name, 2, 1, bo.stop_policy)
    assert rec["obs"].shape == (2, T + 1, N, O) and rec["state"].shape == (2, T + 1, S) and rec["avail"].shape == (2, T + 1, N, A)
    assert rec["u"].shape == (2, T, N) and rec["r"].shape == rec["term"].shape == rec["padded"].shape == (2, T)
    assert rec["units"].shape == (2, 2 * N, 5) and rec["alive_next"].shape == (T, 2)
    assert all(rec[k].dtype == F32 for k in ("obs", "state", "avail", "r", "term", "padded"))


def test_launcher_refuses_unknown_battle_maps_before_anything_is_built():
    from marl_amd import main
    with pytest.raises(ValueError, match="medivac"):
        main.build(["--env", "battle", "--map", "MMM2"])
    with pytest.raises(ValueError, match="no map '8m'"):
        main.build(["--env", "battle", "--map", "8m"])


def test_reset_follows_the_start_rule():
    b = bo.Battle("2s3z", 40, 3, env0=5)
    N = b.N
    i = np.arange(N)[None, :]
    ax, ay, ex, ey = b.un[:, :N, 0], b.un[:, :N, 1], b.un[:, N:, 0], b.un[:, N:, 1]
    assert ((ax >= 8) & (ax <= 10)).all() and ((ex >= 21) & (ex <= 23)).all()
    assert (((ay - (16 + 2 * i - N)) >= 0) & ((ay - (16 + 2 * i - N)) <= 1)).all()
    assert (((ey - (16 + 2 * i - N)) >= 0) & ((ey - (16 + 2 * i - N)) <= 1)).all()
    assert len(np.unique(ax)) == 3 and len(np.unique(ex)) == 3 and (b.un[:, :, 4] == 0).all()
    np.testing.assert_array_equal(b.un[0, :, 2], [80, 80, 100, 100, 100] * 2)
    np.testing.assert_array_equal(b.un[0, :, 3], [80, 80, 50, 50, 50] * 2)
    assert b.scale == F32(20) / F32(2 * 160 + 3 * 150 + 50 + 200)


def test_hand_written_3m_scenario():
    b = bo.Battle("3m", 1, 1)
    assert b.scale == F32(20) / F32(365)
    #                     x   y  hp sh cd
    b.un[0] = np.array([[10, 16, 45, 0, 0], [10, 14, 45, 0, 0], [10, 18, 45, 0, 0],
                        [15, 16, 10, 0, 0], [16, 16, 45, 0, 0], [30, 2, 45, 0, 0]])
    av = b.avail()[0]
    np.testing.assert_array_equal(av[0], [0, 1, 1, 1, 1, 1, 1, 1, 0])        # d2 = 25 and 36: both in range
    np.testing.assert_array_equal(av[1], [0, 1, 1, 1, 1, 1, 1, 0, 0])        # d2 = 29, 40
    o = b.obs()[0, 0]
    np.testing.assert_array_equal(o[:4], [1, 1, 1, 1])
    np.testing.assert_array_equal(o[4:9], [1, F32(5) / F32(9), F32(5) / F32(9), 0, F32(10) / F32(45)])
    np.testing.assert_array_equal(o[9:14], [1, F32(6) / F32(9), F32(6) / F32(9), 0, 1])
    np.testing.assert_array_equal(o[14:19], [0, 0, 0, 0, 0])                 # out of sight
    np.testing.assert_array_equal(o[19:24], [1, F32(2) / F32(9), 0, F32(-2) / F32(9), 1])
    np.testing.assert_array_equal(o[24:30], [1, F32(2) / F32(9), 0, F32(2) / F32(9), 1, 1])
    # step 0: allies 0 and 1 fire at enemy 0 (12 damage on 10 hp: 10 removed + the kill bonus), ally 2 walks north; enemies 0 and 1
    # fire at ally 0 (their nearest), enemy 2 walks 2 cells along x towards ally 1
    r, term, padded, alive, u = b.step(0, np.array([[6, 6, 2]]))
    np.testing.assert_array_equal(b.un[0], [[10, 16, 33, 0, 1], [10, 14, 45, 0, 1], [10, 20, 45, 0, 0],
                                            [15, 16, 0, 0, 1], [16, 16, 45, 0, 1], [28, 2, 45, 0, 0]])
    assert r[0] == F32(20) * b.scale and term[0] == 0 and padded[0] == 0 and alive[0] == 1
    np.testing.assert_array_equal(u[0], [6, 6, 2])
    # step 1: ally 0 fires on cooldown and ally 1 out of range (d2 = 40): both count as stop, the record keeps them; enemy 1 waits
    np.testing.assert_array_equal(b.avail()[0, :, 6:], [[0, 1, 0], [0, 0, 0], [0, 0, 0]])
    r, term, _, _, u = b.step(1, np.array([[7, 7, 1]]))
    np.testing.assert_array_equal(b.un[0], [[10, 16, 33, 0, 0], [10, 14, 45, 0, 0], [10, 20, 45, 0, 0],
                                            [15, 16, 0, 0, 0], [16, 16, 45, 0, 0], [26, 2, 45, 0, 0]])
    assert r[0] == 0 and term[0] == 0
    np.testing.assert_array_equal(u[0], [7, 7, 1])
    s = b.state(u)[0]
    np.testing.assert_array_equal(s[:4], [F32(33) / F32(45), 0, F32(-6) / F32(32), 0])
    np.testing.assert_array_equal(s[12:15], [0, 0, 0])                       # the dead enemy's row
    np.testing.assert_array_equal(s[15:18], [1, 0, 0])
    np.testing.assert_array_equal(s[18:21], [1, F32(10) / F32(32), F32(-14) / F32(32)])
    np.testing.assert_array_equal(s[21:].reshape(3, 9).argmax(axis=1), [7, 7, 1])
    assert s[21:].sum() == 3
    # step 2: the cooldown is over: 6 damage for 6 points
    r, _, _, _, _ = b.step(2, np.array([[7, 1, 1]]))
    assert r[0] == F32(6) * b.scale and b.un[0, 4, 2] == 39 and b.un[0, 0, 2] == 27 and b.un[0, 0, 4] == 1


def test_shield_goes_before_hp_and_counts_for_the_reward():
    b = bo.Battle("2s3z", 1, 1)
    b.un[0, :, 0:2] = [[2, 2 + 6 * k] for k in range(5)] + [[29, 2 + 6 * k] for k in range(5)]       # everyone far from everyone ..
    b.un[0, 2, 0:4] = [15, 14, 100, 10]      # .. but ally zealot 2 (shield 10 left) and enemy stalker 0, 2 cells apart
    b.un[0, 5, 0:2] = [15, 16]
    r, _, _, _, _ = b.step(0, np.array([[1, 1, 6, 1, 1]]))
    np.testing.assert_array_equal(b.un[0, 2], [15, 14, 97, 0, 1])            # 13 damage: 10 off the shield, 3 off hp
    np.testing.assert_array_equal(b.un[0, 5], [15, 16, 80, 64, 2])           # 16 damage, all on the shield; a stalker's cooldown is 2
    assert r[0] == F32(16) * b.scale
    b.step(1, np.array([[1, 1, 6, 1, 1]]))
    np.testing.assert_array_equal(b.un[0, 5, 2:], [80, 64, 1])               # on cooldown: the enemy waits, the ally's shot is a stop
    assert b.un[0, 2, 4] == 0


@pytest.mark.parametrize("name", sorted(bo.CASES))
def test_episode_invariants(name):
    m, E, seed, env0, _, _ = bo.CASES[name]
    rec = bo.case_record(name)
    T, N = rec["u"].shape[1:]
    t = np.arange(T)[None, :]
    L = rec["length"][:, None]
    assert (rec["length"] >= 1).all() and (rec["length"] <= T).all()
    np.testing.assert_array_equal(rec["padded"], (t >= L).astype(F32))
    np.testing.assert_array_equal(rec["term"], (t >= L - 1).astype(F32))
    np.testing.assert_array_equal(rec["alive_next"].T, (t < L - 1).astype(np.int32))
    assert (rec["r"] >= 0).all() and (rec["r"][t >= L] == 0).all()
    assert (rec["u"][(t >= L)[:, :, None].repeat(N, 2)] == -1).all() and (rec["u"][(t < L)[:, :, None].repeat(N, 2)] >= 0).all()
    slots = np.arange(T + 1)[None, :] > L
    assert not rec["obs"][slots].any() and not rec["state"][slots].any() and not rec["avail"][slots].any()
    # a won episode's rewards are all the enemies' hp and shield, the kill bonuses and the win bonus: 20, within fp32 summation error
    won = rec["won"] == 1
    total = rec["r"].astype(np.float64).sum(axis=1)
    assert np.abs(total[won] - 20).max(initial=0) <= T * 20 * 2.0 ** -24
    assert (total[~won] <= 20 - 200 * float(bo.Battle(m, 1, 0).scale) + T * 20 * 2.0 ** -24).all()      # no win bonus
    # hp and shield never rise; availability is the rule recomputed from the unit state; a dead agent has the no-op alone
    b = bo.Battle(m, E, seed, env0=env0)
    for s in range(int(rec["length"].max())):
        live = s <= rec["length"]
        av = rec["avail"][:, s]
        np.testing.assert_array_equal(av[live], b.avail()[live])
        dead = live[:, None] & (b.un[:, :N, 2] <= 0)
        assert (av[dead][:, 0] == 1).all() and (av[dead][:, 1:] == 0).all()
        assert (av[live[:, None] & ~dead][:, 0] == 0).all() and (av[live[:, None] & ~dead][:, 1] == 1).all()
        if s < T:
            before = b.un.copy()
            b.step(s, rec["script"][:, s])
            assert (b.un[:, :, 2:4] <= before[:, :, 2:4]).all() and (b.un[:, :, 2:4] >= 0).all()
            assert (b.un[:, :, 0:2] >= 0).all() and (b.un[:, :, 0:2] <= 31).all()
    np.testing.assert_array_equal(b.un, rec["units"])


def test_same_seed_same_record_and_env0_shifts_the_starts():
    a, b = bo.play("3m", 6, 9, bo.uniform_policy(1)), bo.play("3m", 6, 9, bo.uniform_policy(1))
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    c = bo.play("3m", 6, 9, script=a["script"])
    for k in a:
        np.testing.assert_array_equal(a[k], c[k])
    shifted = bo.Battle("3m", 6, 9, env0=2)
    np.testing.assert_array_equal(shifted.un[:4], a["units0"][2:])
    assert (shifted.un != a["units0"]).any()
    assert (bo.Battle("3m", 6, 9, episode=1).un != a["units0"]).any()


def test_there_is_something_to_learn():
    """64 environments of 3m: firing wins most episodes, standing still wins none"""
    attack, stop = bo.play("3m", 64, 11, bo.attack_policy), bo.play("3m", 64, 11, bo.stop_policy)
    assert stop["won"].sum() == 0 and bo.endings(stop)[1] == 64
    assert attack["won"].sum() > 32
    assert attack["r"].sum() > 4 * stop["r"].sum() + 64


def test_the_gpu_scripts_cover_the_three_endings():
    wins, losses, limits = np.sum([bo.endings(bo.case_record(name)) for name in bo.CASES], axis=0)
    assert wins >= 1 and losses >= 1 and limits >= 1, (wins, losses, limits)
    maps = {bo.CASES[n][0] for n in bo.CASES}
    assert maps == set(TABLE) and {bo.CASES[n][1] for n in bo.CASES} == {3, 65} and any(bo.CASES[n][3] == 7 for n in bo.CASES)
    assert {bo.CASES[n][4] for n in bo.CASES} >= {"uniform", "attack", "stop", "wild"}
    wild = bo.case_record("3m-wild-E65")
    b = bo.Battle("3m", 65, 4)
    unavailable = cooldown = 0
    for t in range(10):
        u, av = wild["script"][:, t], b.avail()
        live = (t < wild["length"])[:, None] & (b.un[:, :3, 2] > 0)
        shot = live & (u >= 6)
        unavailable += int((shot & (np.take_along_axis(av, np.maximum(u, 0)[:, :, None], 2)[:, :, 0] == 0)).sum())
        cooldown += int((shot & (np.take_along_axis(av, np.maximum(u, 0)[:, :, None], 2)[:, :, 0] == 1) & (b.un[:, :3, 4] > 0)).sum())
        b.step(t, u)
    assert unavailable > 0 and cooldown > 0
    assert (wild["script"][wild["length"] < 60][:, -1] == -1).all()
