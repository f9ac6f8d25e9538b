"""numpy restatement of the battle environment's rules, vectorised over environments: integer dynamics, and every
float feature as ONE float32 operation on integers (sqrt of an integer, then one division), so the device must give the same bits.
Written from the rules, not from csrc/battle_env.h: the two are compared in tests/test_gpu_battle.py.

    rec = play("3m", E, seed, attack_policy)         # full episodes; rec["script"] holds the actions the policy gave
    rec = play("3m", E, seed, script=rec["script"])  # the same record again from the (E, T, N) script
"""
import numpy as np

F32 = np.float32
MARINE, STALKER, ZEALOT = 0, 1, 2
HP = np.array([45, 80, 100])
SH = np.array([0, 80, 50])
DMG = np.array([6, 13, 16])
CD = np.array([1, 2, 1])
# map -> (types of either side, T, shield columns, type bits, (O, S, A))
MAPS = {"3m": ([MARINE] * 3, 60, False, 0, (30, 48, 9)),
        "2s3z": ([STALKER] * 2 + [ZEALOT] * 3, 120, True, 2, (80, 120, 11)),
        "3s5z": ([STALKER] * 3 + [ZEALOT] * 5, 150, True, 2, (128, 216, 14))}
ST_AX, ST_AY, ST_EX, ST_EY = 16, 17, 18, 19
MOVES = {2: (0, 2), 3: (0, -2), 4: (2, 0), 5: (-2, 0)}
M32 = 0xFFFFFFFF


def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def hkey(seed, stream, env, t, idx):
    h = mix32((seed & M32) + stream * 0x9E3779B1)
    h = mix32(h + np.asarray(env, dtype=np.uint64) * 0x85EBCA77 + 1)
    h = mix32(h + np.asarray(t, dtype=np.uint64) * 0xC2B2AE3D + 2)
    return mix32(h + np.asarray(idx, dtype=np.uint64) * 0x27D4EB2F + 3)


class Battle:
    """E lock-stepped copies of a map.  un: (E, N + M, 5) int32 x, y, hp, shield, cooldown - allies first"""

    def __init__(self, name, E, seed, env0=0, episode=0):
        types, self.T, self.shield, self.tb, (self.O, self.S, self.A) = MAPS[name]
        self.types = np.array(types)
        self.N = self.M = len(types)
        self.E, self.seed, self.env0, self.episode = E, seed, env0, episode
        self.maxhp = HP[self.types]
        self.maxsh = SH[self.types] if self.shield else np.zeros(self.N, dtype=np.int64)
        total = int(self.maxhp.sum() + self.maxsh.sum()) + 10 * self.M + 200
        self.scale = F32(20) / F32(total)
        self.reset()

    # ---- reset
    def reset(self):
        E, N, M = self.E, self.N, self.M
        env = (self.env0 + np.arange(E))[:, None]
        i = np.arange(N)[None, :]
        un = np.zeros((E, N + M, 5), dtype=np.int32)
        un[:, :N, 0] = 8 + (hkey(self.seed, ST_AX, env, self.episode, i) % 3).astype(np.int32)
        un[:, :N, 1] = 16 + 2 * i - N + (hkey(self.seed, ST_AY, env, self.episode, i) % 2).astype(np.int32)
        un[:, N:, 0] = 23 - (hkey(self.seed, ST_EX, env, self.episode, i) % 3).astype(np.int32)
        un[:, N:, 1] = 16 + 2 * i - M + (hkey(self.seed, ST_EY, env, self.episode, i) % 2).astype(np.int32)
        un[:, :, 2] = np.concatenate([self.maxhp, self.maxhp])
        un[:, :, 3] = np.concatenate([self.maxsh, self.maxsh])
        self.un = un
        self.length = np.full(E, self.T, dtype=np.int32)
        self.won = np.zeros(E, dtype=np.int32)

    # ---- geometry
    def d2(self):
        """(E, N, M) squared distances ally -> enemy, and the deltas"""
        a, e = self.un[:, :self.N], self.un[:, self.N:]
        dx = e[:, None, :, 0] - a[:, :, None, 0]
        dy = e[:, None, :, 1] - a[:, :, None, 1]
        return dx * dx + dy * dy, dx, dy

    def avail(self):
        E, N, A = self.E, self.N, self.A
        a, e = self.un[:, :N], self.un[:, N:]
        alive = a[:, :, 2] > 0
        av = np.zeros((E, N, A), dtype=F32)
        av[:, :, 0] = ~alive
        av[:, :, 1] = alive
        for k, (mx, my) in MOVES.items():
            x, y = a[:, :, 0] + mx, a[:, :, 1] + my
            av[:, :, k] = alive & (x >= 0) & (x <= 31) & (y >= 0) & (y <= 31)
        d2, _, _ = self.d2()
        av[:, :, 6:] = alive[:, :, None] & (e[:, None, :, 2] > 0) & (d2 <= 36)
        return av

    def _health(self, u, idx):
        """[hp / max, shield / max (shield maps), type bits] of units u (..., K, 5) whose indices into the type list are idx (K,)"""
        cols = [u[..., 2].astype(F32) / self.maxhp[idx].astype(F32)]
        if self.shield:
            cols.append(u[..., 3].astype(F32) / self.maxsh[idx].astype(F32))
        for b in range(self.tb):
            cols.append(np.broadcast_to((self.types[idx] == b + 1).astype(F32), u[..., 2].shape))
        return np.stack(cols, axis=-1)

    def obs(self):
        E, N, M = self.E, self.N, self.M
        un = self.un
        av = self.avail()
        out = np.zeros((E, N, self.O), dtype=F32)
        for i in range(N):
            me = un[:, i]
            parts = [av[:, i, 2:6]]
            others = [j for j in range(N) if j != i]
            for idx, first in ((np.arange(N, N + M), None), (np.array(others, dtype=np.int64), 1)):
                if len(idx) == 0:
                    continue
                u = un[:, idx]
                dx, dy = u[:, :, 0] - me[:, None, 0], u[:, :, 1] - me[:, None, 1]
                d2 = dx * dx + dy * dy
                vis = (u[:, :, 2] > 0) & (d2 <= 81)
                lead = (d2 <= 36).astype(F32) if first is None else np.ones_like(d2, dtype=F32)
                geo = np.stack([lead, np.sqrt(d2.astype(F32)) / F32(9), dx.astype(F32) / F32(9), dy.astype(F32) / F32(9)], axis=-1)
                block = np.where(vis[:, :, None], np.concatenate([geo, self._health(u, idx % N)], axis=-1), F32(0))
                parts.append(block.reshape(E, -1))
            parts.append(self._health(me[:, None], np.array([i]))[:, 0])
            row = np.concatenate(parts, axis=1).astype(F32)
            out[:, i] = np.where((me[:, 2] > 0)[:, None], row, F32(0))
        return out

    def state(self, last):
        """last: (E, N) recorded actions of the previous step, or None at slot 0"""
        E, N, M = self.E, self.N, self.M
        a, e = self.un[:, :N], self.un[:, N:]
        pos = lambda u: [(u[:, :, 0] - 16).astype(F32) / F32(32), (u[:, :, 1] - 16).astype(F32) / F32(32)]
        ha, he = self._health(a, np.arange(N)), self._health(e, np.arange(M))
        ally = np.stack([ha[..., 0], a[:, :, 4].astype(F32) / CD[self.types].astype(F32)] + pos(a), axis=-1)
        ally = np.where((a[:, :, 2] > 0)[:, :, None], np.concatenate([ally, ha[..., 1:]], axis=-1), F32(0))
        enemy = np.where((e[:, :, 2] > 0)[:, :, None], np.concatenate([he[..., :1], np.stack(pos(e), axis=-1), he[..., 1:]], axis=-1), F32(0))
        hot = np.zeros((E, N, self.A), dtype=F32)
        if last is not None:
            ok = (last >= 0) & (last < self.A)
            ee, nn = np.nonzero(ok)
            hot[ee, nn, last[ee, nn]] = 1
        return np.concatenate([ally.reshape(E, -1), enemy.reshape(E, -1), hot.reshape(E, -1)], axis=1).astype(F32)

    # ---- one step: every phase from the pre-step state.  Returns (r, term, padded, alive_next, u) of step t
    def step(self, t, act):
        E, N, M, A = self.E, self.N, self.M, self.A
        act = np.asarray(act, dtype=np.int32)
        live = t < self.length
        pre = self.un.copy()
        av = self.avail()
        d2, _, _ = self.d2()
        move = np.zeros((E, N + M, 2), dtype=np.int32)
        fires = np.zeros((E, N + M), dtype=bool)
        dmg = np.zeros((E, N + M), dtype=np.int64)
        alive = pre[:, :, 2] > 0
        rows = np.arange(E)
        for i in range(N):
            a = act[:, i]
            inside = (a >= 0) & (a < A)
            ac = np.where(inside, a, 1)
            ok = live & alive[:, i] & inside & (av[rows, i, ac] > 0)
            for k, (mx, my) in MOVES.items():
                move[ok & (ac == k), i] = (mx, my)
            shoot = ok & (ac >= 6) & (pre[:, i, 4] == 0)
            fires[:, i] = shoot
            np.add.at(dmg, (rows[shoot], N + ac[shoot] - 6), DMG[self.types[i]])
        any_ally = alive[:, :N].any(axis=1)
        for j in range(M):
            dd = np.where(alive[:, :N], d2[:, :, j], 1 << 30)
            tgt = dd.argmin(axis=1)                       # the first minimum: ties go to the lowest index
            bd = dd[rows, tgt]
            can = live & alive[:, N + j] & any_ally
            shoot = can & (bd <= 36) & (pre[:, N + j, 4] == 0)
            fires[:, N + j] = shoot
            np.add.at(dmg, (rows[shoot], tgt[shoot]), DMG[self.types[j]])
            walk = can & (bd > 36)
            ddx = pre[rows, tgt, 0] - pre[:, N + j, 0]
            ddy = pre[rows, tgt, 1] - pre[:, N + j, 1]
            along_x = np.abs(ddx) >= np.abs(ddy)
            move[walk & along_x, N + j, 0] = (np.sign(ddx) * np.minimum(2, np.abs(ddx)))[walk & along_x]
            move[walk & ~along_x, N + j, 1] = (np.sign(ddy) * np.minimum(2, np.abs(ddy)))[walk & ~along_x]
        un = pre.copy()
        un[:, :, 0:2] += move
        from_shield = np.minimum(dmg, pre[:, :, 3])
        from_hp = np.minimum(dmg - from_shield, pre[:, :, 2])
        un[:, :, 3] = pre[:, :, 3] - from_shield
        un[:, :, 2] = pre[:, :, 2] - from_hp
        cds = np.concatenate([CD[self.types], CD[self.types]])[None, :]
        un[:, :, 4] = np.where(fires, cds, np.maximum(pre[:, :, 4] - 1, 0))
        un = np.where(live[:, None, None], un, pre).astype(np.int32)
        removed = (from_shield + from_hp)[:, N:].sum(axis=1)
        kills = ((pre[:, N:, 2] > 0) & (un[:, N:, 2] <= 0)).sum(axis=1)
        allies_left = (un[:, :N, 2] > 0).any(axis=1)
        enemies_left = (un[:, N:, 2] > 0).any(axis=1)
        win = live & ~enemies_left & allies_left
        points = removed + 10 * kills + 200 * win
        over = ~live | ~enemies_left | ~allies_left | (t + 1 == self.T)
        r = np.where(live, points.astype(F32) * self.scale, F32(0)).astype(F32)
        ends = live & over
        self.length[ends] = t + 1
        self.won[ends] = win[ends]
        self.un = un
        u = np.where(live[:, None], act, -1).astype(np.int32)
        return r, over.astype(F32), (~live).astype(F32), (~over).astype(np.int32), u


# ---- policies: (battle, t) -> (E, N) actions from the battle's own availability; finished environments get -1 in play()
def stop_policy(b, t):
    return np.where(b.un[:, :b.N, 2] > 0, 1, 0).astype(np.int32)


def attack_policy(b, t):
    """attack the lowest-index attackable enemy, else move east (stop at the edge)"""
    av = b.avail()
    first = av[:, :, 6:].argmax(axis=2)
    act = np.where(av[:, :, 6:].any(axis=2), 6 + first, np.where(av[:, :, 4] > 0, 4, 1))
    return np.where(av[:, :, 0] > 0, 0, act).astype(np.int32)


def uniform_policy(seed):
    """uniform over the available actions, from a seeded generator"""
    rng = np.random.default_rng(seed)

    def policy(b, t):
        av = b.avail()
        x = rng.random(av.shape[:2])
        n = av.sum(axis=2)
        k = np.minimum((x * n).astype(np.int64), n.astype(np.int64) - 1)
        return (np.cumsum(av, axis=2) > k[:, :, None]).argmax(axis=2).astype(np.int32)
    return policy


def wild_policy(seed):
    """uniform over ALL actions, available or not, dead agents included: unavailable moves, attacks out of range, on dead enemies
    and on cooldown, which the rules turn into stop while the record keeps them"""
    rng = np.random.default_rng(seed)

    def policy(b, t):
        return rng.integers(0, b.A, size=(b.E, b.N)).astype(np.int32)
    return policy


def truce_policy(b, t):
    """attack_policy until one enemy is left, then no more attacks: every ally walks away from it (the available move that does not
    bring it nearer, with the most room to the wall; stop when cornered).  Some of these episodes run into the time limit"""
    N = b.N
    foe = b.un[:, N:]
    last = foe[np.arange(b.E), (foe[:, :, 2] > 0).argmax(axis=1)]
    a, av = b.un[:, :N], b.avail()
    dx, dy = last[:, None, 0] - a[:, :, 0], last[:, None, 1] - a[:, :, 1]
    room = np.stack([np.where(dy <= 0, 31 - a[:, :, 1], -1), np.where(dy >= 0, a[:, :, 1], -1),
                     np.where(dx <= 0, 31 - a[:, :, 0], -1), np.where(dx >= 0, a[:, :, 0], -1)], axis=2)
    room = np.where(av[:, :, 2:6] > 0, room, -1)
    flee = np.where(room.max(axis=2) >= 0, 2 + room.argmax(axis=2), 1)
    flee = np.where(av[:, :, 0] > 0, 0, flee)
    one = (foe[:, :, 2] > 0).sum(axis=1) <= 1
    return np.where(one[:, None], flee, attack_policy(b, t)).astype(np.int32)


def play(name, E, seed, policy=None, script=None, env0=0, episode=0):
    """full episodes of E environments; the (T+1)-slot record, alive_next of every step (T, E), the final unit state and the script"""
    b = Battle(name, E, seed, env0=env0, episode=episode)
    T, N = b.T, b.N
    rec = dict(obs=np.zeros((E, T + 1, N, b.O), F32), state=np.zeros((E, T + 1, b.S), F32), avail=np.zeros((E, T + 1, N, b.A), F32),
               u=np.full((E, T, N), -1, np.int32), r=np.zeros((E, T), F32), term=np.zeros((E, T), F32), padded=np.zeros((E, T), F32),
               alive_next=np.zeros((T, E), np.int32), script=np.full((E, T, N), -1, np.int32), units0=b.un.copy())
    rec["obs"][:, 0], rec["state"][:, 0], rec["avail"][:, 0] = b.obs(), b.state(None), b.avail()
    for t in range(T):
        live = t < b.length
        act = script[:, t] if script is not None else np.where(live[:, None], policy(b, t), -1).astype(np.int32)
        rec["script"][:, t] = act
        rec["r"][:, t], rec["term"][:, t], rec["padded"][:, t], rec["alive_next"][t], rec["u"][:, t] = b.step(t, act)
        o, s, a = b.obs(), b.state(rec["u"][:, t]), b.avail()
        rec["obs"][:, t + 1] = np.where(live[:, None, None], o, F32(0))
        rec["state"][:, t + 1] = np.where(live[:, None], s, F32(0))
        rec["avail"][:, t + 1] = np.where(live[:, None, None], a, F32(0))
    rec["length"], rec["won"], rec["units"] = b.length.copy(), b.won.copy(), b.un.copy()
    return rec


# ---- the scripts tests/test_gpu_battle.py replays on the device: (map, E, seed, env0, policy, policy seed).  Between them: the three
# maps, E = 3 and E = 65, env0 = 7, every policy, and each of the three endings (tests/test_battle_oracle_cpu.py checks that here)
POLICIES = {"stop": lambda s: stop_policy, "attack": lambda s: attack_policy, "truce": lambda s: truce_policy,
            "uniform": uniform_policy, "wild": wild_policy}
CASES = {"3m-attack-E3": ("3m", 3, 5, 0, "attack", 0),
         "3m-uniform-E65-env7": ("3m", 65, 11, 7, "uniform", 1),
         "3m-stop-E65": ("3m", 65, 2, 0, "stop", 0),
         "3m-wild-E65": ("3m", 65, 4, 0, "wild", 2),
         "2s3z-wild-E3": ("2s3z", 3, 1, 0, "wild", 3),
         "2s3z-attack-E65-env7": ("2s3z", 65, 6, 7, "attack", 0),
         "3s5z-uniform-E3": ("3s5z", 3, 2, 0, "uniform", 4),
         "3s5z-truce-E65": ("3s5z", 65, 3, 0, "truce", 0)}
_records = {}


def case_record(name, episode=0):
    """the oracle's record of a case, played once and shared: treat it as read-only"""
    if (name, episode) not in _records:
        m, E, seed, env0, policy, pseed = CASES[name]
        _records[name, episode] = play(m, E, seed, POLICIES[policy](pseed + episode), env0=env0, episode=episode)
    return _records[name, episode]


def endings(rec):
    """(wins, losses, time limits) of a record: an episode that ran to T with both sides standing hit the limit"""
    N, T = rec["u"].shape[2], rec["u"].shape[1]
    allies, enemies = (rec["units"][:, :N, 2] > 0).any(axis=1), (rec["units"][:, N:, 2] > 0).any(axis=1)
    return int((rec["won"] == 1).sum()), int((~allies).sum()), int((allies & enemies & (rec["length"] == T)).sum())
