"""numpy restatement of the hunt environment's rules, vectorised over environments: integer dynamics, and every
float feature 0, 1 or ONE float32 division of two integers, so the device must give the same bits.  Written from the rules, not
from csrc/hunt_env.h (it walks the units where the kernels look cells up in count tiles): the two are compared in
tests/test_gpu_hunt.py.

    rec = play("4v2_p2", E, seed, team_policy)           # full episodes; rec["script"] holds the actions the policy gave
    rec = play("4v2_p2", E, seed, script=rec["script"])  # the same record again from the (E, T, N) script
"""
import numpy as np

from battle_oracle import hkey

F32 = np.float32
# map -> (G, N, M, T)
MAPS = {"2v1": (6, 2, 1, 30), "4v2": (8, 4, 2, 50), "8v8": (10, 8, 8, 100)}
ST_PX, ST_PY, ST_QX, ST_QY, ST_MOVE = 32, 33, 34, 35, 36
A, O, CATCH = 6, 77, 5
MOVES = {1: (0, 1), 2: (0, -1), 3: (1, 0), 4: (-1, 0)}
WIN_DX = np.tile(np.arange(-2, 3), 5)            # cell c = (dy + 2) 5 + (dx + 2)
WIN_DY = np.repeat(np.arange(-2, 3), 5)
EVENTS = ("capture2", "capture3", "lone", "double", "tie", "bad_catch", "off_grid", "outside", "prey_blocked")


def shape_of(name):
    """(G, N, M, T, pen4) of a map name with its optional _p<penalty> suffix, or of the tuple itself (a direct shape)"""
    if isinstance(name, tuple):
        return name
    base, _, pen = name.partition("_p")
    return MAPS[base] + (int(round(4 * float(pen))) if pen else 0,)


class Hunt:
    """E lock-stepped copies of a map.  un: (E, N + M, 3) int32 x, y, live - predators first"""

    def __init__(self, name, E, seed, env0=0, episode=0, episode_limit=None):
        self.G, self.N, self.M, self.T, self.pen4 = shape_of(name)
        if episode_limit is not None:
            self.T = episode_limit
        self.O, self.S, self.A = O, 2 * self.N + 3 * self.M, A
        self.E, self.seed, self.env0, self.episode = E, seed, env0, episode
        self.events = dict.fromkeys(EVENTS, 0)
        self.reset()

    # ---- reset
    def reset(self):
        E, N, M, G = self.E, self.N, self.M, self.G
        env = (self.env0 + np.arange(E))[:, None]
        un = np.ones((E, N + M, 3), dtype=np.int32)
        for sl, idx, sx, sy in ((slice(0, N), np.arange(N)[None, :], ST_PX, ST_PY), (slice(N, N + M), np.arange(M)[None, :], ST_QX, ST_QY)):
            un[:, sl, 0] = (hkey(self.seed, sx, env, self.episode, idx) % G).astype(np.int32)
            un[:, sl, 1] = (hkey(self.seed, sy, env, self.episode, idx) % G).astype(np.int32)
        self.un = un
        self.length = np.full(E, self.T, dtype=np.int32)
        self.won = np.zeros(E, dtype=np.int32)

    # ---- geometry
    def dist(self):
        """(E, N, M) Manhattan distances predator -> prey, a large number where the prey is not live"""
        p, q = self.un[:, :self.N], self.un[:, self.N:]
        d = np.abs(q[:, None, :, 0] - p[:, :, None, 0]) + np.abs(q[:, None, :, 1] - p[:, :, None, 1])
        return np.where(q[:, None, :, 2] > 0, d, 1 << 20)

    def on_grid(self, x, y):
        return (x >= 0) & (x < self.G) & (y >= 0) & (y < self.G)

    def avail(self):
        p = self.un[:, :self.N]
        av = np.zeros((self.E, self.N, A), dtype=F32)
        av[:, :, 0] = 1
        for k, (mx, my) in MOVES.items():
            av[:, :, k] = self.on_grid(p[:, :, 0] + mx, p[:, :, 1] + my)
        av[:, :, CATCH] = (self.dist() <= 1).any(axis=2)
        return av

    def obs(self):
        E, N, G = self.E, self.N, self.G
        p, q = self.un[:, :N], self.un[:, N:]
        wx = p[:, :, None, 0] + WIN_DX[None, None, :]                        # (E, N, 25)
        wy = p[:, :, None, 1] + WIN_DY[None, None, :]
        off = ~self.on_grid(wx, wy)
        at = lambda u: (u[:, None, None, :, 0] == wx[..., None]) & (u[:, None, None, :, 1] == wy[..., None])   # (E, N, 25, units)
        others = ~np.eye(N, dtype=bool)[None, :, None, :]
        pred = (at(p) & others).any(axis=3)
        prey = (at(q) & (q[:, None, None, :, 2] > 0)).any(axis=3)
        win = np.stack([pred & ~off, prey & ~off, off], axis=-1).astype(F32).reshape(E, N, 75)
        own = p[:, :, 0:2].astype(F32) / F32(G - 1)
        return np.concatenate([win, own], axis=2).astype(F32)

    def state(self):
        E, N, G = self.E, self.N, self.G
        p, q = self.un[:, :N], self.un[:, N:]
        live = (q[:, :, 2] > 0)
        prey = np.concatenate([live[:, :, None].astype(F32), q[:, :, 0:2].astype(F32) / F32(G - 1)], axis=2)
        prey = np.where(live[:, :, None], prey, F32(0))
        return np.concatenate([(p[:, :, 0:2].astype(F32) / F32(G - 1)).reshape(E, -1), prey.reshape(E, -1)], axis=1).astype(F32)

    # ---- one step: every decision from the pre-step state.  Returns (r, term, padded, alive_next, u) of step t
    def step(self, t, act):
        E, N, M, G = self.E, self.N, self.M, self.G
        act = np.asarray(act, dtype=np.int32)
        live = t < self.length
        pre = self.un.copy()
        av, d = self.avail(), self.dist()
        rows = np.arange(E)
        tgt = d.argmin(axis=2)                                 # the first minimum: ties go to the lowest index
        bd = d.min(axis=2)
        inside = (act >= 0) & (act < A)
        ac = np.where(inside, act, 0)
        ok = live[:, None] & inside & (np.take_along_axis(av, ac[:, :, None], axis=2)[:, :, 0] > 0)
        catch = ok & (ac == CATCH)
        cnt = np.zeros((E, M), dtype=np.int64)
        ee, ii = np.nonzero(catch)
        np.add.at(cnt, (ee, tgt[ee, ii]), 1)
        qlive = pre[:, N:, 2] > 0
        captured = qlive & (cnt >= 2)
        lone = qlive & (cnt == 1)
        points4 = 40 * captured.sum(axis=1) - self.pen4 * lone.sum(axis=1)
        r = np.where(live, points4.astype(F32) * F32(0.25), F32(0)).astype(F32)
        un = pre.copy()
        for k, (mx, my) in MOVES.items():
            sel = ok & (ac == k)
            un[:, :N, 0] += np.where(sel, mx, 0).astype(np.int32)
            un[:, :N, 1] += np.where(sel, my, 0).astype(np.int32)
        un[:, N:, 2] = np.where(captured, 0, pre[:, N:, 2])
        tg = self.episode * (self.T + 1) + t
        draw = (hkey(self.seed, ST_MOVE, (self.env0 + rows)[:, None], tg, np.arange(M)[None, :]) % 5).astype(np.int64)
        walks = live[:, None] & qlive & ~captured
        blocked = np.zeros((E, M), dtype=bool)
        for k, (mx, my) in MOVES.items():
            x, y = pre[:, N:, 0] + mx, pre[:, N:, 1] + my
            sel = walks & (draw == k)
            go = sel & self.on_grid(x, y)
            blocked |= sel & ~go
            un[:, N:, 0] += np.where(go, mx, 0).astype(np.int32)
            un[:, N:, 1] += np.where(go, my, 0).astype(np.int32)
        # what happened, for the coverage test of the scripts (live environments only)
        ev = self.events
        ev["capture2"] += int((captured & (cnt == 2)).sum())
        ev["capture3"] += int((captured & (cnt >= 3)).sum())
        ev["lone"] += int(lone.sum())
        ev["double"] += int((captured.sum(axis=1) >= 2).sum())
        ev["tie"] += int((catch & ((d == bd[:, :, None]).sum(axis=2) >= 2)).sum())
        given = live[:, None] & inside
        ev["bad_catch"] += int((given & (act == CATCH) & (av[:, :, CATCH] == 0)).sum())
        ev["off_grid"] += int((given & (ac >= 1) & (ac < CATCH) & ~ok).sum())
        ev["outside"] += int((live[:, None] & ~inside).sum())
        ev["prey_blocked"] += int(blocked.sum())
        prey_left = (un[:, N:, 2] > 0).any(axis=1)
        win = live & ~prey_left
        over = ~live | ~prey_left | (t + 1 == self.T)
        ends = live & over
        self.length[ends] = t + 1
        self.won[ends] = win[ends]
        self.un = np.where(live[:, None, None], un, pre).astype(np.int32)
        u = np.where(live[:, None], act, -1).astype(np.int32)
        return r, over.astype(F32), (~live).astype(F32), (~over).astype(np.int32), u


# ---- policies: (hunt, t) -> (E, N) actions; finished environments get -1 in play()
def stay_policy(h, t):
    return np.zeros((h.E, h.N), dtype=np.int32)


def _walk(h, j):
    """the move of every predator towards prey j[e, i]: along the axis of the larger |delta| (ties: x); stay on its cell"""
    p, q = h.un[:, :h.N], h.un[:, h.N:]
    rows = np.arange(h.E)[:, None]
    dx, dy = q[rows, j, 0] - p[:, :, 0], q[rows, j, 1] - p[:, :, 1]
    along_x = np.abs(dx) >= np.abs(dy)
    move = np.where(along_x, np.where(dx > 0, 3, 4), np.where(dy > 0, 1, 2))
    return np.where((dx == 0) & (dy == 0), 0, move).astype(np.int32)


def team_policy(h, t):
    """walk onto the lowest-index live prey; catch only when adjacent to it, it is the nearest prey (the one a catch targets), and
    another predator is adjacent to it with it as its nearest too - so no catch of this policy is a lone attempt"""
    d = h.dist()
    live = h.un[:, h.N:, 2] > 0
    j0 = live.argmax(axis=1)                                               # (an environment without live prey has ended)
    rows = np.arange(h.E)
    near = (d[rows, :, j0] <= 1) & (d.argmin(axis=2) == j0[:, None])       # (E, N): would catch at j0
    ready = near & (near.sum(axis=1) >= 2)[:, None]
    return np.where(ready, CATCH, _walk(h, np.broadcast_to(j0[:, None], (h.E, h.N)))).astype(np.int32)


def lone_policy(h, t):
    """catch whenever a prey is adjacent, else walk to the nearest"""
    d = h.dist()
    return np.where(d.min(axis=2) <= 1, CATCH, _walk(h, d.argmin(axis=2))).astype(np.int32)


def uniform_policy(seed):
    """uniform over the available actions, from a seeded generator"""
    rng = np.random.default_rng(seed)

    def policy(h, t):
        av = h.avail()
        x = rng.random(av.shape[:2])
        n = av.sum(axis=2)
        k = np.minimum((x * n).astype(np.int64), n.astype(np.int64) - 1)
        return (np.cumsum(av, axis=2) > k[:, :, None]).argmax(axis=2).astype(np.int32)
    return policy


def wild_policy(seed):
    """uniform over -2 .. A + 1, available or not: moves off the grid, catches with no prey near and actions outside 0 .. A - 1,
    which the rules turn into stay while the record keeps them"""
    rng = np.random.default_rng(seed)

    def policy(h, t):
        return rng.integers(-2, A + 2, size=(h.E, h.N)).astype(np.int32)
    return policy


def play(name, E, seed, policy=None, script=None, env0=0, episode=0, episode_limit=None):
    """full episodes of E environments; the (T+1)-slot record, alive_next of every step (T, E), the first and final unit state, the
    script and the events the steps counted"""
    h = Hunt(name, E, seed, env0=env0, episode=episode, episode_limit=episode_limit)
    T, N = h.T, h.N
    rec = dict(obs=np.zeros((E, T + 1, N, h.O), F32), state=np.zeros((E, T + 1, h.S), F32), avail=np.zeros((E, T + 1, N, A), F32),
               u=np.full((E, T, N), -1, np.int32), r=np.zeros((E, T), F32), term=np.zeros((E, T), F32), padded=np.zeros((E, T), F32),
               alive_next=np.zeros((T, E), np.int32), script=np.full((E, T, N), -1, np.int32), units0=h.un.copy())
    rec["obs"][:, 0], rec["state"][:, 0], rec["avail"][:, 0] = h.obs(), h.state(), h.avail()
    for t in range(T):
        live = t < h.length
        act = script[:, t] if script is not None else np.where(live[:, None], policy(h, t), -1).astype(np.int32)
        rec["script"][:, t] = act
        rec["r"][:, t], rec["term"][:, t], rec["padded"][:, t], rec["alive_next"][t], rec["u"][:, t] = h.step(t, act)
        rec["obs"][:, t + 1] = np.where(live[:, None, None], h.obs(), F32(0))
        rec["state"][:, t + 1] = np.where(live[:, None], h.state(), F32(0))
        rec["avail"][:, t + 1] = np.where(live[:, None, None], h.avail(), F32(0))
    rec["length"], rec["won"], rec["units"], rec["events"] = h.length.copy(), h.won.copy(), h.un.copy(), dict(h.events)
    return rec


# ---- the scripts tests/test_gpu_hunt.py replays on the device: (map or direct shape (G, N, M, T, pen4), E, seed, env0, policy, policy
# seed, episode limit).  Between them: the three maps and 16 against 16 on the widest grid (every unit lane taken), E = 3 and E = 65,
# env0 = 7, a shortened time limit, penalties 0, 1.5 and 2, every policy (tests/test_hunt_oracle_cpu.py checks what they cover)
POLICIES = {"stay": lambda s: stay_policy, "team": lambda s: team_policy, "lone": lambda s: lone_policy,
            "uniform": uniform_policy, "wild": wild_policy}
CASES = {"2v1-team-E3": ("2v1", 3, 5, 0, "team", 0, None),
         "2v1_p2-uniform-E65-env7": ("2v1_p2", 65, 11, 7, "uniform", 1, None),
         "4v2_p1.5-wild-E65": ("4v2_p1.5", 65, 4, 0, "wild", 2, None),
         "4v2_p2-lone-E65": ("4v2_p2", 65, 6, 0, "lone", 0, None),
         "4v2-team-E65-T12": ("4v2", 65, 2, 0, "team", 0, 12),
         "8v8-team-E3": ("8v8", 3, 1, 0, "team", 0, None),
         "8v8_p2-lone-E65-env7": ("8v8_p2", 65, 3, 7, "lone", 0, None),
         "8v8-stay-E3": ("8v8", 3, 2, 0, "stay", 0, None),
         "16v16-wild-E65": ((32, 16, 16, 8, 8), 65, 9, 0, "wild", 5, None)}
_records = {}


def case_record(name, episode=0):
    """the oracle's record of a case, played once and shared: treat it as read-only"""
    if (name, episode) not in _records:
        m, E, seed, env0, policy, pseed, limit = CASES[name]
        _records[name, episode] = play(m, E, seed, POLICIES[policy](pseed + episode), env0=env0, episode=episode, episode_limit=limit)
    return _records[name, episode]
