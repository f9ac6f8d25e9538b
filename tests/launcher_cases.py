"""What the launcher and the runner do with every algorithm name (TEST INFRASTRUCTURE), shared by tests/golden/make_launcher_matrix.py -
which records it - and tests/test_launcher_matrix_cpu.py, which recomputes every case and compares for equality.  Nothing here
looks inside marl_amd.main or marl_amd.runner: the cases go through ``main.build``, ``main.make_runner`` and ``runner.Runner`` alone, so
the recording does not depend on how they find a table, a check or a class.

``build`` cases: the four environment classes on ``main`` are replaced by a stub that reports its map's sizes (no GPU).  An outcome is
the whole namespace, or the exception's type and text, and either way the number of environments made.
    names     the fifteen algorithms, the ten names with an actor suffix that exist or are refused, iql+commnet, qmix_x, an unknown one
    x --env   smac, matrix, battle
    x --map   2s3z, 3m (the synthetic table lacks it), MMM2 (the battle environment lacks it), 8m (both lack it)
    x extras  nothing; each agent switch alone; each switch whose given value survives a table, given; one out-of-range value for each
              switch a validator reads

``Runner`` cases: ``__init__`` of every controller and learner class, of RolloutWorker and of ReplayBuffer is replaced, on the class
itself, by a recorder.  An outcome is the ordered list of what was built with ``on_policy``, or the exception's type and text with what
had been built by then.
    names     as above
    x         Runner(env, logger, args) on the bare name, and main.make_runner(args, env, logger)
    x         every subset of RTW / world_model / MAIC, overlap_rollout, MAIC_train, mi_loss_weight = 0.5, reuse_network = False

The fixture stays readable and small: per name one full namespace and, for that name's other cases, the fields that differ from the
case with the same --env and --map and no extras (or from the full one); the runner's outcomes are stored once each and a case names
its outcome by position."""
from __future__ import annotations

import contextlib
import copy
import importlib
import itertools
import json
import os
from unittest import mock

ALGS = ["vdn", "qmix", "qplex", "qtran_base", "qtran_alt", "iql", "qatten", "ow_qmix", "cw_qmix", "maven", "central_v", "coma",
        "reinforce", "mappo", "lica"]
ACTOR_NAMES = [b + s for b in ("central_v", "coma", "reinforce", "qmix", "lica") for s in ("+commnet", "+g2anet")]
NAMES = ALGS + ACTOR_NAMES + ["iql+commnet", "qmix_x", "no_such_alg"]
ENVS = ["smac", "matrix", "battle"]
MAPS = ["2s3z", "3m", "MMM2", "8m"]
SWITCHES = ["RTW", "world_model", "MAIC"]
GIVEN = [("--td_lambda", "0.3"), ("--ppo_clip", "0.1"), ("--ppo_epochs", "3"), ("--ppo_norm_adv", "False"), ("--noise_dim", "8"),
         ("--lambda_mi", "0.01"), ("--commnet_k", "2"), ("--g2anet_hard", "False"), ("--g2anet_tau", "0.5"), ("--wqmix_alpha", "0.3"),
         ("--qatten_heads", "2"), ("--qatten_embed_dim", "16"), ("--qatten_unit_dim", "8")]
OUT_OF_RANGE = [("--td_lambda", "1.5"), ("--ppo_clip", "1.5"), ("--ppo_epochs", "0"), ("--noise_dim", "33"), ("--lambda_mi", "-1"),
                ("--commnet_k", "0"), ("--g2anet_tau", "0"), ("--wqmix_alpha", "1.5"), ("--qatten_heads", "9"),
                ("--qatten_embed_dim", "0"), ("--qatten_unit_dim", "1000")]
EXTRAS = [()] + [("--" + s, "True") for s in SWITCHES] + GIVEN + OUT_OF_RANGE
BUILD_CASES = list(itertools.product(NAMES, ENVS, MAPS, EXTRAS))

FLAGS = ["RTW", "world_model", "MAIC", "overlap_rollout", "MAIC_train", "mi_loss_weight", "reuse_network"]
FLAG_SETS = list(itertools.product((False, True), repeat=len(FLAGS)))       # True: the flag is away from its default
RUNNER_CASES = list(itertools.product(NAMES, ("bare", "make_runner"), FLAG_SETS))

ENV_CLASSES = ("SyntheticSMACEnv", "BatchedMatrixGame", "BattleEnv", "FusedBattleEnv")
MACS = ("SharedMAC", "SharedMACWithState", "RTWMAC", "MAICMAC", "PolicyMAC", "MAVENMAC", "CommNetMAC", "G2ANetMAC")
LEARNERS = {"q_learner": "QLearner", "qtran_learner": "QTRANLearner", "rtw_q_learner": "RTWQLearner", "q_learner_state": "QLearnerWithState",
            "maic_q_learner": "MAICQLearner", "maic_td_learner": "MAICTDLearner", "central_v": "CentralVLearner",
            "reinforce": "ReinforceLearner", "iql": "IQLLearner", "wqmix": "WQMIXLearner", "maven": "MAVENLearner", "coma": "COMALearner",
            "ppo": "PPOLearner", "lica": "LICALearner"}


def build_id(case):
    name, env, map_, extra = case
    return "|".join((name, env, map_, " ".join(extra)))


def runner_id(case):
    name, how, flags = case
    return "%s|%s|%s" % (name, how, ",".join(f for f, on in zip(FLAGS, flags) if on))


# ------------------------------------------------------------------------------------------------------------ build
def _stub_envs(made):
    """replacements for main's four environment classes: each reports the sizes of the map it was made for"""
    from marl_amd import main
    from marl_amd.env.battle import battle_shapes

    def env_of(n, o, s, a, t):
        made.append(1)
        return type("E", (), {"get_env_info": lambda self: dict(n_actions=a, n_agents=n, state_shape=s, obs_shape=o, episode_limit=t)})()

    synthetic = lambda n_envs, n, o, s, a, t, seed=0: env_of(n, o, s, a, t)
    battle = lambda n_envs, map_, seed=0: env_of(*battle_shapes(map_))
    matrix = lambda payoff, n_envs, seed=0: env_of(2, 1, 1, 3, 1)
    return [mock.patch.object(main, n, f) for n, f in zip(ENV_CLASSES, (synthetic, matrix, battle, battle))]


def eval_build(case):
    """{"args": the namespace} or {"raises": [type, text]}, and "envs": how many environments were made"""
    from marl_amd import main
    name, env, map_, extra = case
    made = []
    with contextlib.ExitStack() as stack:
        for p in _stub_envs(made):
            stack.enter_context(p)
        try:
            args, _ = main.build(["--alg", name, "--env", env, "--map", map_] + list(extra))
            out = {"args": dict(vars(args))}
        except Exception as e:      # (a SystemExit of the parser is not an outcome any case has)
            out = {"raises": [type(e).__name__, str(e)]}
    out["envs"] = len(made)
    return json.loads(json.dumps(out))


# ------------------------------------------------------------------------------------------------------------ Runner
class _Logger:
    def setup_tb(self, path):
        pass


def _classes():
    from marl_amd import rollout
    from marl_amd.common import replaybuffer
    from marl_amd.controller import share_params
    out = [getattr(share_params, n) for n in MACS] + [rollout.RolloutWorker, replaybuffer.ReplayBuffer]
    return out + [getattr(importlib.import_module("marl_amd.algorithm." + m), n) for m, n in LEARNERS.items()]


@contextlib.contextmanager
def recorders(built):
    """every class the runner can build records its name in ``built`` instead of constructing itself"""
    def init(self, *a, **k):
        built.append(type(self).__name__)
    with contextlib.ExitStack() as stack:
        for cls in _classes():
            stack.enter_context(mock.patch.object(cls, "__init__", init))
        yield


_BASE = {}


def _runner_args(name, result_dir):
    """the namespace of ``--alg name`` after the mixer table, with 2s3z's sizes: what a Runner reads before it builds"""
    from marl_amd.common.arguments import get_common_args, get_mixer_args
    if name not in _BASE:
        a = get_mixer_args(get_common_args(["--alg", name]))
        a.env, a.n_agents, a.obs_shape, a.state_shape, a.n_actions, a.episode_limit = "synthetic", 5, 80, 120, 11, 120
        _BASE[name] = a
    a = copy.copy(_BASE[name])
    a.result_dir = result_dir
    return a


def eval_runner(case, result_dir):
    """{"built": [class names in order], "on_policy": bool} or {"raises": [type, text], "built": [...]}; inside ``recorders``"""
    from marl_amd import main, runner
    name, how, flags = case
    args = _runner_args(name, result_dir)
    for flag, on in zip(FLAGS, flags):
        if on:
            setattr(args, flag, {"mi_loss_weight": 0.5, "reuse_network": False}.get(flag, True))
    built = []
    with recorders(built):
        try:
            r = main.make_runner(args, None, _Logger()) if how == "make_runner" else runner.Runner(None, _Logger(), args)
            return {"built": built, "on_policy": r.on_policy}
        except Exception as e:
            return {"raises": [type(e).__name__, str(e)], "built": built}


# ------------------------------------------------------------------------------------------------------------ the fixture's form
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launcher_matrix.json")
_ABSENT = "<absent>"


def _diff(args, base):
    d = {k: v for k, v in args.items() if k not in base or base[k] != v or type(base[k]) is not type(v)}
    d.update({k: _ABSENT for k in base if k not in args})
    return d


def _patched(base, d):
    out = dict(base)
    out.update(d)
    return {k: v for k, v in out.items() if v != _ABSENT}


def _sibling(case):
    name, env, map_, extra = case
    return build_id((name, env, map_, ()))


def pack_build(outcomes):
    """{"raised": [each distinct refusal once], "names": {name: {"full": the first namespace of that name, "env|map": [one entry per
    extra, in EXTRAS' order]}}}.  An entry is the position of the refusal in "raised", or [environments made, the fields of the
    namespace that differ from its sibling's (same --env and --map, no extras) where that case has a namespace, otherwise from "full"]"""
    raised, names = [], {}
    for case in BUILD_CASES:
        out = outcomes[build_id(case)]
        group = names.setdefault(case[0], {"full": None})
        if "args" in out:
            if group["full"] is None:
                group["full"] = out["args"]
            sib = outcomes[_sibling(case)]
            entry = [out["envs"], _diff(out["args"], sib["args"] if "args" in sib and case[3] else group["full"])]
        else:
            if out not in raised:
                raised.append(out)
            entry = raised.index(out)
        group.setdefault("%s|%s" % case[1:3], []).append(entry)
    return {"raised": raised, "names": names}


def unpack_build(packed):
    outcomes = {}
    for case in BUILD_CASES:
        group = packed["names"][case[0]]
        entry = group["%s|%s" % case[1:3]][EXTRAS.index(case[3])]
        if isinstance(entry, int):
            out = packed["raised"][entry]
        else:
            sib = outcomes.get(_sibling(case), {})
            out = {"args": _patched(sib["args"] if "args" in sib and case[3] else group["full"], entry[1]), "envs": entry[0]}
        outcomes[build_id(case)] = out
    return outcomes


def pack_runner(outcomes):
    """{"outcomes": [each distinct outcome once], "cases": {"name|how": [position in "outcomes" per flag set, in FLAG_SETS' order]}}"""
    distinct, cases = [], {}
    for case in RUNNER_CASES:
        out = outcomes[runner_id(case)]
        if out not in distinct:
            distinct.append(out)
        cases.setdefault("%s|%s" % case[:2], []).append(distinct.index(out))
    return {"outcomes": distinct, "cases": cases}


def unpack_runner(packed):
    return {runner_id(case): packed["outcomes"][packed["cases"]["%s|%s" % case[:2]][FLAG_SETS.index(case[2])]] for case in RUNNER_CASES}


def load():
    with open(PATH) as f:
        data = json.load(f)
    return unpack_build(data["build"]), unpack_runner(data["runner"])
