"""smac-free launcher (counterpart of reference main.py:7-44):

    python -m marl_amd.main --alg qmix --map 2s3z --n_envs 1024 --n_steps 500000
    python -m marl_amd.main --env matrix --alg qplex --n_envs 32 --n_steps 20000
    python -m marl_amd.main --map 2s3z --alg iql --n_envs 1024 --n_steps 500000
    python -m marl_amd.main --map 2s3z --alg qatten --qatten_heads 4 --n_envs 1024 --n_steps 500000
    python -m marl_amd.main --env matrix --alg ow_qmix --n_envs 32 --n_steps 20000
    python -m marl_amd.main --env battle --map 3m --alg cw_qmix --wqmix_alpha 0.75 --n_envs 64 --n_steps 200000
    python -m marl_amd.main --map 2s3z --alg central_v --n_envs 64 --n_steps 200000
    python -m marl_amd.main --map 2s3z --alg coma --n_envs 64 --n_steps 200000
    python -m marl_amd.main --map 2s3z --alg reinforce --policy_entropy_coef 0.01 --n_envs 64 --n_steps 200000
    python -m marl_amd.main --map 2s3z --alg mappo --ppo_epochs 5 --ppo_clip 0.2 --n_envs 64 --n_steps 200000
    python -m marl_amd.main --map 2s3z --alg lica --policy_entropy_coef 0.01 --n_envs 64 --n_steps 200000
    python -m marl_amd.main --map 2s3z --alg reinforce+commnet --n_envs 64 --n_steps 200000
    python -m marl_amd.main --map 2s3z --alg central_v+commnet --commnet_k 2 --n_envs 64 --n_steps 200000
    python -m marl_amd.main --map 2s3z --alg coma+commnet --n_envs 64 --n_steps 200000
    python -m marl_amd.main --map 2s3z --alg reinforce+g2anet --n_envs 64 --n_steps 200000
    python -m marl_amd.main --map 2s3z --alg central_v+g2anet --g2anet_hard False --n_envs 64 --n_steps 200000
    python -m marl_amd.main --map 2s3z --alg coma+g2anet --n_envs 64 --n_steps 200000
    python -m marl_amd.main --map 2s3z --MAIC True --load_model True --evaluate True --evaluate_epoch 1 --n_envs 64
    python -m marl_amd.main --env battle --map 3m --alg qmix --n_envs 64 --n_steps 200000
    python -m marl_amd.main --env battle --map 3m --alg maven --noise_dim 16 --lambda_mi 0.001 --n_envs 64 --n_steps 200000
    python -m marl_amd.main --env hunt --map 4v2 --alg qmix --n_envs 64 --n_steps 200000
    python -m marl_amd.main --env hunt --map 4v2_p2 --alg cw_qmix --n_envs 64 --n_steps 200000

``--env synthetic`` (default) uses the synthetic SMAC-shaped device env with the dims of ``--map``;
``--env matrix`` the batched two-agent matrix game; ``--env battle`` the micro-combat simulator in SMAC's layout (env/battle.py:
maps 3m, 2s3z, 3s5z), whose outcome depends on the actions; ``--env hunt`` predator-prey with a lone-catch penalty (env/hunt.py: maps
2v1, 4v2, 8v8, each with an optional penalty suffix as in 4v2_p2 or 8v8_p1.5), the task monotonic mixing fails on.  StarCraft II
itself is not vendored by the reference."""
from __future__ import annotations

import importlib
import sys

from . import runner as _runner
from .algorithms import COMMNET, G2ANET, _ACTORS, actor_base, lookup  # noqa: F401  (_ACTORS: the one actor table, seen from here too)
from .common.arguments import get_common_args, get_mixer_args, get_RTW_args, get_maic_args, get_qatten_args
from .env.synthetic_smac import SyntheticSMACEnv
from .env.single_state_matrix_game import BatchedMatrixGame
from .env.battle import BattleEnv, FusedBattleEnv, battle_shapes
from .env.hunt import HuntEnv, hunt_shapes
from .runner import Runner, switches_on
from .utils.logging import Logger

MAPS = {"2s3z": (5, 80, 120, 11, 120), "3s5z": (8, 128, 216, 14, 150), "MMM2": (10, 176, 322, 18, 120)}
_MATRIX_GAME = (2, 1, 1, 3, 1)
_SIZE_AT = dict(n_agents=0, state_shape=2, n_actions=3)


def _map_shapes(args):
    """(agents, observation, state, actions, episode limit) of --map, known before the environment is made: ``MAPS`` for the synthetic
    environment, the battle and hunt environments' own tables for ``--env battle`` / ``--env hunt`` (a map they do not have is a
    ValueError); where no map says them, the matrix game's"""
    if args.env == 'battle':
        return battle_shapes(args.map)
    if args.env == 'hunt':
        return hunt_shapes(args.map)
    return MAPS[args.map] if args.env in ('smac', 'synthetic') else _MATRIX_GAME


def commnet_base(alg):
    """'coma+commnet' -> 'coma'; None for a name without the suffix.  The communicating actor belongs to the policy-gradient
    learners: any other base is an error."""
    base, actor = actor_base(alg) if alg.endswith(COMMNET) else (None, None)
    return base if actor == 'commnet' else None


def _qatten(args):
    """get_qatten_args' table (4 heads, embedding 32, U = state_shape // n_agents; --qatten_* values stay) and the mixer's shape check:
    a state too narrow for a block of at least one column per agent (the matrix game), N U > S or a shape outside the row kernel's
    range is a ValueError here"""
    from .network.mixer import qatten_shape_of
    get_qatten_args(args)
    qatten_shape_of(args)


def _check(row, args, early=False):
    """the row's check.  ``early``: before the environment is made, on the sizes it will report (the row's ``early``)"""
    if row.check is None:
        return
    if early:
        for k, v in row.early.items():  # (the map is looked up where a size is asked of it: a map nobody has is the environment's to refuse)
            setattr(args, k, _map_shapes(args)[_SIZE_AT[k]] if v is None else v)
    module, name = row.check.split(':')
    getattr(importlib.import_module('.' + module, __package__), name)(args)


def build(argv=None):
    args = get_common_args(argv)
    row = lookup(args.alg)
    kept = {k: getattr(args, k) for k in row.keeps if getattr(args, k) is not None}
    get_mixer_args(args)
    on = [sw.name for sw in switches_on(args)]
    if on and row.at_launch:            # (maven's: before its table and the battle-map check, where it has always been)
        raise ValueError(row.no_switch % (args.alg, on[0]))
    vars(args).update(kept)             # get_mixer_args' values are defaults, not overrides of the switches: a table that validates
    if row.table is not None:           # (get_maven_args) sees the given ones ...
        row.table(args)
    vars(args).update(kept)             # ... and so are a table's
    if args.env == 'battle':
        battle_shapes(args.map)         # a map the battle environment does not have is refused before anything is built
    if args.env == 'hunt':
        hunt_shapes(args.map)           # (and one the hunt environment does not have, penalty suffix included)
    _, actor = actor_base(args.alg, entry=True)              # raises on any other algorithm with an actor suffix
    if actor is not None and on:
        raise ValueError("%s trains the %s actor as a policy: not with %s" % (args.alg, actor.title, on[0]))
    get_RTW_args(args)
    get_maic_args(args)
    _check(row, args, early=True)       # refused before the environment is made
    if args.env == 'smac':
        args.env = 'synthetic'
    if args.env == 'synthetic':
        n, o, s, a, t = MAPS[args.map]
        env = SyntheticSMACEnv(args.n_envs, n, o, s, a, t, seed=args.seed)
    elif args.env == 'battle':
        env = (FusedBattleEnv if args.battle_fused else BattleEnv)(args.n_envs, args.map, seed=args.seed)
    elif args.env == 'hunt':
        env = HuntEnv(args.n_envs, args.map, seed=args.seed)
    elif args.env == 'matrix':
        env = BatchedMatrixGame([[8, -12, -12], [-12, 0, 0], [-12, 0, 0]], args.n_envs, seed=args.seed)
        args.map = 'MatrixGame'
    else:
        raise ValueError("env not found")
    info = env.get_env_info()
    args.n_actions, args.n_agents = info["n_actions"], info["n_agents"]
    args.state_shape, args.obs_shape, args.episode_limit = info["state_shape"], info["obs_shape"], info["episode_limit"]
    args.batch_size = max(args.batch_size, args.n_envs)
    args.buffer_size = max(2 * args.n_envs, min(args.buffer_size, 8 * args.n_envs))
    _check(row, args)                   # ... and with the environment's own sizes, before a controller is built
    return args, env


def make_runner(args, env, logger=None):
    """the Runner of a built (args, env).  The rows that are ``launcher_only`` get their learner and controller named here, as
    ``learner_cls`` / ``mac_cls``: a Runner built on such a bare name keeps refusing it."""
    actor_base(args.alg)                # raises on a refused actor suffix
    row = lookup(args.alg)
    learner_cls, mac_cls = (getattr(_runner, row.learner), getattr(_runner, row.mac)) if row.launcher_only else (None, None)
    return Runner(env, logger if logger is not None else Logger(), args, learner_cls=learner_cls, mac_cls=mac_cls)


def main(argv=None):
    args, env = build(argv)
    runner = make_runner(args, env)
    if not args.evaluate:
        loss = runner.run(0)
        print("final loss", loss)
    else:
        win_rate, _ = runner.evaluate()
        print('The win rate of {} is  {}'.format(args.alg, win_rate))
    env.close()


if __name__ == '__main__':
    main(sys.argv[1:])
