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

``--env synthetic`` (default) uses the synthetic SMAC-shaped device env with the dims of ``--map``;
``--env matrix`` the batched two-agent matrix game; ``--env battle`` the micro-combat simulator in SMAC's layout (env/battle.py:
maps 3m, 2s3z, 3s5z), the one environment here whose outcome depends on the actions.  StarCraft II itself is not vendored by the
reference."""
from __future__ import annotations

import sys
from collections import namedtuple

from .common.arguments import get_common_args, get_mixer_args, get_RTW_args, get_maic_args, get_centralv_args, \
    get_reinforce_args, get_coma_args, get_commnet_args, get_g2anet_args, get_mappo_args, get_qatten_args, get_lica_args, get_wqmix_args, get_maven_args, WQMIX_ALGS
from .env.synthetic_smac import SyntheticSMACEnv
from .env.single_state_matrix_game import BatchedMatrixGame
from .env.battle import BattleEnv, FusedBattleEnv, battle_shapes
from .runner import Runner
from .utils.logging import Logger

MAPS = {"2s3z": (5, 80, 120, 11, 120), "3s5z": (8, 128, 216, 14, 150), "MMM2": (10, 176, 322, 18, 120)}


COMMNET = '+commnet'
G2ANET = '+g2anet'
_POLICY_ALGS = ('central_v', 'coma', 'reinforce')


def _map_shapes(args):
    """(agents, observation, state, actions, episode limit) of --map, known before the environment is made: ``MAPS`` for the synthetic
    environment, the battle environment's own table for ``--env battle`` (a map it does not have is a ValueError); None otherwise"""
    if args.env == 'battle':
        return battle_shapes(args.map)
    return MAPS[args.map] if args.env in ('smac', 'synthetic') else None


def _map_counts(args):
    """(agents, actions) of --map, known before the environment is made; (2, 1) where no map says them"""
    shapes = _map_shapes(args)
    return (shapes[0], shapes[3]) if shapes is not None else (2, 1)


# What the launcher does for an actor suffix.  table: the argument table (commnet: k = 2 on map 3m, otherwise 3; g2anet: attention_dim =
# 32, hard = True); switch: the command-line override (argparse has typed it) of the table's ``sets``; check: the shape check of
# controller.share_params (a name: imported when it runs) and early: the (agents, actions) it is handed before the environment is
# made - CommNet's range of k depends on nothing else, G2ANet's is the map's counts (a bad --g2anet_tau is refused all the same);
# mac: the controller class, by name as well
_Actor = namedtuple('_Actor', 'name title table switch sets check early mac')
_ACTORS = {COMMNET: _Actor(name='commnet', title='CommNet', table=get_commnet_args, switch='commnet_k', sets='k',
                           check='commnet_k_of', early=lambda args: (2, 1), mac='CommNetMAC'),
           G2ANET: _Actor(name='g2anet', title='G2ANet', table=get_g2anet_args, switch='g2anet_hard', sets='hard',
                          check='g2anet_shape_of', early=_map_counts, mac='G2ANetMAC')}


def _share(name):
    from .controller import share_params
    return getattr(share_params, name)


def actor_base(alg, entry=False):
    """'coma+commnet' -> ('coma', 'commnet'), 'reinforce+g2anet' -> ('reinforce', 'g2anet'); (alg, None) for a name without such a
    suffix.  The communicating actors belong to the policy-gradient learners: any other base is an error.  ``entry``: the _ACTORS
    entry in the place of the actor's name"""
    for suffix, a in _ACTORS.items():
        if alg.endswith(suffix):
            base = alg[:-len(suffix)]
            if base not in _POLICY_ALGS:
                raise ValueError("%s: the %s actor is trained by central_v, coma or reinforce, not by %r" % (alg, a.title, base))
            return base, (a if entry else a.name)
    return alg, None


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


def _lica(args):
    """the LICA critic's shape check: agents, actions or mixing_embed_dim outside the row kernels' range are a ValueError here"""
    from .algorithm.lica import lica_shape_of
    lica_shape_of(args)


def _maven(args, early=False):
    """the MAVEN kernels' shape check (network/maven.py: maven_shape_of): a noise_dim, a lambda_mi or sizes outside their range are
    a ValueError here.  ``early``: with the map's sizes, before the environment is made (the matrix game: 2 agents, 3 actions, width 1)"""
    from .network.maven import maven_shape_of
    if early:
        shapes = _map_shapes(args)
        n, s, a = (shapes[0], shapes[2], shapes[3]) if shapes is not None else (2, 1, 3)
        maven_shape_of(args, n_agents=n, n_actions=a, state_shape=s)
    else:
        maven_shape_of(args)


def build(argv=None):
    args = get_common_args(argv)
    given_maven = (args.noise_dim, args.lambda_mi)      # get_mixer_args assigns the table's values over them
    get_mixer_args(args)
    if args.alg == 'maven':
        on = [sw for sw in ('RTW', 'world_model', 'MAIC') if getattr(args, sw, False)]
        if on:
            raise ValueError("maven trains the noise-conditioned shared agent in MAVENLearner: not with %s" % on[0])
        for k, v in zip(('noise_dim', 'lambda_mi'), given_maven):
            if v is not None:           # the table's values are defaults, not overrides of the switches
                setattr(args, k, v)
        get_maven_args(args)            # a bad --noise_dim / --lambda_mi is refused before anything is built
    if args.env == 'battle':
        battle_shapes(args.map)         # a map the battle environment does not have is refused before anything is built
    base, actor = actor_base(args.alg, entry=True)           # raises on a Q-learning algorithm with an actor suffix
    if actor is not None:
        on = [sw for sw in ('RTW', 'world_model', 'MAIC') if getattr(args, sw, False)]
        if on:
            raise ValueError("%s trains the %s actor as a policy: not with %s" % (args.alg, actor.title, on[0]))
    if base in ('central_v', 'coma', 'lica'):      # (an actor suffix on lica was refused above: _POLICY_ALGS does not hold the name)
        given = args.td_lambda
        {'central_v': get_centralv_args, 'coma': get_coma_args, 'lica': get_lica_args}[base](args)
        if given is not None:           # the table's 0.8 is the default, not an override of --td_lambda
            args.td_lambda = given
    elif base == 'reinforce':
        get_reinforce_args(args)
    elif base == 'mappo':               # (an actor suffix on it was refused above: _POLICY_ALGS does not hold the name)
        given = {k: getattr(args, k) for k in ('td_lambda', 'ppo_clip', 'ppo_epochs', 'ppo_norm_adv')}
        get_mappo_args(args)
        for k, v in given.items():      # the table's values are defaults, not overrides of the switches
            if v is not None:
                setattr(args, k, v)
        from .algorithm.ppo import ppo_settings_of
        ppo_settings_of(args)           # a bad --ppo_clip / --ppo_epochs is refused before the environment is made
    if actor is not None:
        actor.table(args)
        if getattr(args, actor.switch, None) is not None:
            setattr(args, actor.sets, getattr(args, actor.switch))
        n, a = actor.early(args)
        _share(actor.check)(args, n_agents=n, n_actions=a)      # refused before the environment is made
    get_RTW_args(args)
    get_maic_args(args)
    if args.alg in WQMIX_ALGS:          # Weighted QMIX (WQMIXLearner): the table's alpha and central width; a --wqmix_alpha outside
        get_wqmix_args(args)            # [0, 1] is refused before the environment is made
    if args.alg == 'qatten':            # the sizes the environment will report are the map's (the matrix game: 2 agents, state width 1):
        shapes = _map_shapes(args)
        args.n_agents, args.state_shape = (shapes[0], shapes[2]) if shapes is not None else (2, 1)
        _qatten(args)                   # refused before the environment is made
    if args.alg == 'lica':              # likewise: the map's agent, action and state sizes (the matrix game: 2 agents, 3 actions, width 1)
        shapes = _map_shapes(args)
        args.n_agents, args.n_actions, args.state_shape = (shapes[0], shapes[3], shapes[2]) if shapes is not None else (2, 3, 1)
        _lica(args)                     # refused before the environment is made
    if args.alg == 'maven':
        _maven(args, early=True)        # refused before the environment is made
    if args.env == 'smac':
        args.env = 'synthetic'
    if args.env == 'synthetic':
        n, o, s, a, t = MAPS[args.map]
        env = SyntheticSMACEnv(args.n_envs, n, o, s, a, t, seed=args.seed)
    elif args.env == 'battle':
        env = (FusedBattleEnv if args.battle_fused else BattleEnv)(args.n_envs, args.map, seed=args.seed)
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
    if args.alg == 'qatten':
        _qatten(args)                   # ... and with the environment's own sizes
    if args.alg == 'lica':
        _lica(args)
    if args.alg == 'maven':
        _maven(args)
    if actor is not None:
        _share(actor.check)(args)       # ... and the environment's agent and action counts with it, before a controller is built
    return args, env


def make_runner(args, env, logger=None):
    """the Runner of a built (args, env).  ``--alg coma`` names its learner here: the runner's own table of on-policy learners
    holds central_v and reinforce, and a Runner built on the bare name 'coma' still refuses it; ``--alg mappo`` (PPOLearner) and
    ``--alg lica`` (LICALearner) likewise (with RTW, world_model or MAIC the runner refuses them as it refuses central_v).  The algorithms with an actor suffix
    get their learner class and their actor's controller (``mac_cls``, the _ACTORS entry's) the same way."""
    learner_cls = mac_cls = None
    base, actor = actor_base(args.alg, entry=True)
    if base == 'coma':
        from .algorithm.coma import COMALearner
        learner_cls = COMALearner
    elif base == 'mappo':
        from .algorithm.ppo import PPOLearner
        learner_cls = PPOLearner
    elif base == 'lica':
        from .algorithm.lica import LICALearner
        learner_cls = LICALearner
    elif actor is not None:             # the names with an actor suffix are the launcher's: the runner's own table does not hold them
        from .algorithm.central_v import CentralVLearner
        from .algorithm.reinforce import ReinforceLearner
        learner_cls = CentralVLearner if base == 'central_v' else ReinforceLearner
    if actor is not None:
        mac_cls = _share(actor.mac)
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
