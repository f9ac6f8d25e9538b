"""smac-free launcher (counterpart of reference main.py:7-44):

    python -m marl_amd.main --alg qmix --map 2s3z --n_envs 1024 --n_steps 500000
    python -m marl_amd.main --env matrix --alg qplex --n_envs 32 --n_steps 20000
    python -m marl_amd.main --map 2s3z --alg central_v --n_envs 64 --n_steps 200000
    python -m marl_amd.main --map 2s3z --alg coma --n_envs 64 --n_steps 200000
    python -m marl_amd.main --map 2s3z --alg reinforce --policy_entropy_coef 0.01 --n_envs 64 --n_steps 200000
    python -m marl_amd.main --map 2s3z --alg reinforce+commnet --n_envs 64 --n_steps 200000
    python -m marl_amd.main --map 2s3z --alg central_v+commnet --commnet_k 2 --n_envs 64 --n_steps 200000
    python -m marl_amd.main --map 2s3z --alg coma+commnet --n_envs 64 --n_steps 200000
    python -m marl_amd.main --map 2s3z --MAIC True --load_model True --evaluate True --evaluate_epoch 1 --n_envs 64

``--env synthetic`` (default) uses the synthetic SMAC-shaped device env with the dims of ``--map``;
``--env matrix`` the batched two-agent matrix game.  StarCraft II itself is not vendored by the reference."""
from __future__ import annotations

import sys

from .common.arguments import get_common_args, get_mixer_args, get_RTW_args, get_maic_args, get_centralv_args, \
    get_reinforce_args, get_coma_args, get_commnet_args
from .env.synthetic_smac import SyntheticSMACEnv
from .env.single_state_matrix_game import BatchedMatrixGame
from .runner import Runner
from .utils.logging import Logger

MAPS = {"2s3z": (5, 80, 120, 11, 120), "3s5z": (8, 128, 216, 14, 150), "MMM2": (10, 176, 322, 18, 120)}


COMMNET = '+commnet'
_POLICY_ALGS = ('central_v', 'coma', 'reinforce')


def commnet_base(alg):
    """'coma+commnet' -> 'coma'; None for a name without the suffix.  The communicating actor belongs to the policy-gradient
    learners: any other base is an error."""
    if not alg.endswith(COMMNET):
        return None
    base = alg[:-len(COMMNET)]
    if base not in _POLICY_ALGS:
        raise ValueError("%s: the CommNet actor is trained by central_v, coma or reinforce, not by %r" % (alg, base))
    return base


def build(argv=None):
    args = get_common_args(argv)
    get_mixer_args(args)
    commnet = commnet_base(args.alg)             # raises on a Q-learning algorithm with +commnet
    if commnet is not None:
        on = [sw for sw in ('RTW', 'world_model', 'MAIC') if getattr(args, sw, False)]
        if on:
            raise ValueError("%s trains the CommNet actor as a policy: not with %s" % (args.alg, on[0]))
    base = commnet if commnet is not None else args.alg
    if base in ('central_v', 'coma'):
        given = args.td_lambda
        (get_centralv_args if base == 'central_v' else get_coma_args)(args)
        if given is not None:           # the table's 0.8 is the default, not an override of --td_lambda
            args.td_lambda = given
    elif base == 'reinforce':
        get_reinforce_args(args)
    if commnet is not None:
        get_commnet_args(args)          # k = 2 on map 3m, otherwise 3
        if getattr(args, "commnet_k", None) is not None:
            args.k = args.commnet_k
        from .controller.share_params import commnet_k_of
        commnet_k_of(args, n_agents=2, n_actions=1)     # the range of k depends on nothing else: refused before the environment is made
    get_RTW_args(args)
    get_maic_args(args)
    if args.env == 'smac':
        args.env = 'synthetic'
    if args.env == 'synthetic':
        n, o, s, a, t = MAPS[args.map]
        env = SyntheticSMACEnv(args.n_envs, n, o, s, a, t, seed=args.seed)
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
    if commnet is not None:
        commnet_k_of(args)              # ... and the environment's agent and action counts with it, before a controller is built
    return args, env


def make_runner(args, env, logger=None):
    """the Runner of a built (args, env).  ``--alg coma`` names its learner here: the runner's own table of on-policy learners
    holds central_v and reinforce, and a Runner built on the bare name 'coma' still refuses it.  The three ``+commnet`` algorithms get
    their learner class and CommNetMAC (``mac_cls``) the same way."""
    learner_cls = mac_cls = None
    commnet = commnet_base(args.alg)
    if args.alg == 'coma' or commnet == 'coma':
        from .algorithm.coma import COMALearner
        learner_cls = COMALearner
    elif commnet is not None:           # the +commnet names are the launcher's: the runner's own table does not hold them
        from .algorithm.central_v import CentralVLearner
        from .algorithm.reinforce import ReinforceLearner
        learner_cls = CentralVLearner if commnet == 'central_v' else ReinforceLearner
    if commnet is not None:
        from .controller.share_params import CommNetMAC
        mac_cls = CommNetMAC
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
