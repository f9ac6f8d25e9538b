"""Argument helpers (mirror of reference common/arguments.py:9-45, 86-147): every function the reference's callers
import (matrix_game_test.py:9, main.py:3) exists with the same name and effect.  Booleans parse properly here (the
reference's ``type=bool`` treats any non-empty string as True), and ``--RTW`` / ``--load_model``
default to False: the RTW research variant is outside the hot path and no checkpoint ships with this build."""
import argparse
import numbers


def _bool(v):
    if isinstance(v, bool):
        return v
    return str(v).lower() not in ("", "0", "false", "no", "none")


def get_common_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--RTW', type=_bool, default=False)
    # not in the reference's parser (its runner never builds SharedMACWithState + QLearnerWithState): the world-model agent
    p.add_argument('--world_model', type=_bool, default=False)
    # the reference's parser has no switch for its MAIC agent (network/MAIC.py) either: MAICMAC, inference and rollouts only ...
    p.add_argument('--MAIC', type=_bool, default=False)
    # ... and with --MAIC_train the learner that trains it on the TD loss (MAICTDLearner; needs --MAIC)
    p.add_argument('--MAIC_train', type=_bool, default=False)
    # the weights of the agent's MI and attention-entropy losses (network/MAIC.py:88-123) in MAICTDLearner's loss; 0 = TD only
    p.add_argument('--mi_loss_weight', type=float, default=0.0)
    p.add_argument('--entropy_loss_weight', type=float, default=0.0)
    # TD(lambda) returns as the Q learners' targets (the reference ships utils/rl_utils.py:build_td_lambda_targets and never calls
    # it); absent = None = the one-step target.  get_mixer_args leaves the field alone: a namespace without it means "off"
    p.add_argument('--td_lambda', type=float, default=None)
    # weight of the entropy bonus on the actor loss of the policy-gradient learners (central_v, reinforce, coma); the reference's tables
    # carry entropy_coefficient = 0.001 and nothing reads it.  (--entropy_loss_weight is MAIC's attention entropy)
    p.add_argument('--policy_entropy_coef', type=float, default=0.0)
    # communication rounds of the +commnet actors; absent = get_commnet_args' table (2 on map 3m, otherwise 3)
    p.add_argument('--commnet_k', type=int, default=None)
    # the +g2anet actors: hard attention on / off and its temperature; absent = get_g2anet_args' True and the published 0.01
    p.add_argument('--g2anet_hard', type=_bool, default=None)
    p.add_argument('--g2anet_tau', type=float, default=None)
    # --alg mappo: the surrogate's clip c in (0, 1), the passes over one rollout and whether the advantage is standardised over the
    # live steps; absent = get_mappo_args' 0.2, 5 and True
    p.add_argument('--ppo_clip', type=float, default=None)
    p.add_argument('--ppo_epochs', type=int, default=None)
    p.add_argument('--ppo_norm_adv', type=_bool, default=None)
    # --alg qatten: attention heads, embedding width and the width of an agent's unit features in the state row; absent =
    # get_qatten_args' 4, 32 and state_shape // n_agents
    p.add_argument('--qatten_heads', type=int, default=None)
    p.add_argument('--qatten_embed_dim', type=int, default=None)
    p.add_argument('--qatten_unit_dim', type=int, default=None)
    # --alg ow_qmix / cw_qmix: the weight alpha in [0, 1] of the steps the weighting holds back; absent = get_wqmix_args' 0.5 / 0.75
    p.add_argument('--wqmix_alpha', type=float, default=None)
    # --alg maven: the number of noise values K in [1, 32] and the weight of the mutual-information term (>= 0); absent = the table's
    # noise_dim = 16 and lambda_mi = 0.001 (get_mixer_args / get_maven_args)
    p.add_argument('--noise_dim', type=int, default=None)
    p.add_argument('--lambda_mi', type=float, default=None)
    p.add_argument('--env', type=str, default='smac')
    # --env battle: the environment with the fused step and the whole-rollout kernel (env/battle.py: FusedBattleEnv)
    p.add_argument('--battle_fused', type=_bool, default=False)
    p.add_argument('--difficulty', type=str, default='7')
    p.add_argument('--game_version', type=str, default='latest')
    p.add_argument('--map', type=str, default='2s3z')
    p.add_argument('--seed', type=int, default=123)
    p.add_argument('--step_mul', type=int, default=8)
    p.add_argument('--replay_dir', type=str, default='')
    p.add_argument('--alg', type=str, default='qmix')
    p.add_argument('--n_steps', type=int, default=800000)
    p.add_argument('--n_episodes', type=int, default=1)
    p.add_argument('--last_action', type=_bool, default=True)
    p.add_argument('--reuse_network', type=_bool, default=True)
    p.add_argument('--gamma', type=float, default=0.99)
    p.add_argument('--optimizer', type=str, default="RMS")
    p.add_argument('--evaluate_cycle', type=int, default=5000)
    p.add_argument('--evaluate_epoch', type=int, default=0)
    p.add_argument('--model_dir', type=str, default='./model')
    p.add_argument('--result_dir', type=str, default='./result')
    p.add_argument('--load_model', type=_bool, default=False)
    p.add_argument('--evaluate', type=_bool, default=False)
    p.add_argument('--cuda', type=_bool, default=True)
    p.add_argument('--n_envs', type=int, default=1, help='parallel environments for the batched rollout')
    return p.parse_args(argv)


def get_mixer_args(args):
    args.rnn_hidden_dim = 64
    args.qmix_hidden_dim = 32
    args.two_hyper_layers = False
    if not hasattr(args, "mixer_dtype"):
        args.mixer_dtype = "fp32"     # build extension (BASELINE config 5): "bf16" = mixer GEMMs on the bf16 matrix cores
    args.hyper_hidden_dim = 64
    args.qtran_hidden_dim = 64
    args.lr = 5e-4
    args.epsilon = 1
    args.min_epsilon = 0.05
    anneal_steps = 50000
    args.anneal_epsilon = (args.epsilon - args.min_epsilon) / anneal_steps
    args.epsilon_anneal_scale = 'step'
    args.train_steps = 1
    args.batch_size = 32
    args.buffer_size = int(5e3)
    args.save_cycle = 5000
    args.target_update_cycle = 200
    args.lambda_opt = 1
    args.lambda_nopt = 1
    args.grad_norm_clip = 10
    args.noise_dim, args.lambda_mi, args.lambda_ql, args.entropy_coefficient = 16, 0.001, 1, 0.001   # MAVEN (--alg maven reads the first two: get_maven_args)
    args.adv_hypernet_embed = 64
    args.num_kernel = 10
    args.adv_hypernet_layers = 3
    args.weighted_head = True
    args.hypernet_embed = 64
    args.is_minus_one = True
    args.mixing_embed_dim = 32
    args.double_q = True
    return args


# ---- hyper-parameter tables of the algorithms outside the hot path (reference common/arguments.py:48-83,151-214).
# Nothing in marl_amd reads these fields; the functions exist because the reference's entry scripts import them
# (matrix_game_test.py:9, main.py:3) and main.py:12 calls get_RTW_args on every run.
_ACTOR_CRITIC = dict(rnn_hidden_dim=64, critic_dim=128, lr_actor=1e-4, lr_critic=1e-3, epsilon=0.5,
                     anneal_epsilon=0.00064, min_epsilon=0.02, epsilon_anneal_scale='episode', save_cycle=5000,
                     grad_norm_clip=10)


def _assign(args, table):
    for k, v in table.items():
        setattr(args, k, v)
    return args


def get_RTW_args(args):
    """reference :48-53 (returns None there as well)"""
    _assign(args, dict(world_loss_weight=1, teammate_loss_weight=1, hidden_dim=64, attn_dim=64, not_self_model=True))


def get_maic_args(args):
    """The MAIC agent's sizes (network/MAIC.py:13-17,59-61 reads them from args).  The reference's arguments.py sets only
    attention_dim = 32 (:215, get_g2anet_args); latent_dim 8, nn_hidden_size 64 and var_floor 0.002 are the MAIC paper's
    defaults.  Values the caller already set are kept."""
    for k, v in dict(latent_dim=8, nn_hidden_size=64, var_floor=0.002, attention_dim=32).items():
        if not hasattr(args, k):
            setattr(args, k, v)
    return args


def get_coma_args(args):
    """reference :56-83"""
    return _assign(args, dict(_ACTOR_CRITIC, td_lambda=0.8, target_update_cycle=200))


def get_centralv_args(args):
    """reference :151-177"""
    return _assign(args, dict(_ACTOR_CRITIC, td_lambda=0.8, target_update_cycle=200))


def get_lica_args(args):
    """This project's own table for LICA (the reference ships none): the actor-critic fields of central-V, td_lambda = 0.8 and a
    target critic that follows every 200 updates.  The critic's widths, mixing_embed_dim and hypernet_embed, stay get_mixer_args'."""
    return _assign(args, dict(_ACTOR_CRITIC, td_lambda=0.8, target_update_cycle=200))


def get_mappo_args(args):
    """This project's own table (the reference ships none for PPO): the actor-critic fields of central-V, td_lambda = 0.95 (with
    adv = G - V that is GAE(0.95)), clip 0.2, five passes over a rollout, standardised advantages.  There is no target network, so
    no target_update_cycle is set here.  ``args.optimizer`` stays as given: the MAPPO paper's Adam at 5e-4 is not imposed - the
    learning rates are the table's lr_actor / lr_critic with whichever optimizer the user named."""
    return _assign(args, dict(_ACTOR_CRITIC, td_lambda=0.95, ppo_clip=0.2, ppo_epochs=5, ppo_norm_adv=True))


def get_reinforce_args(args):
    """reference :181-200.  Its table has no td_lambda: the parser's unset (None) --td_lambda is taken off again, so the namespace
    has the reference's fields (a value the user gave stays)"""
    if getattr(args, "td_lambda", 0) is None:
        del args.td_lambda
    return _assign(args, dict(_ACTOR_CRITIC))


def get_commnet_args(args):
    """reference :204-209"""
    args.k = 2 if args.map == '3m' else 3
    return args


def get_g2anet_args(args):
    """reference :212-215"""
    return _assign(args, dict(attention_dim=32, hard=True))


WQMIX_ALGS = ('ow_qmix', 'cw_qmix')


def wqmix_alpha_of(args):
    """args.wqmix_alpha, a number in [0, 1] (unset: get_wqmix_args' 0.5 for ow_qmix, 0.75 for cw_qmix); anything else is an error"""
    alpha = getattr(args, "wqmix_alpha", None)
    if alpha is None:
        alpha = 0.5 if args.alg == 'ow_qmix' else 0.75
    if isinstance(alpha, bool) or not 0.0 <= alpha <= 1.0:
        raise ValueError("wqmix_alpha must be a number in [0, 1], got %r" % (alpha,))
    return float(alpha)


def get_wqmix_args(args):
    """This project's own table for Weighted QMIX (the reference ships none): wqmix_alpha = 0.5 for ow_qmix and 0.75 for cw_qmix
    (the paper's SMAC values) and central_mixing_embed_dim = 256.  Values the caller set (not None) are kept; an alpha outside
    [0, 1] is a ValueError."""
    for k, v in dict(wqmix_alpha=wqmix_alpha_of(args), central_mixing_embed_dim=256).items():
        if getattr(args, k, None) is None:
            setattr(args, k, v)
    return args


def noise_dim_of(args):
    """args.noise_dim as the kernels take it: an int in [1, 32]; anything else is an error"""
    K = getattr(args, "noise_dim", None)
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= 32:
        raise ValueError("noise_dim must be an integer in [1, 32], got %r" % (K,))
    return K


def lambda_mi_of(args):
    """args.lambda_mi: a number >= 0; anything else is an error"""
    lam = getattr(args, "lambda_mi", None)
    if isinstance(lam, bool) or not isinstance(lam, numbers.Real) or not lam >= 0.0:
        raise ValueError("lambda_mi must be a number >= 0, got %r" % (lam,))
    return float(lam)


def get_maven_args(args):
    """This project's own table for MAVEN (the reference's tables carry noise_dim = 16 and lambda_mi = 0.001 and ship no MAVEN to
    read them): those two and the discriminator's width maven_discrim_dim = 64.  Values the caller set (not None) are kept; a
    noise_dim outside [1, 32] or a negative lambda_mi is a ValueError."""
    for k, v in dict(noise_dim=16, lambda_mi=0.001, maven_discrim_dim=64).items():
        if getattr(args, k, None) is None:
            setattr(args, k, v)
    noise_dim_of(args)
    lambda_mi_of(args)
    return args


def get_qatten_args(args):
    """This project's own table for the Qatten mixer (the reference ships none): 4 heads, embedding width 32, and the unit features
    of agent i are columns [i U, (i + 1) U) of the state row with U = state_shape // n_agents (24 at 2s3z, 27 at 3s5z, 32 at MMM2,
    whose last 2 of 322 state columns are then no unit's).  Called once the environment's sizes are known; values the caller set
    (not None) are kept."""
    for k, v in dict(qatten_heads=4, qatten_embed_dim=32, qatten_unit_dim=args.state_shape // args.n_agents).items():
        if getattr(args, k, None) is None:
            setattr(args, k, v)
    return args
