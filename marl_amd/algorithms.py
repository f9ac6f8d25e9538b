"""The algorithm table: one row per ``--alg`` name says everything the launcher (main.py) and the Runner need to know about it.
Plain data and a lookup; adding an algorithm is adding a row here (and its learner's import in runner.py).

    table          the get_*_args function main.build applies after get_mixer_args, or None
    keeps          command-line fields whose given (non-None) value survives get_mixer_args and ``table``: those are defaults
    check          'module:function' under marl_amd, resolved when it runs: the shape or settings check main.build calls as check(args)
                   before the environment is made and again after it (a bad value is refused before anything is built)
    early          the sizes written into args for the early call: None = the map's (the matrix game's where no map says it), a
                   number = that number whatever the map
    mac, learner   class names, resolved in marl_amd.runner's namespace when a Runner is constructed
    on_policy      no replay buffer: one update on the episodes a rollout just generated, told the exploration rate they were drawn at.
                   With an agent switch the Runner raises ValueError, with overlapped rollouts NotImplementedError (an on-policy
                   update needs the weights the last one wrote)
    launcher_only  main.make_runner names the learner and the controller (Runner's learner_cls / mac_cls); a Runner built on the bare
                   name answers 'learner <name> cannot find!', as for a name no row knows
    no_switch      the ValueError text (% (name, switch)) with --RTW / --world_model / --MAIC; None: the name goes on to the switch rows
                   (runner._AGENT_SWITCHES), or is on_policy
    no_overlap     the NotImplementedError text with overlapped rollouts, or None
    at_launch      main.build gives the ``no_switch`` refusal itself, first thing"""
from collections import namedtuple

from .common.arguments import get_centralv_args, get_reinforce_args, get_coma_args, get_commnet_args, get_g2anet_args, \
    get_mappo_args, get_lica_args, get_maven_args

Row = namedtuple('Row', 'table keeps check early mac learner on_policy launcher_only no_switch no_overlap at_launch',
                 defaults=(None, (), None, {}, 'SharedMAC', None, False, False, None, None, False))

_MAP_SIZES = dict(n_agents=None, n_actions=None, state_shape=None)
_VALUE = Row(learner='QLearner')             # an agent switch puts its own learner in QLearner's place
_QTRAN = Row(learner='QTRANLearner')         # every agent switch refuses it (the switch rows)
_WQMIX = Row(check='common.arguments:get_wqmix_args', learner='WQMIXLearner',       # the table's alpha and central width; it is the
             no_switch="%s trains the plain shared agent beside a central one in WQMIXLearner: not with %s")   # check for its validator
UNKNOWN = Row()                              # builds, then 'learner <name> cannot find!'

ALGORITHMS = {
    'vdn': _VALUE, 'qmix': _VALUE, 'qplex': _VALUE,
    'qtran_base': _QTRAN, 'qtran_alt': _QTRAN,
    # independent Q-learning without a mixer.  With world_model the switch row refuses it as an unknown mixer; RTW and MAIC build
    # their controller and end in 'cannot find!'
    'iql': Row(learner='IQLLearner'),
    # QLearner with QattenMixer.  The check applies get_qatten_args first: its unit width needs the sizes.  The switches' learners keep
    # their own three-mixer tables
    'qatten': Row(check='main:_qatten', early=dict(n_agents=None, state_shape=None), learner='QLearner',
                  no_switch="%s mixes the plain shared agent's values in QLearner: not with %s"),
    # Weighted QMIX: an exact name, so the 'qmix' family below never sees it.  Rollouts act through the eval agent alone
    'ow_qmix': _WQMIX, 'cw_qmix': _WQMIX,
    # rollouts take the per-step path (the whole-rollout kernels have no MAVEN head) and draw one noise index per episode
    'maven': Row(table=get_maven_args, keeps=('noise_dim', 'lambda_mi'), check='network.maven:maven_shape_of', early=_MAP_SIZES,
                 mac='MAVENMAC', learner='MAVENLearner', at_launch=True,
                 no_switch="%s trains the noise-conditioned shared agent in MAVENLearner: not with %s",
                 no_overlap="overlapped rollouts use the whole-rollout kernel, which has no MAVEN head"),
    'central_v': Row(table=get_centralv_args, keeps=('td_lambda',), mac='PolicyMAC', learner='CentralVLearner', on_policy=True),
    'reinforce': Row(table=get_reinforce_args, mac='PolicyMAC', learner='ReinforceLearner', on_policy=True),
    'coma': Row(table=get_coma_args, keeps=('td_lambda',), mac='PolicyMAC', learner='COMALearner', on_policy=True, launcher_only=True),
    'mappo': Row(table=get_mappo_args, keeps=('td_lambda', 'ppo_clip', 'ppo_epochs', 'ppo_norm_adv'),
                 check='algorithm.ppo:ppo_settings_of', mac='PolicyMAC', learner='PPOLearner', on_policy=True, launcher_only=True),
    'lica': Row(table=get_lica_args, keeps=('td_lambda',), check='algorithm.lica:lica_shape_of', early=_MAP_SIZES,
                mac='PolicyMAC', learner='LICALearner', on_policy=True, launcher_only=True),
}

# The actor suffixes of the policy-gradient learners.  table: the argument table (commnet: k = 2 on map 3m, otherwise 3; g2anet:
# attention_dim = 32, hard = True); switch: the command-line override (argparse has typed it) of the table's ``sets``; check, early,
# mac: the row's - CommNet's range of k depends on no size, G2ANet's check takes the map's counts (a bad --g2anet_tau is refused all
# the same)
COMMNET = '+commnet'
G2ANET = '+g2anet'
_POLICY_ALGS = ('central_v', 'coma', 'reinforce')
_Actor = namedtuple('_Actor', 'name title table switch sets check early mac')
_ACTORS = {COMMNET: _Actor(name='commnet', title='CommNet', table=get_commnet_args, switch='commnet_k', sets='k',
                           check='controller.share_params:commnet_k_of', early=dict(n_agents=2, n_actions=1), mac='CommNetMAC'),
           G2ANET: _Actor(name='g2anet', title='G2ANet', table=get_g2anet_args, switch='g2anet_hard', sets='hard',
                          check='controller.share_params:g2anet_shape_of', early=dict(n_agents=None, n_actions=None), mac='G2ANetMAC')}


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


def _with_actor(base, actor):
    """the row of a policy-gradient algorithm with an actor suffix: the base's tables, then the actor's and its switch"""
    def table(args):
        base.table(args)
        actor.table(args)
        if getattr(args, actor.switch, None) is not None:
            setattr(args, actor.sets, getattr(args, actor.switch))
    return base._replace(table=table, check=actor.check, early=actor.early, mac=actor.mac, launcher_only=True)


def value_mixer(alg):
    return any(alg.find(a) > -1 for a in ('vdn', 'qmix', 'qplex'))


def qtran(alg):
    return alg.find('qtran_base') > -1 or alg.find('qtran_alt') > -1


def lookup(alg):
    """the row of a name: the exact name, a policy-gradient name with an actor suffix, then the two substring families ('qmix_x' is
    QLearner's; a refused suffix as in 'qmix+commnet' is main.build's to raise, through actor_base).  Never an error: UNKNOWN"""
    if alg in ALGORITHMS:
        return ALGORITHMS[alg]
    for suffix, actor in _ACTORS.items():
        if alg.endswith(suffix) and alg[:-len(suffix)] in _POLICY_ALGS:
            return _with_actor(ALGORITHMS[alg[:-len(suffix)]], actor)
    return _VALUE if value_mixer(alg) else _QTRAN if qtran(alg) else UNKNOWN
