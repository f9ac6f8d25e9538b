"""A caller written against the REFERENCE's module paths, following the steps of its matrix_game_test.py (arguments ->
alg qtran_base -> TwoAgentsMatrixGame with the first payoff table -> env_info into args -> SharedMAC -> RolloutWorker ->
QTRANLearner -> train on env.get_episodes() -> Q tables) with a short horizon.  Run through the launcher
(`python -m marl_amd.dropin tests/dropin_matrix_game_flow.py`) every import must resolve to marl_amd; without a GPU the
run stops at the learner's constructor ("no CPU fallback") - tests/test_host_logic.py::
test_reference_matrix_game_script_runs_on_dropin checks exactly that."""
import sys

from rollout import RolloutWorker
from controller.share_params import SharedMAC
from algorithm.q_learner import QLearner
from algorithm.qtran_learner import QTRANLearner
from common.arguments import get_common_args, get_mixer_args
from env.single_state_matrix_game import TwoAgentsMatrixGame

if __name__ == '__main__':
    args = get_common_args()
    get_mixer_args(args)
    args.alg, args.lr, args.cuda = 'qtran_base', 0.001, True
    env = TwoAgentsMatrixGame(payoff_table=[[8, -12, -12], [-12, 0, 0], [-12, 0, 0]])
    env_info = env.get_env_info()
    args.n_actions, args.n_agents = env_info["n_actions"], env_info["n_agents"]
    args.state_shape, args.obs_shape, args.episode_limit = env_info["state_shape"], env_info["obs_shape"], env_info["episode_limit"]
    mac = SharedMAC(args)
    worker = RolloutWorker(env, mac, args)
    learner = QTRANLearner(mac, args) if args.alg == 'qtran_base' else QLearner(mac, args)
    loss = None
    for train_step in range(200):
        loss = learner.train(env.get_episodes(), train_step)
    q_tot, q_i, q_j = learner.get_q_and_q_tot_table()
    mods = {type(worker).__module__, type(learner).__module__, type(mac).__module__, type(env).__module__}
    print("MATRIX_FLOW_OK loss=%.5f greedy=%s modules=%s" % (float(loss), divmod(int(q_tot.argmax()), q_tot.shape[1]), sorted(mods)))
    sys.exit(0 if all(m.startswith("marl_amd") for m in mods) else 1)
