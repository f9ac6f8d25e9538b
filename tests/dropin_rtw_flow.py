"""A caller written against the REFERENCE's module paths, following its main.py with RTW on and --evaluate: arguments
(+ get_mixer_args / get_RTW_args) -> StarCraft2Env -> env_info into args -> Runner (RTWMAC + RTWQLearner, load_model) ->
runner.evaluate().  The shipped QMIX RTW model (tests/golden/ref_ckpt/qmix_rtw) is copied into a temporary model_dir.
Run through the launcher (`python -m marl_amd.dropin tests/dropin_rtw_flow.py`) every import must resolve to marl_amd."""
import os
import shutil
import sys
import tempfile

from runner import Runner
from smac.env import StarCraft2Env
from network.RTW import RTWAgent
from controller.share_params import RTWMAC
from algorithm.RTW_q_learner import RTWQLearner
from common.arguments import get_common_args, get_mixer_args, get_RTW_args
from utils.logging import Logger

HERE = os.path.dirname(os.path.abspath(__file__))

if __name__ == '__main__':
    tmp = tempfile.mkdtemp()
    shutil.copytree(os.path.join(HERE, "golden", "ref_ckpt", "qmix_rtw"), os.path.join(tmp, "model", "qmix", "2s3z"))
    sys.argv = [sys.argv[0], "--alg", "qmix", "--map", "2s3z", "--RTW", "True", "--load_model", "True", "--evaluate", "True",
                "--evaluate_epoch", "4", "--model_dir", os.path.join(tmp, "model"), "--result_dir", os.path.join(tmp, "result")]
    args = get_common_args()
    get_mixer_args(args)
    get_RTW_args(args)
    env = StarCraft2Env(map_name=args.map)
    env_info = env.get_env_info()
    args.n_actions, args.n_agents = env_info["n_actions"], env_info["n_agents"]
    args.state_shape, args.obs_shape, args.episode_limit = env_info["state_shape"], env_info["obs_shape"], env_info["episode_limit"]
    runner = Runner(env, Logger(), args)
    win_rate, _ = runner.evaluate()
    mods = {type(runner.mac).__module__, type(runner.learner).__module__, type(runner.mac.agent).__module__,
            RTWAgent.__module__, RTWMAC.__module__, RTWQLearner.__module__, Runner.__module__}
    ok = (all(m.startswith("marl_amd") for m in mods) and type(runner.mac) is RTWMAC and type(runner.learner) is RTWQLearner
          and type(runner.mac.agent) is RTWAgent)
    print("The win rate of {} is  {}".format(args.alg, win_rate))
    print("RTW drop-in ok" if ok else "RTW drop-in FAILED modules=%s" % sorted(mods))
    shutil.rmtree(tmp, ignore_errors=True)
    sys.exit(0 if ok else 1)
