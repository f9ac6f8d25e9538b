"""A caller written against the REFERENCE's module paths that evaluates the MAIC agent: arguments (+ get_mixer_args /
get_maic_args) -> StarCraft2Env -> env_info into args -> MAICMAC -> RolloutWorker evaluation episodes, then a save_models /
load_models round trip.  Run through the launcher (`python -m marl_amd.dropin tests/dropin_maic_flow.py`) every import must
resolve to marl_amd."""
import os
import shutil
import sys
import tempfile

import numpy as np

from smac.env import StarCraft2Env
from network.MAIC import MAICAgent
from controller.share_params import MAICMAC
from common.arguments import get_common_args, get_mixer_args, get_maic_args
from rollout import RolloutWorker

if __name__ == '__main__':
    tmp = tempfile.mkdtemp()
    sys.argv = [sys.argv[0], "--alg", "qmix", "--map", "2s3z", "--MAIC", "True", "--model_dir", os.path.join(tmp, "model")]
    args = get_common_args()
    get_mixer_args(args)
    get_maic_args(args)
    env = StarCraft2Env(map_name=args.map)
    env_info = env.get_env_info()
    args.n_actions, args.n_agents = env_info["n_actions"], env_info["n_agents"]
    args.state_shape, args.obs_shape, args.episode_limit = env_info["state_shape"], env_info["obs_shape"], env_info["episode_limit"]
    np.random.seed(3)
    mac = MAICMAC(args)
    mac.agent.eval()
    worker = RolloutWorker(env, mac, args)
    _, rewards, wins, steps = worker.generate_episodes(env.n_envs, evaluate=True)
    path = os.path.join(tmp, "rnn_net_params.pkl")
    mac.save_models(path)
    mac.load_models(path)
    mods = {type(mac).__module__, type(mac.agent).__module__, MAICAgent.__module__}
    ok = all(m.startswith("marl_amd") for m in mods) and type(mac.agent) is MAICAgent and steps > 0 and all(np.isfinite(rewards))
    print("win rate", sum(wins) / len(wins))
    print("MAIC drop-in ok" if ok else "MAIC drop-in FAILED modules=%s" % sorted(mods))
    shutil.rmtree(tmp, ignore_errors=True)
    sys.exit(0 if ok else 1)
