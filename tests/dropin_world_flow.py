"""A caller written against the REFERENCE's module paths that builds the world-model pair the way its runner builds
QLearner (runner.py:4,10): arguments (+ get_mixer_args) -> StarCraft2Env -> env_info into args -> SharedMACWithState +
QLearnerWithState -> RolloutWorker episodes -> ReplayBuffer -> a few train() calls, then save_models / load_models.
Run through the launcher (`python -m marl_amd.dropin tests/dropin_world_flow.py`) every import must resolve to marl_amd."""
import math
import os
import shutil
import sys
import tempfile

import numpy as np

from smac.env import StarCraft2Env
from network.world_model import Agent
from controller.share_params import SharedMACWithState
from algorithm.q_learner_state import QLearnerWithState
from common.arguments import get_common_args, get_mixer_args
from common.replaybuffer import ReplayBuffer
from rollout import RolloutWorker

if __name__ == '__main__':
    tmp = tempfile.mkdtemp()
    sys.argv = [sys.argv[0], "--alg", "qmix", "--map", "2s3z", "--model_dir", os.path.join(tmp, "model")]
    args = get_common_args()
    get_mixer_args(args)
    env = StarCraft2Env(map_name=args.map)
    env_info = env.get_env_info()
    args.n_actions, args.n_agents = env_info["n_actions"], env_info["n_agents"]
    args.state_shape, args.obs_shape, args.episode_limit = env_info["state_shape"], env_info["obs_shape"], env_info["episode_limit"]
    args.batch_size = env.n_envs
    args.buffer_size = 4 * env.n_envs
    np.random.seed(3)
    mac = SharedMACWithState(args)
    learner = QLearnerWithState(mac, args)
    worker = RolloutWorker(env, mac, args)
    buf = ReplayBuffer(args)
    losses = []
    for i in range(3):
        episode = worker.generate_episodes(env.n_envs)[0]
        buf.store_episode(episode)
        losses.append(float(learner.train(buf.sample(args.batch_size), i)))
    learner.save_models(0)
    for kind in ("rnn_net", "mixer_net"):
        shutil.copyfile(learner.model_dir + "/0_%s_params.pkl" % kind, learner.model_dir + "/%s_params.pkl" % kind)
    learner.load_models()
    mods = {type(mac).__module__, type(learner).__module__, type(mac.agent).__module__, Agent.__module__}
    ok = all(m.startswith("marl_amd") for m in mods) and type(mac.agent) is Agent and all(math.isfinite(x) for x in losses)
    print("losses", losses)
    print("world drop-in ok" if ok else "world drop-in FAILED modules=%s losses=%s" % (sorted(mods), losses))
    shutil.rmtree(tmp, ignore_errors=True)
    sys.exit(0 if ok else 1)
