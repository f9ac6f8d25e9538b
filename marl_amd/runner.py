"""Runner (mirror of reference runner.py:14-141): wires MAC + RolloutWorker + ReplayBuffer + learner
and reproduces the train / evaluate cadence, the logging tags and the save cycle.  With a batched env
every iteration collects ``env.n_envs`` episodes in lock-step and trains on ``batch_size`` sampled
episodes; with a serial env it behaves exactly like the reference loop.

``args.overlap_rollout`` (opt-in, batched envs): the rollout of iteration k+1 runs on a side HIP stream while the
learner trains on iteration k's sample.  The rollout reads a SNAPSHOT of the agent taken before update k (policy lag
of one update - the reference has lag 0, which is why this is off by default), writes into ring slots the sampler
excludes, and the cadence of runner.py:85-98 (store -> train_steps updates -> log -> save) is unchanged.
``"lag1_serial"`` runs the same schedule on one stream (the parity check of the overlapped mode: identical losses).

The controller, the learner and the refusals of ``args.alg`` are its row's in algorithms.py (``lookup``); ``args.RTW`` /
``args.world_model`` / ``args.MAIC`` put the controller and learner of their row of ``_AGENT_SWITCHES`` in their place, for vdn / qmix /
qplex (rollouts then take the per-step path).  ``args.MAIC_train`` (with MAIC): MAICTDLearner, which trains the MAIC agent on the TD
loss and, with ``args.mi_loss_weight`` / ``args.entropy_loss_weight`` positive, on its MI and attention-entropy losses.  Every refusal
comes before anything is built; a name without a learner ends in 'learner <name> cannot find!' after the controller, the worker
and the buffer exist.

``learner_cls`` (a constructor argument): an on-policy learner over PolicyMAC, named by the caller instead of by the row - what the
rows say of ``on_policy`` holds for it.  ``main.make_runner`` passes the learner of the ``launcher_only`` rows so; a Runner built
on such a bare name answers 'cannot find!'.  ``mac_cls`` (with ``learner_cls``): the stochastic controller that learner trains in
the place of PolicyMAC.

Full resume: ``save_resume`` / ``load_resume`` carry what the reference's checkpoints lack - optimizer
state, target networks, epsilon, the loop counters, the numpy RNG state (the replay ring refills)."""
from __future__ import annotations

import collections
import copy
import os

import numpy as np
import torch

from .rollout import RolloutWorker
from .algorithms import UNKNOWN, lookup, qtran, value_mixer
from .controller.share_params import SharedMAC, SharedMACWithState, RTWMAC, MAICMAC, PolicyMAC, MAVENMAC, CommNetMAC, G2ANetMAC  # noqa: F401
from .common.replaybuffer import ReplayBuffer
from .algorithm.q_learner import QLearner
from .algorithm.qtran_learner import QTRANLearner
from .algorithm.rtw_q_learner import RTWQLearner
from .algorithm.q_learner_state import QLearnerWithState
from .algorithm.maic_q_learner import MAICQLearner
from .algorithm.maic_td_learner import MAICTDLearner
from .algorithm.central_v import CentralVLearner  # noqa: F401  (the rows' classes: algorithms.py names them, __init__ finds them here)
from .algorithm.reinforce import ReinforceLearner  # noqa: F401
from .algorithm.coma import COMALearner  # noqa: F401
from .algorithm.ppo import PPOLearner  # noqa: F401
from .algorithm.lica import LICALearner  # noqa: F401
from .algorithm.iql import IQLLearner  # noqa: F401
from .algorithm.wqmix import WQMIXLearner  # noqa: F401
from .algorithm.maven import MAVENLearner  # noqa: F401
from .utils.logging import Logger


# One row per agent switch: the controller, the learner, and its refusals as (exception type, text) - combined with a
# switch of an earlier row, with a learner it cannot drive, with overlapped rollouts.  The rows and a row's checks run in
# this order, before anything is built.  The types differ per row on purpose: the reference pairs RTWMAC with the plain
# QTRANLearner, which cannot run (NotImplementedError here); world_model with qtran_* gives the reference's own ValueError
# (q_learner_state.py:32); the reference never builds the world-model or the MAIC pair, whose other refusals are this project's.
_Switch = collections.namedtuple("_Switch", "name mac learner combined alg_refused alg overlap")
_AGENT_SWITCHES = (
    _Switch("RTW", RTWMAC, lambda mac, logger, args: RTWQLearner(mac, logger, args),
            None,
            lambda args: qtran(args.alg), (NotImplementedError, "RTW with a QTRAN learner is not supported (the reference's "
                                                                "QTRANLearner cannot drive an RTW controller)"),
            (NotImplementedError, "overlapped rollouts use the whole-rollout kernel, which has no RTW head")),
    _Switch("world_model", SharedMACWithState, lambda mac, logger, args: QLearnerWithState(mac, args),
            (ValueError, "world_model and RTW are two different agents: choose one"),
            lambda args: not value_mixer(args.alg), (ValueError, "Mixer {} not recognised."),     # q_learner_state.py:32
            (NotImplementedError, "overlapped rollouts use the whole-rollout kernel, which has no world-model head")),
    _Switch("MAIC", MAICMAC,
            lambda mac, logger, args: (MAICTDLearner if getattr(args, "MAIC_train", False) else MAICQLearner)(mac, args),
            (ValueError, "MAIC, RTW and world_model are three different agents: choose one"),
            lambda args: qtran(args.alg), (NotImplementedError, "MAIC with a QTRAN learner is not supported"),
            (NotImplementedError, "overlapped rollouts use the whole-rollout kernel, which has no MAIC head")),
)


def switches_on(args):
    """the rows of _AGENT_SWITCHES whose switch is on, in table order"""
    return [sw for sw in _AGENT_SWITCHES if getattr(args, sw.name, False)]


class Runner:
    def __init__(self, env, logger, args, learner_cls=None, mac_cls=None):
        self.env = env
        # ---- the checks that hold for every algorithm
        if not args.reuse_network:
            raise NotImplementedError("only the shared-parameter controller (reuse_network) is on the hot path")
        if getattr(args, "MAIC_train", False) and not getattr(args, "MAIC", False):
            raise ValueError("MAIC_train trains the MAIC agent: it needs MAIC as well")
        if (getattr(args, "mi_loss_weight", 0) > 0 or getattr(args, "entropy_loss_weight", 0) > 0) \
                and not getattr(args, "MAIC_train", False):
            raise ValueError("mi_loss_weight / entropy_loss_weight are terms of MAICTDLearner's loss: they need MAIC_train")
        # ---- the row's refusals, then the switch rows'
        row = lookup(args.alg)
        if row.launcher_only and learner_cls is None:
            row = UNKNOWN
        on, overlap = switches_on(args), getattr(args, "overlap_rollout", False)
        if on and row.no_switch:
            raise ValueError(row.no_switch % (args.alg, on[0].name))
        if overlap and row.no_overlap:
            raise NotImplementedError(row.no_overlap)
        self.on_policy = learner_cls is not None or row.on_policy
        if self.on_policy:
            if on:
                raise ValueError("%s trains the plain shared agent as a policy: not with %s" % (args.alg, on[0].name))
            if overlap:
                raise NotImplementedError("%s is on-policy: a rollout needs the weights the last update wrote" % args.alg)
        for sw in on:
            for hit, refusal in ((sw is not on[0], sw.combined), (sw.alg_refused(args), sw.alg), (overlap, sw.overlap)):
                if hit:
                    raise refusal[0](refusal[1].format(args.alg))
        # ---- building: the classes are this module's attributes of the row's names, looked up now
        if on:                          # a switch's learner stands in for QLearner; it drives no other row's
            mac_cls, make_learner = on[0].mac, on[0].learner if row.learner == 'QLearner' else None
        else:                           # (mac_cls stands in for an on-policy learner's PolicyMAC alone)
            mac_cls = self.on_policy and mac_cls or globals()['PolicyMAC' if learner_cls else row.mac]
            learner_cls = learner_cls or row.learner and globals()[row.learner]
            make_learner = learner_cls and (lambda mac, logger, args: learner_cls(mac, args))
        if mac_cls is MAICMAC:
            from .common.arguments import get_maic_args
            get_maic_args(args)
        self.mac = mac_cls(args)
        self.rolloutWorker = RolloutWorker(env, self.mac, args)
        self.buffer = None if self.on_policy else ReplayBuffer(args)
        self.rolloutWorker.record_sink = self.buffer   # batched rollouts write into the replay ring in place
        self.args = args
        self.eval_win_rates = []
        self.eval_episode_rewards = []
        if self.args.env in ('smac', 'synthetic', 'matrix', 'battle', 'hunt'):
            self.save_path = self.args.result_dir + '/' + args.alg + '/' + args.map
        else:
            raise ValueError("env {} dose not exist!".format(self.args.env))
        os.makedirs(self.save_path, exist_ok=True)
        logger.setup_tb(self.save_path + '/tb/other')
        self.logger = logger
        if make_learner is None:
            raise ValueError('learner {} cannot find!'.format(args.alg))
        self.learner = make_learner(self.mac, logger, args)
        if args.load_model:
            self.learner.load_models()
        self.time_steps, self.train_steps, self.evaluate_steps = 0, 0, -1     # loop counters (restored by load_resume)
        self.losses = []
        self.overlap = overlap
        self._side = None
        self._mac_roll = None
        if getattr(args, "resume", ""):
            self.load_resume(args.resume)

    # ------------------------------------------------------------------ overlapped rollout
    def _launch_rollout(self):
        """snapshot the agent, then enqueue the next training rollout - on the side stream when overlapping"""
        from .hostutil import flatten_module
        if self._mac_roll is None:
            self._mac_roll = copy.deepcopy(self.mac)
            flatten_module(self._mac_roll.agent, self.learner.device)
            self._mac_roll._dev = self.learner.device
        cur = torch.cuda.current_stream()
        # the snapshot is taken ON THE MAIN STREAM: it is ordered after every update enqueued so far and before the
        # optimizer kernel of the next one (a copy on the side stream would only be ordered against the past)
        self._mac_roll.agent._flat.flat.copy_(self.mac.agent._flat.flat)
        if self.overlap is True:
            if self._side is None:
                self._side = torch.cuda.Stream(device=cur.device)
            self._side.wait_stream(cur)         # the rollout reads the snapshot (and the ring) as of this point
            ctx = torch.cuda.stream(self._side)
        else:
            ctx = torch.cuda.stream(cur)
        with ctx:
            pending = self.rolloutWorker.launch_episodes(mac=self._mac_roll)
        slot = getattr(pending[0], "sink_slot", None)
        return pending, (None if slot is None else (slot, pending[0].E))

    def _finish_rollout(self, pending):
        if self._side is not None:
            torch.cuda.current_stream().wait_stream(self._side)
        return self.rolloutWorker.finish_episodes(pending)

    def run(self, num):
        """reference runner.py:61-113."""
        a = self.args
        n_ep = getattr(self.env, "n_envs", a.n_episodes)
        loss = float("nan")
        pending, in_flight = None, None
        while self.time_steps < a.n_steps:
            if self.time_steps // a.evaluate_cycle > self.evaluate_steps:
                win_rate, episode_reward = self.evaluate()
                self.eval_win_rates.append(win_rate)
                self.eval_episode_rewards.append(episode_reward)
                self.plt(num)
                self.logger.log_stat("test_win_rate", win_rate, self.time_steps)
                self.logger.log_stat("test_episode_reward", episode_reward, self.time_steps)
                self.evaluate_steps += 1
            if self.overlap:
                if pending is None:
                    pending, _ = self._launch_rollout()          # first iteration: nothing to overlap with yet
                episodes, rewards, win_tags, steps = self._finish_rollout(pending)
            else:
                episodes, rewards, win_tags, steps = self.rolloutWorker.generate_episodes(n_episodes=n_ep, random_select=False)
            self.time_steps += steps
            self.logger.log_stat("episode_length", steps, self.time_steps)
            self.logger.log_stat("train_win_rate", sum(win_tags) / n_ep, self.time_steps)
            self.logger.log_stat("train_episode_reward", sum(rewards) / n_ep, self.time_steps)
            if self.on_policy:                                   # one update on the episodes just generated
                loss = self.learner.train(episodes, self.train_steps, epsilon=self.rolloutWorker.epsilon)
                self.losses.append(loss)
                self.train_steps += 1
            else:
                self.buffer.store_episode(episodes)
            if self.overlap:
                pending, in_flight = self._launch_rollout()      # rollout k+1 flies while update k trains below
            for _ in range(0 if self.on_policy else a.train_steps):
                mini_batch = self.buffer.sample(min(self.buffer.current_size, a.batch_size), exclude=in_flight)
                loss = self.learner.train(mini_batch, self.train_steps)
                self.losses.append(loss)
                self.train_steps += 1
            self.logger.log_stat("total_loss", loss, self.time_steps)
            if self.train_steps > 0 and self.train_steps % a.save_cycle == 0:
                self.learner.save_models(self.train_steps)
                if getattr(a, "save_resume", True):
                    self.save_resume(self.save_path + '/resume.pt')
        if pending is not None:
            self._finish_rollout(pending)                        # drain the rollout still in flight
        win_rate, episode_reward = self.evaluate()
        self.eval_win_rates.append(win_rate)
        self.eval_episode_rewards.append(episode_reward)
        self.plt(num)
        return loss

    # ------------------------------------------------------------------ full resume
    def save_resume(self, path):
        torch.save({"learner": self.learner.resume_state(), "epsilon": self.rolloutWorker.epsilon,
                    "time_steps": self.time_steps, "train_steps": self.train_steps, "evaluate_steps": self.evaluate_steps,
                    "eval_win_rates": list(self.eval_win_rates), "eval_episode_rewards": list(self.eval_episode_rewards),
                    "env_episode": getattr(self.env, "episode", None), "np_random": np.random.get_state(),
                    "ring_noise": self._ring_noise()}, path)

    def _ring_noise(self):
        """the replay ring's per-episode noise (MAVEN) as a host tensor, or None where the ring holds none"""
        rec = getattr(self.buffer, "record", None)
        return None if rec is None or rec.noise is None else rec.noise.detach().cpu().clone()

    def load_resume(self, path):
        sd = torch.load(path, map_location="cpu", weights_only=False)
        self.learner.load_resume_state(sd["learner"])
        self.rolloutWorker.epsilon = sd["epsilon"]
        self.time_steps, self.train_steps, self.evaluate_steps = sd["time_steps"], sd["train_steps"], sd["evaluate_steps"]
        self.eval_win_rates, self.eval_episode_rewards = list(sd["eval_win_rates"]), list(sd["eval_episode_rewards"])
        if sd.get("env_episode") is not None and hasattr(self.env, "episode"):
            self.env.episode = sd["env_episode"]
        np.random.set_state(sd["np_random"])
        noise, rec = sd.get("ring_noise"), getattr(self.buffer, "record", None)
        if noise is not None and rec is not None and rec.E == noise.numel():      # (a ring not allocated yet refills with its own)
            if rec.noise is None:
                rec.noise = torch.zeros(rec.E, dtype=torch.int32, device=rec.obs.device)
            rec.noise.copy_(noise)

    def evaluate(self):
        """reference runner.py:115-121."""
        if self.args.evaluate_epoch == 0:
            return 0, 0
        n = getattr(self.env, "n_envs", self.args.evaluate_epoch)
        _, episodes_reward, win_tags, _ = self.rolloutWorker.generate_episodes(n_episodes=n, evaluate=True)
        return sum(win_tags) / len(win_tags), sum(episodes_reward) / len(episodes_reward)

    def plt(self, num):
        """reference runner.py:123-141: the curves are saved as .npy (the PNG needs matplotlib, optional)."""
        np.save(self.save_path + '/win_rates_{}'.format(num), self.eval_win_rates)
        np.save(self.save_path + '/episode_rewards_{}'.format(num), self.eval_episode_rewards)
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
            plt.figure()
            plt.subplot(2, 1, 1); plt.plot(range(len(self.eval_win_rates)), self.eval_win_rates)
            plt.ylabel('win_rates')
            plt.subplot(2, 1, 2); plt.plot(range(len(self.eval_episode_rewards)), self.eval_episode_rewards)
            plt.xlabel('step*{}'.format(self.args.evaluate_cycle)); plt.ylabel('episode_rewards')
            plt.savefig(self.save_path + '/plt_{}.png'.format(num), format='png')
            plt.close()
        except Exception:
            pass
