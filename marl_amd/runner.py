"""Runner (mirror of reference runner.py:14-141): wires MAC + RolloutWorker + ReplayBuffer + learner
and reproduces the train / evaluate cadence, the logging tags and the save cycle.  With a batched env
every iteration collects ``env.n_envs`` episodes in lock-step and trains on ``batch_size`` sampled
episodes; with a serial env it behaves exactly like the reference loop.

``args.overlap_rollout`` (opt-in, batched envs): the rollout of iteration k+1 runs on a side HIP stream while the
learner trains on iteration k's sample.  The rollout reads a SNAPSHOT of the agent taken before update k (policy lag
of one update - the reference has lag 0, which is why this is off by default), writes into ring slots the sampler
excludes, and the cadence of runner.py:85-98 (store -> train_steps updates -> log -> save) is unchanged.
``"lag1_serial"`` runs the same schedule on one stream (the parity check of the overlapped mode: identical losses).

``args.RTW`` (with reuse_network, reference runner.py:20-23,46-49): RTWMAC and RTWQLearner.  Evaluation and rollouts run
(the per-step path; no overlapped rollouts); training raises the reference's TypeError.  Divergence: the reference pairs
RTWMAC with the plain QTRANLearner for qtran_base / qtran_alt, which cannot run on an RTW controller; here that
combination raises NotImplementedError.

``args.world_model`` (a switch of this project; the reference runner never builds the pair): SharedMACWithState and
QLearnerWithState (reference controller/share_params.py:185-387, algorithm/q_learner_state.py) for vdn / qmix / qplex.
Rollouts take the per-step path.  With RTW it raises ValueError, with qtran_* the reference's ValueError, with overlapped
rollouts NotImplementedError.

``args.MAIC`` (a switch of this project; the reference ships network/MAIC.py without a controller or a learner): MAICMAC and
MAICQLearner for vdn / qmix / qplex.  Evaluation and rollouts run (the per-step path); ``learner.train`` raises
NotImplementedError and touches nothing.  With RTW or world_model it raises ValueError, with qtran_* or overlapped rollouts
NotImplementedError - all before anything is built.

``args.MAIC_train`` (with MAIC): the learner is MAICTDLearner, which trains the agent on the TD loss through the message
head's backward pass and, with ``args.mi_loss_weight`` / ``args.entropy_loss_weight`` positive, on the agent's MI and
attention-entropy losses (csrc/maic_aux.hip); the refusals above hold for it too.  Without MAIC it raises ValueError before
anything is built, and so does a positive loss weight without MAIC_train.

``args.alg == 'central_v'`` / ``'reinforce'``: PolicyMAC and CentralVLearner (algorithm/central_v.py) or ReinforceLearner
(algorithm/reinforce.py), trained ON-POLICY: the episodes a rollout just
generated are the batch of the one update that follows it - nothing goes through the replay buffer - and the learner is told the
exploration rate they were drawn at.  With RTW / world_model / MAIC it raises ValueError, with overlapped rollouts
NotImplementedError (an on-policy update needs the weights the last one wrote) - before anything is built.
``learner_cls`` (a constructor argument): a further on-policy learner over PolicyMAC, named by the caller instead of by the runner's
own table; everything above holds for it.  The launcher passes COMALearner (algorithm/coma.py) for ``--alg coma``
(``main.make_runner``); a Runner built without it keeps answering 'learner coma cannot find!', as it always has.  ``--alg lica``
gets LICALearner (algorithm/lica.py) the same way: PolicyMAC, on-policy batches, and a Runner on the bare name answers
'learner lica cannot find!'.
``mac_cls`` (a constructor argument, with ``learner_cls``): the stochastic controller that learner trains in the place of PolicyMAC - the
launcher passes the GroupHeadMAC subclass of its actor table (CommNetMAC for the three ``+commnet`` algorithms, G2ANetMAC for the three
``+g2anet`` ones); a Runner built on a bare ``+commnet`` / ``+g2anet`` name answers 'cannot find!' too.

``args.alg == 'iql'`` (no agent switch on): SharedMAC, the replay buffer and IQLLearner (algorithm/iql.py), independent Q-learning
without a mixer.  With an agent switch the name is answered as before: world_model refuses it as an unknown mixer, RTW and MAIC
end in 'learner iql cannot find!'.

``args.alg == 'qatten'`` (no agent switch on): SharedMAC, the replay buffer and QLearner with QattenMixer (network/mixer.py).  With
RTW, world_model or MAIC it raises ValueError before anything is built: their learners keep their own three-mixer tables.

``args.alg == 'ow_qmix'`` / ``'cw_qmix'`` (no agent switch on): SharedMAC, the replay buffer and WQMIXLearner (algorithm/wqmix.py),
Weighted QMIX.  The names are decided before the value-mixer branch, whose substring match would take them for qmix.  With RTW,
world_model or MAIC it raises ValueError before anything is built.  Rollouts act through the eval agent alone.

``args.alg == 'maven'`` (no agent switch on): MAVENMAC, the replay buffer and MAVENLearner (algorithm/maven.py).  Rollouts take the
per-step path (the whole-rollout kernels have no MAVEN head) and draw one noise index per episode, which the records and the replay ring
carry.  With RTW, world_model or MAIC it raises ValueError, with overlapped rollouts NotImplementedError - before anything is built.

Full resume: ``save_resume`` / ``load_resume`` carry what the reference's checkpoints lack - optimizer
state, target networks, epsilon, the loop counters, the numpy RNG state (the replay ring refills)."""
from __future__ import annotations

import collections
import copy
import os

import numpy as np
import torch

from .rollout import RolloutWorker
from .controller.share_params import SharedMAC, SharedMACWithState, RTWMAC, MAICMAC, PolicyMAC, MAVENMAC
from .common.replaybuffer import ReplayBuffer
from .algorithm.q_learner import QLearner
from .algorithm.qtran_learner import QTRANLearner
from .algorithm.rtw_q_learner import RTWQLearner
from .algorithm.q_learner_state import QLearnerWithState
from .algorithm.maic_q_learner import MAICQLearner
from .algorithm.maic_td_learner import MAICTDLearner
from .algorithm.central_v import CentralVLearner
from .algorithm.reinforce import ReinforceLearner
from .algorithm.iql import IQLLearner
from .algorithm.wqmix import WQMIXLearner, WQMIX_ALGS
from .algorithm.maven import MAVENLearner
from .utils.logging import Logger


def _qtran(args):
    return args.alg.find('qtran_base') > -1 or args.alg.find('qtran_alt') > -1


def _value_mixer(args):
    return any(args.alg.find(a) > -1 for a in ('vdn', 'qmix', 'qplex'))


# One row per agent switch: the controller, the learner, and its refusals as (exception type, text) - combined with a
# switch of an earlier row, with a learner it cannot drive, with overlapped rollouts.  The rows and a row's checks run in
# this order, before anything is built; the types differ per row on purpose (module docstring).
_Switch = collections.namedtuple("_Switch", "name mac learner combined alg_refused alg overlap")
_AGENT_SWITCHES = (
    _Switch("RTW", RTWMAC, lambda mac, logger, args: RTWQLearner(mac, logger, args),
            None,
            _qtran, (NotImplementedError, "RTW with a QTRAN learner is not supported (the reference's QTRANLearner cannot "
                                          "drive an RTW controller)"),
            (NotImplementedError, "overlapped rollouts use the whole-rollout kernel, which has no RTW head")),
    _Switch("world_model", SharedMACWithState, lambda mac, logger, args: QLearnerWithState(mac, args),
            (ValueError, "world_model and RTW are two different agents: choose one"),
            lambda args: not _value_mixer(args), (ValueError, "Mixer {} not recognised."),     # q_learner_state.py:32
            (NotImplementedError, "overlapped rollouts use the whole-rollout kernel, which has no world-model head")),
    _Switch("MAIC", MAICMAC,
            lambda mac, logger, args: (MAICTDLearner if getattr(args, "MAIC_train", False) else MAICQLearner)(mac, args),
            (ValueError, "MAIC, RTW and world_model are three different agents: choose one"),
            _qtran, (NotImplementedError, "MAIC with a QTRAN learner is not supported"),
            (NotImplementedError, "overlapped rollouts use the whole-rollout kernel, which has no MAIC head")),
)


_ON_POLICY = {'central_v': CentralVLearner, 'reinforce': ReinforceLearner}      # policy-gradient learners over PolicyMAC


class Runner:
    def __init__(self, env, logger, args, learner_cls=None, mac_cls=None):
        self.env = env
        policy_mac_cls = mac_cls if mac_cls is not None else PolicyMAC
        if not args.reuse_network:
            raise NotImplementedError("only the shared-parameter controller (reuse_network) is on the hot path")
        if getattr(args, "MAIC_train", False) and not getattr(args, "MAIC", False):
            raise ValueError("MAIC_train trains the MAIC agent: it needs MAIC as well")
        if (getattr(args, "mi_loss_weight", 0) > 0 or getattr(args, "entropy_loss_weight", 0) > 0) \
                and not getattr(args, "MAIC_train", False):
            raise ValueError("mi_loss_weight / entropy_loss_weight are terms of MAICTDLearner's loss: they need MAIC_train")
        mac_cls, make_learner = SharedMAC, lambda mac, logger, args: QLearner(mac, args)
        on = [sw for sw in _AGENT_SWITCHES if getattr(args, sw.name, False)]
        if args.alg == 'qatten' and on:      # their learners keep their own three-mixer tables
            raise ValueError("qatten mixes the plain shared agent's values in QLearner: not with %s" % on[0].name)
        wqmix = args.alg in WQMIX_ALGS       # decided before _value_mixer, whose substring match would take the names for qmix
        if wqmix and on:
            raise ValueError("%s trains the plain shared agent beside a central one in WQMIXLearner: not with %s"
                             % (args.alg, on[0].name))
        maven = args.alg == 'maven'
        if maven and on:
            raise ValueError("maven trains the noise-conditioned shared agent in MAVENLearner: not with %s" % on[0].name)
        if maven and getattr(args, "overlap_rollout", False):
            raise NotImplementedError("overlapped rollouts use the whole-rollout kernel, which has no MAVEN head")
        if maven:
            mac_cls = MAVENMAC
        self.on_policy = learner_cls is not None or args.alg in _ON_POLICY
        if self.on_policy:
            if on:
                raise ValueError("%s trains the plain shared agent as a policy: not with %s" % (args.alg, on[0].name))
            if getattr(args, "overlap_rollout", False):
                raise NotImplementedError("%s is on-policy: a rollout needs the weights the last update wrote" % args.alg)
            mac_cls = policy_mac_cls
        for sw in on:
            for hit, refusal in ((sw is not on[0], sw.combined), (sw.alg_refused(args), sw.alg),
                                 (getattr(args, "overlap_rollout", False), sw.overlap)):
                if hit:
                    raise refusal[0](refusal[1].format(args.alg))
            mac_cls, make_learner = sw.mac, sw.learner
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
        if self.args.env in ('smac', 'synthetic', 'matrix', 'battle'):
            self.save_path = self.args.result_dir + '/' + args.alg + '/' + args.map
        else:
            raise ValueError("env {} dose not exist!".format(self.args.env))
        os.makedirs(self.save_path, exist_ok=True)
        logger.setup_tb(self.save_path + '/tb/other')
        self.logger = logger
        if self.on_policy:
            self.learner = (learner_cls or _ON_POLICY[args.alg])(self.mac, args)
        elif wqmix:
            self.learner = WQMIXLearner(self.mac, args)
        elif maven:
            self.learner = MAVENLearner(self.mac, args)
        elif _value_mixer(args):
            self.learner = make_learner(self.mac, logger, args)
        elif _qtran(args):
            self.learner = QTRANLearner(self.mac, args)
        elif args.alg == 'qatten':
            self.learner = QLearner(self.mac, args)
        elif args.alg == 'iql' and not on:
            self.learner = IQLLearner(self.mac, args)
        else:
            raise ValueError('learner {} cannot find!'.format(args.alg))
        if args.load_model:
            self.learner.load_models()
        self.time_steps, self.train_steps, self.evaluate_steps = 0, 0, -1     # loop counters (restored by load_resume)
        self.losses = []
        self.overlap = getattr(args, "overlap_rollout", False)
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
