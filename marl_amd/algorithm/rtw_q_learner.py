"""RTWQLearner (mirror of reference algorithm/RTW_q_learner.py:9-214).

Construction, the target copies, the optimizer and the model files (``<n>_rnn_net_params.pkl`` /
``<n>_mixer_net_params.pkl``, :198-214) are QLearner's.  ``train`` is not: in the reference it always fails with a
TypeError before any parameter changes (RTWMAC.get_next_q_values feeds obs_next = None into RTWAgent.forward,
network/RTW.py:178), so this learner raises the same error and leaves the parameters, the optimizer state and the
target networks untouched.  RTW training is outside the project."""
from __future__ import annotations

from .q_learner import QLearner


class RTWQLearner(QLearner):
    def __init__(self, mac, logger, args):
        self.logger = logger
        super().__init__(mac, args)

    def train(self, batch, train_step):
        raise TypeError("RTWQLearner.train: the reference's target pass concatenates obs with obs_next = None "
                        "(network/RTW.py:178); RTW training is not defined")
