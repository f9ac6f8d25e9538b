"""MAICQLearner: the learner object a Runner with a MAICMAC holds.  The reference has no learner for its MAIC agent.

Construction, the target copies and the model files (``<n>_rnn_net_params.pkl`` / ``<n>_mixer_net_params.pkl``) are QLearner's,
so a saved model loads and evaluates.  ``train`` raises before anything is touched: parameters, optimizer state and target
networks stay as they are.  This is the learner of ``--MAIC True`` alone (inference and rollouts).  Training on the TD loss is
MAICTDLearner (``--MAIC_train True``, algorithm/maic_td_learner.py); the MI and entropy losses of network/MAIC.py:88-121 are not
built by either."""
from __future__ import annotations

from .q_learner import QLearner


class MAICQLearner(QLearner):
    def train(self, batch, train_step):
        raise NotImplementedError("MAIC training is not implemented (inference and rollouts only): the message head has no "
                                  "backward pass and the MI / entropy losses are not built")

    def get_q_and_q_tot_table(self):
        raise NotImplementedError("get_q_and_q_tot_table is not defined for the MAIC agent")
