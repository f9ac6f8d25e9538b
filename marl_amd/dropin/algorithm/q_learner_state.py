"""`from algorithm.q_learner_state import QLearnerWithState` (reference runner.py:10) resolves to the product class."""
from marl_amd.algorithm.q_learner_state import QLearnerWithState  # noqa: F401
