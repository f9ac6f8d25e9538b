"""`from algorithm.RTW_q_learner import RTWQLearner` (reference runner.py:9) resolves to the product class."""
from marl_amd.algorithm.rtw_q_learner import RTWQLearner  # noqa: F401
