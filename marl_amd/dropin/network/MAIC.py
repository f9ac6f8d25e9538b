"""`from network.MAIC import MAICAgent` resolves to the product class."""
from marl_amd.network.maic import MAICAgent  # noqa: F401
