from marl_amd.network.rtw import RTWAgent  # noqa: F401
