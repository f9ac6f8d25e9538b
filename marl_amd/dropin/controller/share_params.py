from marl_amd.controller.share_params import SharedMAC, SeparatedMAC, SharedMACWithState, RTWMAC, MAICMAC  # noqa: F401
