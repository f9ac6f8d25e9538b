"""RTWAgent mirror (reference network/RTW.py:6-203): the RNNQNet agent plus the teammate, world and reflection nets.

The module tree and state_dict keys are the reference's (teammate_net / world_net / w_v as Sequential(Linear, ReLU, Linear)),
so the shipped model/qmix/2s3z/*rnn_net_params.pkl files load strictly.  The agent part is the HIP unroll kernel
(csrc/agent.hip) as in RNNQNet; the reflection term is csrc/rtw_head.hip (act mode: test_mode=True; given mode:
target=False).  Training-time losses are the constant 0 the reference returns (RTW.py:147-150,167-171); its target pass
(target=True) fails with a TypeError there, and raises the same error here.
"""
import torch
import torch.nn as nn

from .. import ops
from ..hostutil import require_cuda
from ..hostutil import cached_module_struct
from .q_network import RNNQNet


class RTWAgent(RNNQNet):
    def __init__(self, input_shape, args):
        super().__init__(input_shape, args)
        H, N, A, O = args.rnn_hidden_dim, args.n_agents, args.n_actions, args.obs_shape
        hid, attn = getattr(args, "hidden_dim", 64), getattr(args, "attn_dim", 64)
        self.teammate_net = nn.Sequential(nn.Linear(H + N, hid), nn.ReLU(), nn.Linear(hid, A))
        self.world_net = nn.Sequential(nn.Linear(O + N * A, hid), nn.ReLU(), nn.Linear(hid, O))
        self.w_q = nn.Linear(O + O, attn)
        self.w_k = nn.Linear(A, attn)
        self.w_v = nn.Sequential(nn.Linear(H + A, attn), nn.ReLU(), nn.Linear(attn, A))
        if (hid, attn) != (64, 64):
            raise ValueError("the gfx950 RTW head is specialised for hidden_dim = attn_dim = 64")

    def not_self_model(self):
        return bool(getattr(self.args, "not_self_model", True))

    def rtw_weights(self):
        """marl_rtw_weights_t over the current parameter storage (rebuilt only when a parameter moved, as weights())."""
        return cached_module_struct(self, "rtw", ops.rtw_weights)

    def forward(self, inputs, hidden_state, obs, obs_next, u, avail_u, target=False, test_mode=False, agent_num=0):
        """reference RTW.py:59-203: (q, h) with test_mode, else (q, h, loss_t, loss_w) with both losses 0."""
        a = self.args
        N, A, O = a.n_agents, a.n_actions, a.obs_shape
        if not test_mode and (target or obs_next is None or u is None):
            # RTW.py:178 concatenates obs with obs_next = None on the target pass (RTWMAC.get_next_q_values)
            raise TypeError("expected Tensor as element 1 in argument 0, but got NoneType")
        dev = require_cuda("RTWAgent.forward")
        q, h = RNNQNet.forward(self, inputs, hidden_state)
        w = self.rtw_weights()
        obs = obs.to(device=dev, dtype=torch.float32).reshape(-1, O)
        if test_mode:
            # one row (agent agent_num of one environment): run it as row agent_num of a one-environment tile
            hh = torch.zeros(N, a.rnn_hidden_dim, device=dev)
            oo = torch.zeros(N, O, device=dev)
            hh[agent_num], oo[agent_num] = h[0], obs[0]
            qq = torch.zeros(N, A, device=dev)
            qq[agent_num] = q[0]
            av = avail_u.to(device=dev, dtype=torch.float32).reshape(N, A).contiguous()
            ops.rtw_head_act(w, hh, oo, N, 0, av, N, 0, qq, 1, N, O, A, self.not_self_model())
            return qq[agent_num:agent_num + 1], h
        rows = q.shape[0]
        B = rows // N
        on = obs_next.to(device=dev, dtype=torch.float32).reshape(-1, O).contiguous()
        uu = u.to(device=dev).reshape(-1).to(torch.int32).contiguous()
        ops.rtw_head_given(w, h, obs.contiguous(), N, 0, on, N, 0, uu, N, 0, q, B, 1, N, O, A, self.not_self_model())
        return q, h, 0, 0
