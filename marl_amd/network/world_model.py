"""World-model agent (mirror of reference network/world_model.py:7-75): the RNNQNet agent plus a WorldModel head.

The module tree and state_dict keys are the reference's (fc1 / rnn / fc2, then world.hidden_embd.{0,2}, world.r_out,
world.o_out, world.terminate_out), so reference state dicts load strictly and the parameter order - the layout of the
learner's flat buffer - is the reference's ``list(mac.parameters())``.  The agent part is the HIP unroll kernel
(csrc/agent.hip) as in RNNQNet; the head is csrc/world_head.hip: q = fc2(h) + r (world_model.py:71).
"""
import torch
import torch.nn as nn

from .. import ops
from ..hostutil import require_cuda
from ..hostutil import cached_module_struct
from .q_network import RNNQNet


class WorldModel(nn.Module):
    """reference world_model.py:7-41 (parameter container; the arithmetic is csrc/world_head.hip)"""

    def __init__(self, args):
        super().__init__()
        self.args = args
        H = args.rnn_hidden_dim
        self.hidden_embd = nn.Sequential(nn.Linear(H, H), nn.ReLU(), nn.Linear(H, H))
        self.r_out = nn.Linear(H, args.n_actions)
        self.o_out = nn.Linear(H, args.obs_shape)
        self.terminate_out = nn.Linear(H, 2)


class Agent(RNNQNet):
    def __init__(self, input_shape, args):
        super().__init__(input_shape, args)
        self.world = WorldModel(args)
        if not ops.world_supported(args.n_agents, args.obs_shape, args.n_actions, args.rnn_hidden_dim):
            raise ValueError("the gfx950 world-model head covers N <= 16, O <= 256, A <= 32 (n_agents %d, obs_shape %d, "
                             "n_actions %d)" % (args.n_agents, args.obs_shape, args.n_actions))

    def world_weights(self):
        """marl_world_weights_t over the current parameter storage (rebuilt only when a parameter moved, as weights())."""
        return cached_module_struct(self, "world", ops.world_weights)

    def world_grads(self):
        """marl_world_grads_t over the parameters' .grad views (the learner's flat gradient buffer)."""
        return ops.world_grads({k: v.grad for k, v in self.named_parameters() if k.startswith("world.")})

    def forward(self, obs, hidden_state):
        """reference world_model.py:59-75: (q with r added, returns{hidden_state, r, o_next, terminated})."""
        a = self.args
        dev = require_cuda("world_model.Agent.forward")
        q, h = RNNQNet.forward(self, obs, hidden_state)
        rows = q.shape[0]
        r = torch.empty(rows, a.n_actions, device=dev)
        ohat = torch.empty(rows, a.obs_shape, device=dev)
        tau = torch.empty(rows, 2, device=dev)
        ops.world_head_fwd(self.world_weights(), h, q, rows, 1, 1, a.obs_shape, a.n_actions, r_out=r, ohat_out=ohat,
                           tau_out=tau)
        return q, {"hidden_state": h, "r": r, "o_next": ohat, "terminated": tau}
