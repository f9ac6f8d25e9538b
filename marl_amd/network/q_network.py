"""RNNQNet mirror (reference network/q_network.py:6-21): fc1 -> ReLU -> GRUCell -> fc2.

The nn.Linear / nn.GRUCell members are parameter containers only (state_dict keys fc1.*, rnn.*,
fc2.* as in the reference); the arithmetic is the persistent HIP unroll kernel
(marl_amd/csrc/agent.hip) called with T = 1.
"""
import weakref

import torch
import torch.nn as nn

from .. import ops
from ..hostutil import require_cuda


# module -> {struct name: (parameters and buffers, their data pointers, the ctypes struct)}: a struct is rebuilt only when
# a tensor's storage moved (flat-buffer adoption, .to(), load_state_dict into new storage) - walking named_parameters()
# on every launch cost ~15 us, five times per update
_STRUCTS = weakref.WeakKeyDictionary()


def cached_struct(module, name, build, buffers=False):
    """``build(dict name -> tensor)`` over the module's current parameter storage (with ``buffers``: and its buffers).
    On a miss the module is moved to the device and its parameters are made contiguous first."""
    c = _STRUCTS.get(module, {}).get(name)
    if c is not None:
        tlist, ptrs, w = c
        if all(q.data_ptr() == o and q.is_cuda for q, o in zip(tlist, ptrs)):
            return w
    if next(module.parameters()).device.type != "cuda":
        module.to(require_cuda("RNNQNet"))
    tracked = dict(module.named_parameters())      # the Parameter objects: `p.data = ...` (flat-buffer adoption) shows in them
    for v in tracked.values():
        if not v.data.is_contiguous():
            v.data = v.data.contiguous()
    tensors = {k: v.data for k, v in tracked.items()}
    if buffers:
        tracked.update(module.named_buffers())
        tensors.update(module.named_buffers())
    w = build(tensors)
    tlist = list(tracked.values())
    _STRUCTS.setdefault(module, {})[name] = (tlist, [q.data_ptr() for q in tlist], w)
    return w


class RNNQNet(nn.Module):
    def __init__(self, input_shape, args):
        super().__init__()
        self.args = args
        self.input_shape = input_shape
        self.fc1 = nn.Linear(input_shape, args.rnn_hidden_dim)
        self.rnn = nn.GRUCell(args.rnn_hidden_dim, args.rnn_hidden_dim)
        self.fc2 = nn.Linear(args.rnn_hidden_dim, args.n_actions)
        if args.rnn_hidden_dim != 64:
            raise ValueError("the gfx950 agent kernel is specialised for rnn_hidden_dim = 64 (wave64)")

    def weights(self):
        """marl_agent_weights_t over the current parameter storage."""
        return cached_struct(self, "agent", ops.agent_weights)

    def forward(self, obs, hidden_state):
        """obs (rows, input_shape) already concatenated; hidden (rows, H) -> (q, h)."""
        dev = require_cuda("RNNQNet.forward")
        w = self.weights()
        x = obs.to(device=dev, dtype=torch.float32).contiguous()
        rows = x.shape[0]
        h_in = hidden_state.reshape(-1, self.args.rnn_hidden_dim).to(device=dev, dtype=torch.float32).contiguous()
        q = torch.empty(rows, self.args.n_actions, device=dev)
        h = torch.empty(rows, self.args.rnn_hidden_dim, device=dev)
        # rows act as "episodes" with one agent; the whole vector is the observation segment
        ops.agent_unroll_fwd(w, x, 1, 0, None, 0, 0, h_in, q, None, h, None, rows, 1, 1, self.input_shape,
                             self.args.n_actions, last_action=False, reuse_network=False)
        return q, h
