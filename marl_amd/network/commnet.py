"""CommNetAgent: the communicating actor of coma+commnet, central_v+commnet and reinforce+commnet (the reference ships only their
argument table, common/arguments.py:23-25,203; the definition is this project's own, taken from the published implementation the
table comes from - include/marl_hip.h).  H = rnn_hidden_dim = 64, K = args.k rounds, state-dict names as
published, so a published rnn_net_params.pkl loads:

    encoding = Linear(I, H)    f_obs = GRUCell(H, H)    f_comm = GRUCell(H, H)    decoding = Linear(H, A)

Per step t and environment, over the N agent rows (x_t = [obs | one-hot(u_{t-1}) | agent id], as RNNQNet's input):

    e      = sigmoid(encoding(x_t))
    h_t    = f_obs(e, h_{t-1})                  # the ONLY recurrence in time; h_t is the carried hidden state
    g^(0)  = f_comm(0, h_t)                     # round 0: the input is zero, so its input side is b_ih alone
    g^(j)  = f_comm(c^(j), g^(j-1)),  c_i^(j) = (sum over l != i of g_l^(j-1)) / N        for j = 1 .. K-1
    logits = decoding(g^(K-1))

Kept quirks: the mean divides by N, not N - 1; round 0 still runs f_comm, so decoding never sees h_t directly (K = 1 included);
dead agents and finished environments are not masked out of the sum.

The members are parameter containers; ``forward`` is the plain-torch statement of one step (tests, CPU), the product path is
CommNetMAC (controller/share_params.py): ops.linear + the sigmoid kernel, the agent unroll over an identity front layer, and the
head kernels of csrc/commnet.hip.
"""
import torch
import torch.nn as nn

from .. import ops
from ..hostutil import cached_module_struct

FRONT_A = 1      # actions of the dummy fc2 the unroll kernels are fed: the smallest count they accept


class CommNetAgent(nn.Module):
    def __init__(self, input_shape, args):
        super().__init__()
        if args.rnn_hidden_dim != 64:
            raise ValueError("the gfx950 agent kernel is specialised for rnn_hidden_dim = 64 (wave64)")
        H = args.rnn_hidden_dim
        self.args = args
        self.input_shape = input_shape
        self.encoding = nn.Linear(input_shape, H)
        self.f_obs = nn.GRUCell(H, H)
        self.f_comm = nn.GRUCell(H, H)
        self.decoding = nn.Linear(H, args.n_actions)
        # the unroll's front layer as constants (not parameters, not in the state dict): fc1 = I with a zero bias, so that
        # relu(I e + 0) = e exactly for e = sigmoid(.) >= 0, and a zero fc2 whose output goes to scratch
        self.register_buffer("_front_w", torch.eye(H), persistent=False)
        self.register_buffer("_front_b", torch.zeros(H), persistent=False)
        self.register_buffer("_dummy_w", torch.zeros(FRONT_A, H), persistent=False)
        self.register_buffer("_dummy_b", torch.zeros(FRONT_A), persistent=False)

    # ------------------------------------------------------------------ one step in plain torch (the published signature)
    def forward(self, obs, hidden_state):
        """obs (rows, input_shape) already concatenated, rows = environments x n_agents in agent order; hidden (rows, H)
        -> (logits (rows, A), h_out (rows, H))"""
        N, H = self.args.n_agents, self.args.rnn_hidden_dim
        e = torch.sigmoid(self.encoding(obs))
        h_out = self.f_obs(e, hidden_state.reshape(-1, H))
        g = self.f_comm(torch.zeros_like(h_out), h_out)
        for _ in range(1, self.args.k):
            gg = g.reshape(-1, N, H)
            c = ((gg.sum(dim=1, keepdim=True) - gg) / N).reshape(-1, H)
            g = self.f_comm(c, g)
        return self.decoding(g), h_out

    # ------------------------------------------------------------------ what the ops need
    def front_weights(self):
        """marl_agent_weights_t of the recurrence: identity fc1, rnn = f_obs, the zero dummy fc2"""
        return cached_module_struct(self, "front", lambda t: ops.agent_weights({
            "fc1.weight": t["_front_w"], "fc1.bias": t["_front_b"], "rnn.weight_ih": t["f_obs.weight_ih"],
            "rnn.weight_hh": t["f_obs.weight_hh"], "rnn.bias_ih": t["f_obs.bias_ih"], "rnn.bias_hh": t["f_obs.bias_hh"],
            "fc2.weight": t["_dummy_w"], "fc2.bias": t["_dummy_b"]}), buffers=True)

    def head_weights(self):
        """marl_commnet_weights_t: f_comm and decoding"""
        return cached_module_struct(self, "head", ops.commnet_weights)

    def head_grads(self):
        """marl_commnet_grads_t over the .grad views of f_comm and decoding"""
        return ops.commnet_grads({k: p.grad for k, p in self.named_parameters() if k.startswith(("f_comm.", "decoding."))})
