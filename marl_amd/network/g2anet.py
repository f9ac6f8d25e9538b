"""G2ANetAgent: the attention actor of coma+g2anet, central_v+g2anet and reinforce+g2anet (the reference ships only their argument
table, common/arguments.py:212-215: attention_dim = 32, hard = True; the definition is this project's own, taken from the published
implementation the table comes from - include/marl_hip.h).  H = rnn_hidden_dim = 64, D = attention_dim = 32,
tau = 0.01; 22 tensors under the published state-dict names, so a published rnn_net_params.pkl loads:

    encoding = Linear(I, 64)    h = GRUCell(64, 64)    hard_bi_GRU = GRU(128, 64, bidirectional=True)    hard_encoding = Linear(128, 2)
    q = Linear(64, 32, bias=False)    k = Linear(64, 32, bias=False)    v = Linear(64, 32)    decoding = Linear(96, A)

Per step t and environment, over the N agent rows (x_t = [obs | one-hot(u_{t-1}) | agent id], as RNNQNet's input):

    h_t        = h(relu(encoding(x_t)), h_{t-1})                # the ONLY recurrence in time: RNNQNet's fc1 + rnn
    hard:        the partners of agent i are j_1 < .. < j_{N-1}, all j != i, x_{i,p} = [h_i | h_{j_p}]
    f_{i,p}    = GRU_fwd(x_{i,p}, f_{i,p-1}),  f_{i,0} = 0      b_{i,p} = GRU_rev(x_{i,p}, b_{i,p+1}),  b_{i,N} = 0
    y_{i,p}    = hard_encoding([f_{i,p} | b_{i,p}])
    w_{i,p}    = softmax((y + gumbel) / tau)[1] = sigmoid((y_1 - y_0 + l_{i,p}) / tau),  l = g_1 - g_0 ~ Logistic(0, 1)
    soft:        a_{i,.} = softmax over p of q(h_i) . k(h_{j_p}) / sqrt(32),   x_i = sum_p a_{i,p} w_{i,p} relu(v(h_{j_p}))
    logits_i   = decoding([h_i | x_i])

Kept quirks: gumbel_softmax(tau=0.01) is called with hard=False and column 1 is taken, so w is a soft weight that is almost always
0 or 1 and its gradient goes through the sigmoid; noise is drawn in every pass, training and evaluation; there is no
renormalisation after w; dead agents and finished environments are not masked out of the partners; N = 1 has no partner and is
refused.  With args.hard false w = 1: the hard layers stay in the state dict and receive no gradient.

The members are parameter containers; ``forward`` is the plain-torch statement of one step (tests, CPU), the product path is
G2ANetMAC (controller/share_params.py): the agent unroll with fc1 = encoding, rnn = h and a zero fc2, then the head kernels
of csrc/g2anet.hip, which never build the (N-1) x 128 input of the bidirectional GRU.
"""
import math

import torch
import torch.nn as nn

from .. import ops
from ..hostutil import cached_module_struct

TAU = 0.01       # the published temperature of the hard attention

_HEAD = ("hard_bi_GRU.", "hard_encoding.", "q.", "k.", "v.", "decoding.")


def tau_of(args):
    """args.g2anet_tau (absent or None: the published 0.01); anything that is not a positive number is an error"""
    tau = getattr(args, "g2anet_tau", None)
    tau = TAU if tau is None else float(tau)
    if not (tau > 0.0 and math.isfinite(tau)):
        raise ValueError("g2anet_tau must be a positive number, got %r" % (tau,))
    return tau


def partners(N, device=None):
    """(N, N-1) long: row i = the agents j != i in agent order"""
    idx = torch.arange(N, device=device)
    return torch.stack([torch.cat([idx[:i], idx[i + 1:]]) for i in range(N)])


class G2ANetAgent(nn.Module):
    def __init__(self, input_shape, args):
        super().__init__()
        if args.rnn_hidden_dim != 64:
            raise ValueError("the gfx950 agent kernel is specialised for rnn_hidden_dim = 64 (wave64)")
        if getattr(args, "attention_dim", 32) != 32:
            raise ValueError("the gfx950 G2ANet head is specialised for attention_dim = 32")
        if args.n_agents < 2:
            raise ValueError("G2ANet: an agent without a partner has nothing to attend to (n_agents = %d)" % args.n_agents)
        H, D = args.rnn_hidden_dim, 32
        self.args = args
        self.input_shape = input_shape
        self.encoding = nn.Linear(input_shape, H)
        self.h = nn.GRUCell(H, H)
        self.hard_bi_GRU = nn.GRU(2 * H, H, bidirectional=True)
        self.hard_encoding = nn.Linear(2 * H, 2)
        self.q = nn.Linear(H, D, bias=False)
        self.k = nn.Linear(H, D, bias=False)
        self.v = nn.Linear(H, D)
        self.decoding = nn.Linear(H + D, args.n_actions)
        # the unroll's dummy fc2 as constants (not parameters, not in the state dict): zeros whose output goes to scratch.  It has
        # n_actions rows, not CommNet's one: the unroll's action count is also the width of the one-hot block of its virtual input
        self.register_buffer("_dummy_w", torch.zeros(args.n_actions, H), persistent=False)
        self.register_buffer("_dummy_b", torch.zeros(args.n_actions), persistent=False)

    # ------------------------------------------------------------------ one step in plain torch (the published signature)
    def forward(self, obs, hidden_state, noise=None):
        """obs (rows, input_shape) already concatenated, rows = environments x n_agents in agent order; hidden (rows, H);
        noise (rows, N-1): the logistic draws l (None: fresh ones) -> (logits (rows, A), h_out (rows, H))"""
        N, H = self.args.n_agents, self.args.rnn_hidden_dim
        h_out = self.h(torch.relu(self.encoding(obs)), hidden_state.reshape(-1, H))
        hg = h_out.reshape(-1, N, H)
        G = hg.shape[0]
        part = partners(N, hg.device)
        if getattr(self.args, "hard", True):
            x = torch.cat([hg.unsqueeze(2).expand(-1, -1, N - 1, -1), hg[:, part]], dim=-1)       # (G, N, N-1, 2H)
            y, _ = self.hard_bi_GRU(x.permute(2, 0, 1, 3).reshape(N - 1, G * N, 2 * H))
            y = self.hard_encoding(y).permute(1, 0, 2)                # (G N, N-1, 2)
            if noise is None:
                u = torch.rand(G * N, N - 1, device=y.device, dtype=y.dtype).clamp(1e-7, 1.0 - 1e-7)
                noise = torch.log(u) - torch.log1p(-u)
            w = torch.sigmoid((y[..., 1] - y[..., 0] + noise.reshape(G * N, N - 1)) / tau_of(self.args)).reshape(G, N, N - 1)
        else:
            w = torch.ones(G, N, N - 1, device=hg.device, dtype=hg.dtype)
        qv, kv, vv = self.q(hg), self.k(hg), torch.relu(self.v(hg))
        a = torch.softmax((qv.unsqueeze(2) * kv[:, part]).sum(-1) / math.sqrt(qv.shape[-1]), dim=-1)
        x = ((a * w).unsqueeze(-1) * vv[:, part]).sum(2)
        return self.decoding(torch.cat([hg, x], dim=-1)).reshape(G * N, -1), h_out

    # ------------------------------------------------------------------ what the ops need
    def front_weights(self):
        """marl_agent_weights_t of the recurrence: fc1 = encoding, rnn = h, the zero dummy fc2"""
        return cached_module_struct(self, "front", lambda t: ops.agent_weights({
            "fc1.weight": t["encoding.weight"], "fc1.bias": t["encoding.bias"], "rnn.weight_ih": t["h.weight_ih"],
            "rnn.weight_hh": t["h.weight_hh"], "rnn.bias_ih": t["h.bias_ih"], "rnn.bias_hh": t["h.bias_hh"],
            "fc2.weight": t["_dummy_w"], "fc2.bias": t["_dummy_b"]}), buffers=True)

    def head_weights(self):
        """marl_g2anet_weights_t: the sixteen tensors behind the recurrence"""
        return cached_module_struct(self, "head", ops.g2anet_weights)

    def head_grads(self):
        """marl_g2anet_grads_t over the .grad views of the head's tensors"""
        return ops.g2anet_grads({k: p.grad for k, p in self.named_parameters() if k.startswith(_HEAD)})
