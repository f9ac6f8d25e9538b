"""MAICAgent mirror (reference network/MAIC.py:10-94): the RNNQNet agent plus the MAIC message head.  ``forward`` is the
reference's inference forward; ``head_backward`` is the head's backward pass for the TD loss (MAICTDLearner).

The module tree and state_dict keys are the reference's, in its order (embed_net.{0,1,3}, inference_net.{0,1,3}, fc1, rnn,
fc2, msg_net.{0,2}, w_key, w_query, the BatchNorm buffers included), so a reference-trained state dict loads strictly.
inference_net is held and saved but never evaluated: it only feeds the MI loss, which is not built (neither is the entropy
loss: ``forward`` refuses ``train_mode`` with a positive weight for either).  The agent part is the HIP unroll kernel
(csrc/agent.hip) as in RNNQNet; the head is csrc/maic_head.hip, its backward csrc/maic_head_bwd.hip.

BatchNorm follows the module's ``training`` flag as torch does: ``eval()`` normalises with the running statistics; in training
mode - the state of a freshly built module, and the reference never calls ``.eval()`` - with the statistics of all bs * N rows
of the call, and the running statistics move.  In that mode the rows of one call are coupled.
"""
import torch
import torch.nn as nn

from .. import ops
from ..hostutil import require_cuda
from .q_network import RNNQNet, cached_struct


class MAICAgent(RNNQNet):
    def __init__(self, input_shape, args):
        nn.Module.__init__(self)
        self.args = args
        self.input_shape = input_shape
        self.n_agents, self.latent_dim, self.n_actions = args.n_agents, args.latent_dim, args.n_actions
        H, NH, N, L, A = args.rnn_hidden_dim, args.nn_hidden_size, args.n_agents, args.latent_dim, args.n_actions
        act = nn.LeakyReLU()
        self.embed_net = nn.Sequential(nn.Linear(H, NH), nn.BatchNorm1d(NH), act, nn.Linear(NH, N * L * 2))
        self.inference_net = nn.Sequential(nn.Linear(H + A, NH), nn.BatchNorm1d(NH), act, nn.Linear(NH, L * 2))
        self.fc1 = nn.Linear(input_shape, H)
        self.rnn = nn.GRUCell(H, H)
        self.fc2 = nn.Linear(H, A)
        self.msg_net = nn.Sequential(nn.Linear(H + L, NH), act, nn.Linear(NH, A))
        self.w_key = nn.Linear(H, args.attention_dim)
        self.w_query = nn.Linear(L, args.attention_dim)
        if H != 64:
            raise ValueError("the gfx950 agent kernel is specialised for rnn_hidden_dim = 64 (wave64)")
        if not ops.maic_supported(N, args.obs_shape, A, H, NH, L, args.attention_dim):
            raise ValueError("the gfx950 MAIC head covers N <= 16, A <= 32, nn_hidden_size 64, latent_dim 8, attention_dim 32 "
                             "(n_agents %d, n_actions %d, nn_hidden_size %d, latent_dim %d, attention_dim %d)"
                             % (N, A, NH, L, args.attention_dim))

    def init_hidden(self):
        return self.fc1.weight.new(1, self.args.rnn_hidden_dim).zero_()

    def maic_weights(self):
        """marl_maic_weights_t over the current parameter and buffer storage (rebuilt only when one moved, as weights())."""
        return cached_struct(self, "maic", ops.maic_weights, buffers=True)

    def head(self, h, q, bs, test_mode, eps=None, **outs):
        """q (bs*N, A) += the gated messages from h (bs*N, 64), BatchNorm in this module's mode (csrc/maic_head.hip)"""
        a = self.args
        bn = self.embed_net[1]
        if not test_mode and eps is None:
            eps = torch.randn(bs * a.n_agents, a.n_agents * a.latent_dim, device=h.device)
        ops.maic_head_fwd(self.maic_weights(), h, q, bs, a.n_agents, a.n_actions, test_mode=test_mode, bn_batch=self.training,
                          eps=None if test_mode else eps, var_floor=a.var_floor, bn_eps=bn.eps,
                          bn_momentum=0.1 if bn.momentum is None else bn.momentum, **outs)

    def maic_grads(self):
        """marl_maic_grads_t over the head parameters' .grad views (the learner's flat gradient buffer); inference_net has no
        part in it."""
        return ops.maic_grads({k: v.grad for k, v in self.named_parameters() if not k.startswith("inference_net.")})

    def head_backward(self, h, u_act, dq_val, bs, test_mode, eps, dh):
        """Backward of ``head`` for the sparse gradient (u_act, dq_val) on the returned q, one pair per row: dh (bs*N, 64) =
        the head's contribution to the gradient on h (the identity path is BPTT's own), the head's weight gradients
        accumulate into the .grad views.  Same h, eps and modes as the forward call; the running statistics do not move
        (csrc/maic_head_bwd.hip)."""
        a = self.args
        ops.maic_head_bwd(self.maic_weights(), self.maic_grads(), h, u_act, dq_val, dh, bs, a.n_agents, a.n_actions,
                          test_mode=test_mode, bn_batch=self.training, eps=None if test_mode else eps, var_floor=a.var_floor,
                          bn_eps=self.embed_net[1].eps)

    def forward(self, inputs, hidden_state, bs, test_mode=False, **kwargs):
        """reference MAIC.py:52-94: (return_q, h, returns) with returns = {}.  ``eps`` (keyword, an extension): the noise of
        the sampled latents instead of a fresh torch.randn draw."""
        a = self.args
        if kwargs.get("train_mode") and (getattr(a, "mi_loss_weight", 0) > 0 or getattr(a, "entropy_loss_weight", 0) > 0):
            raise NotImplementedError("MAIC training (the MI and entropy losses of network/MAIC.py:88-92) is not implemented: "
                                      "this agent is inference only")
        require_cuda("MAICAgent.forward")
        q, h = RNNQNet.forward(self, inputs, hidden_state)
        if q.shape[0] != bs * a.n_agents:
            raise ValueError("inputs has %d rows, bs * n_agents = %d" % (q.shape[0], bs * a.n_agents))
        self.head(h, q, bs, bool(test_mode), kwargs.get("eps"))
        return q, h, {}
