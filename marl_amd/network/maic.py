"""MAICAgent mirror (reference network/MAIC.py:10-94): the RNNQNet agent plus the MAIC message head.  ``forward`` is the
reference's inference forward; ``head_backward`` is the head's backward pass for the TD loss (MAICTDLearner).

The module tree and state_dict keys are the reference's, in its order (embed_net.{0,1,3}, inference_net.{0,1,3}, fc1, rnn,
fc2, msg_net.{0,2}, w_key, w_query, the BatchNorm buffers included), so a reference-trained state dict loads strictly.
The agent part is the HIP unroll kernel (csrc/agent.hip) as in RNNQNet; the head is csrc/maic_head.hip, its backward
csrc/maic_head_bwd.hip.  The MI and the attention-entropy loss (MAIC.py:88-123) are ``aux_backward`` (csrc/maic_aux.hip),
values and gradients in one call - the only place inference_net is evaluated; MAICTDLearner calls it.  ``forward`` itself does
not return the two losses: it still refuses ``train_mode`` with a positive weight for either.

BatchNorm follows the module's ``training`` flag as torch does: ``eval()`` normalises with the running statistics; in training
mode - the state of a freshly built module, and the reference never calls ``.eval()`` - with the statistics of all bs * N rows
of the call, and the running statistics move.  In that mode the rows of one call are coupled.
"""
import torch
import torch.nn as nn

from .. import ops
from ..hostutil import require_cuda
from ..hostutil import cached_module_struct
from .q_network import RNNQNet


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
        return cached_module_struct(self, "maic", ops.maic_weights, buffers=True)

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

    def head_backward(self, h, u_act, dq_val, bs, test_mode, eps, dh, dpar_extra=None):
        """Backward of ``head`` for the sparse gradient (u_act, dq_val) on the returned q, one pair per row: dh (bs*N, 64) =
        the head's contribution to the gradient on h (the identity path is BPTT's own), the head's weight gradients
        accumulate into the .grad views.  Same h, eps and modes as the forward call; the running statistics do not move
        (csrc/maic_head_bwd.hip).  ``dpar_extra``: ``aux_backward``'s dpar, carried through the same embed_net backward."""
        a = self.args
        kw = {} if dpar_extra is None else dict(dpar_extra=dpar_extra)
        ops.maic_head_bwd(self.maic_weights(), self.maic_grads(), h, u_act, dq_val, dh, bs, a.n_agents, a.n_actions,
                          test_mode=test_mode, bn_batch=self.training, eps=None if test_mode else eps, var_floor=a.var_floor,
                          bn_eps=self.embed_net[1].eps, **kw)

    def infer_weights(self):
        """marl_maic_infer_t over inference_net's current parameter and buffer storage"""
        return cached_module_struct(self, "maic_infer", ops.maic_infer_weights, buffers=True)

    def infer_grads(self):
        """marl_maic_infer_grads_t over inference_net's .grad views"""
        return ops.maic_infer_grads({k: v.grad for k, v in self.named_parameters() if k.startswith("inference_net.")})

    def aux_backward(self, h, q, bs, test_mode, eps, dpar, dh, mi_out, ent_out, den=None, dscale=1.0, weight_scale=1.0):
        """The two auxiliary losses of the reference's ``forward(train_mode=True)`` (MAIC.py:88-123) for one head call over
        ``bs`` environments, with their gradients (csrc/maic_aux.hip).  ``h`` (bs*N, 64), ``eps`` and the modes as the head call
        had them, ``q`` (bs*N, A) the Q values AFTER the messages were added.  With pair row (b*N + i)*N + j:

        MI (calculate_action_mi_loss): g1 = Normal(mean[b,i,j], sqrt(var[b,i,j])) from embed_net (var = max(exp(.), var_floor));
        a[b,j] = argmax q[b*N + j] - no availability mask, the lowest index wins a tie, not differentiated; inference_net reads
        [h[b,i] | onehot(a[b,j])], its BatchNorm runs over all bs*N*N pair rows (diagonal included) in this module's ``training``
        mode and in that mode moves inference_net.1's running statistics once per call, as torch does;
        g2 = Normal(out[:, :L], sqrt(max(exp(out[:, L:]), var_floor))); mi = mi_loss_weight * mean over the pairs of
        sum_L KL(g1 || g2).  Its gradient reaches inference_net, h through inference_net's input (-> ``dh``, written) and h
        and embed_net through mean / var (-> ``dpar`` (bs*N, 2*N*L), written: hand it to ``head_backward``); both clamps pass
        gradient only above the floor; nothing flows into q.

        Entropy: alpha = softmax_j(w_key(h) . w_query(latent)) with h and latent detached, NO 1/sqrt(D) scale and NO diagonal
        mask; ent = entropy_loss_weight * mean over the bs*N rows of -sum_j a' log2 a', a' = max(alpha, 1e-4).  Its gradient
        reaches only w_key and w_query (w_query.bias: analytically zero).

        ``mi_out`` / ``ent_out`` (one-float device views) += the two losses times ``weight_scale``; the gradients accumulate
        into the .grad views, scaled by weight_scale * dscale * den[0] (den None: 1).  embed_net.1's buffers are not touched."""
        a = self.args
        bn = self.inference_net[1]
        ops.maic_aux(self.maic_weights(), self.infer_weights(), self.maic_grads(), self.infer_grads(), h, q, bs,
                     a.n_agents, a.n_actions, weight_scale * getattr(a, "mi_loss_weight", 0.0),
                     weight_scale * getattr(a, "entropy_loss_weight", 0.0), mi_out, ent_out, dpar, dh, test_mode=test_mode,
                     bn_batch=self.training, eps=None if test_mode else eps, den=den, dscale=dscale, var_floor=a.var_floor,
                     bn_eps=bn.eps, bn_momentum=0.1 if bn.momentum is None else bn.momentum)

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
