"""MAVEN's networks (Mahajan et al., NeurIPS 2019; the reference ships no MAVEN - the definition is this project's own: DESIGN
section 9, include/marl_hip.h).

``MavenAgent`` is the plain RNNQNet agent plus four tables: for episode b with noise index k_b, agent n and hidden state h

    q'(b, t, n, :) = fc2(h) + (noise_w[k_b] + id_w[n]) h + noise_b[k_b] + id_b[n]

- NoiseRNNAgent's hyper-layer Linear(K + N -> A H) applied to [one-hot(k) | one-hot(n)]: a one-hot input makes it a sum of two table
rows, its bias matrix is fc2, and the second, A-wide hyper-layer gives the two bias tables.  The tables are initialised as the columns
of those nn.Linear layers would be.  The module tree is fc1 / rnn / fc2 / maven.{noise_w, id_w, noise_b, id_b}: the agent part of a
state dict is RNNQNet's.  The arithmetic is csrc/maven.hip (the head kernel after the unroll; fp32 in either gemm_mode).

``MavenDiscriminator`` is the parameter container of the MI pass: logits = l2(relu(l1([p_0 | .. | p_{N-1} | s]))), l1 (N A + S -> D),
l2 (D -> K); its parameters sit in the learner's flat buffer and it has no target copy."""
import torch
import torch.nn as nn

from .. import ops
from ..common.arguments import noise_dim_of, lambda_mi_of      # (the validators live beside get_maven_args)
from ..hostutil import cached_module_struct, cached_struct
from .q_network import RNNQNet


def maven_shape_of(args, n_agents=None, n_actions=None, state_shape=None):
    """(K, D) of a maven namespace as the kernels take them; a shape they do not cover is an error.  ``n_agents`` / ``n_actions`` /
    ``state_shape``: instead of the namespace's (the launcher checks before the environment is made)"""
    K = noise_dim_of(args)
    lambda_mi_of(args)
    D = getattr(args, "maven_discrim_dim", 64)
    N = args.n_agents if n_agents is None else n_agents
    A = args.n_actions if n_actions is None else n_actions
    S = args.state_shape if state_shape is None else state_shape
    if isinstance(D, bool) or not isinstance(D, int) or not ops.maven_supported(N, A, K, S, D):
        raise ValueError("MAVEN: %d agents, %d actions, state width %d, noise_dim %d and maven_discrim_dim %r are outside the kernels' "
                         "range (marl_maven_supported)" % (N, A, S, K, D))
    return K, D


class MavenTables(nn.Module):
    """noise_w (K, A, H), id_w (N, A, H), noise_b (K, A), id_b (N, A): the columns of Linear(K + N -> A H) and Linear(K + N -> A)"""

    def __init__(self, K, N, A, H):
        super().__init__()
        wl, bl = nn.Linear(K + N, A * H), nn.Linear(K + N, A)
        cols = lambda lin, lo, hi, *shape: nn.Parameter(lin.weight.detach()[:, lo:hi].t().reshape(hi - lo, *shape).contiguous().clone())
        self.noise_w, self.id_w = cols(wl, 0, K, A, H), cols(wl, K, K + N, A, H)
        self.noise_b, self.id_b = cols(bl, 0, K, A), cols(bl, K, K + N, A)


class MavenAgent(RNNQNet):
    def __init__(self, input_shape, args):
        super().__init__(input_shape, args)
        self.noise_dim = noise_dim_of(args)
        self.maven = MavenTables(self.noise_dim, args.n_agents, args.n_actions, args.rnn_hidden_dim)

    def maven_weights(self):
        """marl_maven_weights_t over the current parameter storage (rebuilt only when a parameter moved, as weights())"""
        return cached_module_struct(self, "maven", ops.maven_weights)

    def maven_grads(self):
        """marl_maven_grads_t over the tables' .grad views (the learner's flat gradient buffer)"""
        grads = {k: v.grad for k, v in self.named_parameters() if k.startswith("maven.")}
        return cached_struct(self, "maven_grads", grads.values(), lambda: ops.maven_grads(grads))


class MavenDiscriminator(nn.Module):
    def __init__(self, args):
        super().__init__()
        K, D = maven_shape_of(args)
        self.l1 = nn.Linear(args.n_agents * args.n_actions + args.state_shape, D)
        self.l2 = nn.Linear(D, K)

    def weights(self):
        return cached_module_struct(self, "maven_disc", ops.maven_disc)

    def grads(self):
        grads = {k: v.grad for k, v in self.named_parameters()}
        return cached_struct(self, "maven_disc_grads", grads.values(), lambda: ops.maven_disc_grads(grads))
