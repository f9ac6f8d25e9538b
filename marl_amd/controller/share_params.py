"""Multi-agent controller with shared parameters (mirror of reference
controller/share_params.py:8-182, class SharedMAC).

Same constructor / method surface; the network evaluation is the persistent HIP unroll kernel.
Batched extensions (not in the reference): ``step_batch`` for lock-step rollouts and the
``unroll`` primitive the learners use.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from ..hostutil import Scratch, require_cuda, to_dev, onehot_to_index, flatten_module
from ..network.mixer import x6_mode
from ..network.q_network import RNNQNet
from ..network.rtw import RTWAgent
from ..network.world_model import Agent as WorldAgent
from ..network.maic import MAICAgent
from ..network.commnet import CommNetAgent, FRONT_A
from ..network.g2anet import G2ANetAgent, tau_of
from ..network.maven import MavenAgent, maven_shape_of


class SharedMAC:
    # the head seam: a subclass whose Q values are "the unroll, then a head kernel that adds a term to q" overrides these two
    # attributes, _step_head (serial choose_action) and rollout_head (batched lock-step)
    head_name = None                  # as error texts name the head; None: the whole-rollout kernels may run
    stochastic = False                # True: training rollouts sample from the policy over the logits (PolicyMAC)
    choose_action_inputs = "agent"    # what the serial rollout hands choose_action: "agent" the agent's own row of obs /
                                      # last action / availability, "avail_all" every agent's availability, "all" all three whole

    def __init__(self, args):
        self.n_actions = args.n_actions
        self.n_agents = args.n_agents
        self.state_shape = args.state_shape
        self.obs_shape = args.obs_shape
        self.args = args
        input_shape = self._get_input_shape()
        self._build_agents(input_shape)
        self.hidden_states = None   # (n_episodes, n_agents, hidden_dim)
        self._dev = None

    # ------------------------------------------------------------------ plumbing
    def _get_input_shape(self):
        """reference share_params.py:114-123"""
        shape = self.obs_shape
        if self.args.last_action:
            shape += self.n_actions
        if self.args.reuse_network:
            shape += self.n_agents
        return shape

    def _build_agents(self, input_shape):
        self.agent = RNNQNet(input_shape, self.args)

    def device(self):
        if self._dev is None:
            self._dev = require_cuda("SharedMAC")
        p = next(self.agent.parameters())
        if p.device != self._dev:
            self.cuda()
        return self._dev

    def cuda(self):
        dev = require_cuda("SharedMAC")
        self._dev = dev
        if next(self.agent.parameters()).device != dev or not hasattr(self.agent, "_flat"):
            self.agent.to(dev)
            flatten_module(self.agent, dev)

    def parameters(self):
        return self.agent.parameters()

    def load_state(self, other_mac):
        src, dst = getattr(other_mac.agent, "_flat", None), getattr(self.agent, "_flat", None)
        if src is not None and dst is not None and src.n == dst.n and _is_flat(other_mac.agent) and _is_flat(self.agent):
            dst.flat.copy_(src.flat)       # one D2D copy
        else:
            self.agent.load_state_dict(other_mac.agent.state_dict())

    def save_models(self, path):
        torch.save({k: v.detach().cpu() for k, v in self.agent.state_dict().items()}, path)

    def load_models(self, path):
        self.agent.load_state_dict(torch.load(path, map_location="cpu"))

    def init_hidden(self, episode_num):
        """zeros (episodes, N, H) - reference :74-76 (here on the device)."""
        self.hidden_states = torch.zeros((episode_num, self.n_agents, self.args.rnn_hidden_dim), device=self.device())

    # ------------------------------------------------------------------ serial action choice
    def choose_action(self, obs, last_action, agent_num, avail_actions, epsilon, evaluate=False):
        """One agent, one env (reference :37-72), same numpy RNG draw order: one uniform per call, one choice only when
        exploring.  ``avail_actions``: the agent's row, or every agent's (choose_action_inputs = "avail_all")."""
        avail = np.asarray(avail_actions, dtype=np.float32)
        if self.choose_action_inputs == "avail_all":
            avail = avail.reshape(self.n_agents, self.n_actions)
        obs_full, ufed = self._one_agent_inputs(obs, last_action, agent_num)
        q, h_out = self._agent_step_one(obs_full, ufed)
        self._step_head(h_out, q, obs_full, avail, evaluate)
        self.hidden_states[0, agent_num] = h_out[agent_num]
        return self._draw(q[0, 0, agent_num].cpu(), avail if avail.ndim == 1 else avail[agent_num], epsilon)

    def _one_agent_inputs(self, obs, last_action, agent_num):
        """(obs_full (1,1,N,O), ufed (1,1,N)) that run row ``agent_num`` of a 1-episode batch: the agent axis is padded so the id
        block matches; the last-action index is -1 where there is none"""
        dev = self.device()
        N, O = self.n_agents, self.obs_shape
        la = -1
        if self.args.last_action:
            nz = np.nonzero(np.asarray(last_action))[0]
            la = int(nz[0]) if nz.size else -1
        obs_full = torch.zeros(1, 1, N, O, device=dev)
        obs_full[0, 0, agent_num] = to_dev(np.asarray(obs, dtype=np.float32).reshape(O), dev)
        ufed = torch.full((1, 1, N), -1, dtype=torch.int32, device=dev)
        ufed[0, 0, agent_num] = la
        return obs_full, ufed

    def _agent_step_one(self, obs_full, ufed):
        """the T = 1 unroll of one environment from self.hidden_states: (q (1,1,N,A), h_out (N,H))"""
        N, A, O = self.n_agents, self.n_actions, self.obs_shape
        q = torch.empty(1, 1, N, A, device=obs_full.device)
        h_in = self.hidden_states.reshape(N, -1).contiguous()
        h_out = torch.empty_like(h_in)
        ops.agent_unroll_fwd(self.agent.weights(), obs_full, N, 0, ufed, N, 0, h_in, q, None, h_out, None,
                             1, 1, N, O, A, self.args.last_action, self.args.reuse_network)
        return q, h_out

    def _step_head(self, h_out, q, obs_full, avail, evaluate):
        """q (1,1,N,A) += the head's term for one environment; ``avail`` as choose_action received it"""

    @staticmethod
    def _draw(q_row, avail_row, epsilon):
        """epsilon-greedy over the available actions: one uniform, one choice only when exploring"""
        q_row[torch.as_tensor(avail_row, dtype=torch.float32) == 0.0] = -float("inf")
        if np.random.uniform() < epsilon:
            return np.random.choice(np.nonzero(avail_row)[0])
        return torch.argmax(q_row)

    def rollout_head(self, h, q, rec, t, E, evaluate, rseed, env):
        """q (E,1,N,A) += the head's term at lock-step t of a batched rollout (h (E*N,H): the step's GRU output)"""

    def rollout_weights(self):
        """what a batched rollout looks up once and hands to every ``rollout_step``"""
        return self.agent.weights()

    def rollout_step(self, w, rec, t, h, q, E):
        """the agent step of lock-step t of a batched rollout: the unroll kernel with T = 1 reading slot t of the record in place;
        h (E*N,H) is advanced in place, q (E,1,N,A) written"""
        N, T, a = self.n_agents, rec.T, self.args
        ops.agent_unroll_fwd(w, rec.obs, (T + 1) * N, t, rec.u, T * N, t - 1, h, q, None, h, None,
                             E, 1, N, self.obs_shape, self.n_actions, a.last_action, a.reuse_network)

    # ------------------------------------------------------------------ batched primitives
    def unroll_x6(self, B, T, obs=None):
        """True when a T-step unroll over B episodes runs on the bf16x6 split kernel (args.gemm_mode = "bf16x6", a shape
        csrc/agent_x6.hip covers and - when given - an observation tensor on a 16-byte boundary: a misaligned view takes the
        fp32 kernels instead of failing in the entry point)."""
        return (T >= 4 and x6_mode(self.args)
                and (obs is None or obs.data_ptr() % 16 == 0)
                and ops.agent_unroll_x6_supported(B, T, self.n_agents, self.obs_shape, self.n_actions, self.args.last_action,
                                                  self.args.reuse_network))

    def unroll(self, obs, obs_bs, obs_t0, ufed, u_bs, u_t0, B, T, q, hs=None, h_last=None, saved=None, h0="state",
               ep_len=None, ep_map=None, cu_budget=0, gi_out=None, gi_in=None):
        """T-step unroll over B episodes starting from self.hidden_states (or zeros if None)."""
        dev = self.device()
        N, A, O = self.n_agents, self.n_actions, self.obs_shape
        if h0 == "state":
            h0 = None if self.hidden_states is None else self.hidden_states.reshape(B * N, -1).contiguous()
        if self.unroll_x6(B, T, obs):
            # opt-in: every product of the unroll as six bf16 MFMA products (csrc/agent_x6.hip); same `saved` layout, so the
            # fp32 BPTT kernel runs from it; gi_out / gi_in pair up because every unroll of these dimensions comes here
            ops.agent_unroll_fwd_x6(self.agent.weights(), obs, obs_bs, obs_t0, ufed, u_bs, u_t0, h0, q, hs, h_last, saved,
                                    B, T, N, O, A, self.args.last_action, self.args.reuse_network, ep_len=ep_len, ep_map=ep_map,
                                    cu_budget=cu_budget, gi_out=gi_out, gi_in=gi_in)
            return
        ops.agent_unroll_fwd(self.agent.weights(), obs, obs_bs, obs_t0, ufed, u_bs, u_t0, h0, q, hs, h_last, saved,
                             B, T, N, O, A, self.args.last_action, self.args.reuse_network, ep_len=ep_len, ep_map=ep_map,
                             cu_budget=cu_budget, gi_out=gi_out, gi_in=gi_in)

    def _batch_unroll(self, batch, T, which):
        dev = self.device()
        N, A, O, H = self.n_agents, self.n_actions, self.obs_shape, self.args.rnn_hidden_dim
        key = "o" if which == "cur" else "o_next"
        obs = to_dev(batch[key][:, :T], dev)
        B = obs.shape[0]
        if "u_idx" in batch:
            uidx = to_dev(batch["u_idx"][:, :T], dev, torch.int32).view(B, T, N)
        else:
            uidx = onehot_to_index(to_dev(batch["u_onehot"][:, :T], dev)).view(B, T, N)
        q = torch.empty(B, T, N, A, device=dev)
        hs = torch.empty(B, T, N, H, device=dev)
        h_last = torch.empty(B * N, H, device=dev)
        self.unroll(obs, T * N, 0, uidx, T * N, -1 if which == "cur" else 0, B, T, q, hs, h_last)
        self.hidden_states = h_last.view(B, N, H)
        return q, hs

    def get_current_q_values(self, batch, max_episode_len):
        """q (B,T,N,A) and the hidden state after each step (B,T,N,H) - reference :125-146."""
        return self._batch_unroll(batch, max_episode_len, "cur")

    def get_next_q_values(self, batch, max_episode_len):
        """reference :148-168 (inputs o_next, u_onehot[t])."""
        return self._batch_unroll(batch, max_episode_len, "next")


def _is_flat(module):
    fp = getattr(module, "_flat", None)
    if fp is None:
        return False
    ps = list(module.parameters())
    return len(ps) == len(fp.params) and all(p.data.data_ptr() == fp.flat.data_ptr() + 4 * o
                                              for p, o in zip(ps, fp.offsets))


class _Unsupported:
    def __init__(self, *a, **k):
        raise NotImplementedError("%s is outside the MI355X hot path (see DESIGN.md, out of scope)" % type(self).__name__)


class SeparatedMAC(_Unsupported):
    """name kept for `from controller.share_params import ...` (reference runner.py:4); the reference class is broken."""


class SharedMACWithState(SharedMAC):
    """reference controller/share_params.py:185-387: SharedMAC over a world_model.Agent, whose Q values include the world
    head's r (network/world_model.py:71).  Every pass is the agent unroll followed by the head (csrc/world_head.hip)."""

    world = True                      # QLearnerWithState asks for it
    head_name = "world-model"

    def _build_agents(self, input_shape):
        self.agent = WorldAgent(input_shape, self.args)

    def _step_head(self, h_out, q, obs_full, avail, evaluate):
        """q += r (reference :214-260)"""
        ops.world_head_fwd(self.agent.world_weights(), h_out, q, 1, 1, self.n_agents, self.obs_shape, self.n_actions)

    def rollout_head(self, h, q, rec, t, E, evaluate, rseed, env):
        """q += r: choose_action for every agent of every environment"""
        ops.world_head_fwd(self.agent.world_weights(), h, q, E, 1, self.n_agents, self.obs_shape, self.n_actions)

    def head(self, hs, q, B, T, with_ohat=True, with_tau=True):
        """q (B,T,N,A) += r from hs (B,T,N,64); returns the reference's `returns` dict (:303-375) without ep_hidden_states"""
        dev = hs.device
        N, A, O = self.n_agents, self.n_actions, self.obs_shape
        r = torch.empty(B, T, N, A, device=dev)
        ohat = torch.empty(B, T, N, O, device=dev) if with_ohat else None
        tau = torch.empty(B, T, N, 2, device=dev) if with_tau else None
        ops.world_head_fwd(self.agent.world_weights(), hs, q, B, T, N, O, A, r_out=r, ohat_out=ohat, tau_out=tau)
        return {"r": r, "o_next": ohat, "terminated": tau}

    def _world_q_values(self, batch, T, which):
        q, hs = self._batch_unroll(batch, T, which)
        returns = {"ep_hidden_states": hs}
        returns.update(self.head(hs, q, q.shape[0], T))
        return q, returns

    def get_current_q_values(self, batch, max_episode_len):
        """(q + r, returns{ep_hidden_states, r, o_next, terminated}) - reference :303-338"""
        return self._world_q_values(batch, max_episode_len, "cur")

    def get_next_q_values(self, batch, max_episode_len):
        """reference :340-375 (inputs o_next, u_onehot[t])"""
        return self._world_q_values(batch, max_episode_len, "next")


class PolicyMAC(SharedMAC):
    """The actor of the actor-critic learners (central-V): SharedMAC over the unchanged RNNQNet, whose fc2 output is read as the
    logits of a stochastic policy (csrc/policy.hip: the softmax mixed with epsilon of the uniform policy over the available
    actions).  Training rollouts sample from it - ``stochastic`` makes the whole-rollout kernel and the fused step draw from the
    policy, and the unfused path call ops.policy_sample in the place of ops.select_actions (one rule, one stream of draws:
    marl_amd/rollout.py); evaluation is greedy, and the policy's argmax over the available actions is the masked argmax of
    the logits, so an evaluation rollout is SharedMAC's at epsilon 0, the whole-rollout kernel included."""

    stochastic = True

    def choose_action(self, obs, last_action, agent_num, avail_actions, epsilon, evaluate=False):
        """One agent, one env: pi of the agent's row, then its argmax (``evaluate``) or one np.random.choice draw from it."""
        dev, A = self.device(), self.n_actions
        avail = np.asarray(avail_actions, dtype=np.float32).reshape(A)
        obs_full, ufed = self._one_agent_inputs(obs, last_action, agent_num)
        q, h_out = self._agent_step_one(obs_full, ufed)
        self.hidden_states[0, agent_num] = h_out[agent_num]
        pi = torch.empty(1, A, device=dev)
        ops.policy_probs(q[0, 0, agent_num].contiguous().view(1, A), to_dev(avail, dev).view(1, A),
                         0.0 if evaluate else epsilon, pi, 1, A)
        pi = pi[0].cpu().numpy().astype(np.float64)
        if evaluate:
            return int(np.argmax(pi))
        return int(np.random.choice(A, p=pi / pi.sum()))


class GroupHeadMAC(PolicyMAC):
    """PolicyMAC whose logits of an environment-step come from all N agents' hidden states: every pass is a front (what feeds the
    recurrence, and the agent unroll over it - the fp32 kernels in either gemm_mode) followed by a group head.  ``unroll`` and
    ``backward`` (what the policy learners call in the place of agent_backward) are written here once; an actor supplies
      ``planes_cls`` / ``extra``     the planes its backward reads: hs and one more, under that attribute and scratch name
      ``_extra_plane(get, name, B, T)``   that plane (B, T, N, .) from ``get``, filled if an unroll only reads it
      ``_front_forward(src, B, T, extra, h0, hs, h_last, saved, **kw)``   the recurrence's input and ops.agent_unroll_fwd
      ``_head_forward(hs, extra, q, G)`` / ``_head_backward(hs, extra, dlogits, dhs, G)``   the head over G = B T groups
      ``front_cell`` / ``front_rows``   the GRUCell that holds the recurrence's gradients, the rows of the dummy fc2 (None: n_actions)
      ``_after_bptt(dxp, extra)``    between BPTT and the encoder's weight gradient (nothing by default)."""

    planes_cls = extra = couples = front_cell = front_rows = None

    def __init__(self, args):
        PolicyMAC.__init__(self, args)
        self._buf = Scratch()

    def _scratch(self, name, shape, dtype=torch.float32, zero=False):
        return self._buf.get(name, shape, self.device(), dtype, zero)

    def choose_action(self, obs, last_action, agent_num, avail_actions, epsilon, evaluate=False):
        raise NotImplementedError("%s.choose_action: %s needs every agent's observation in one call - use a batched rollout"
                                  % (type(self).__name__, self.couples))

    def rollout_weights(self):
        return None

    def _input(self, obs, remap0, ufed, remapi, ep_map=None):
        """the virtual input [obs | one-hot(u_{t-1}) | agent id] as agent_backward builds it"""
        return ops.agent_input_src(self.args, self.n_agents, self.n_actions, self.obs_shape, obs, remap0, ufed, remapi, ep_map)

    def _after_bptt(self, dxp, extra):
        pass

    def unroll(self, obs, obs_bs, obs_t0, ufed, u_bs, u_t0, B, T, q, hs=None, h_last=None, saved=None, h0="state",
               ep_len=None, ep_map=None, cu_budget=0, gi_out=None, gi_in=None):
        """SharedMAC.unroll's signature; q receives the logits.  ``hs``: None, a (B, T, N, H) tensor, or the ``planes_cls`` a later
        ``backward`` reads (``planes``).  Without planes the extra plane is the controller's own scratch (and the learner's planes
        stay untouched).  Gate-sum reuse does not exist here."""
        if gi_out is not None or gi_in is not None:
            raise ValueError("%s.unroll has no gate-sum reuse" % type(self).__name__)
        N, H = self.n_agents, self.args.rnn_hidden_dim
        if B == 0:
            return
        if h0 == "state":
            h0 = None if self.hidden_states is None else self.hidden_states.reshape(B * N, -1).contiguous()
        if isinstance(hs, self.planes_cls):
            assert tuple(hs.hs.shape) == (B, T, N, H)
            extra, hs = getattr(hs, self.extra), hs.hs
        else:
            extra = self._extra_plane(self._scratch, self.extra, B, T)
            if hs is None:
                hs = self._scratch("hs", (B, T, N, H))
        self._front_forward((obs, obs_bs, obs_t0, ufed, u_bs, u_t0), B, T, extra, h0, hs, h_last, saved, ep_len=ep_len, ep_map=ep_map,
                            cu_budget=cu_budget)
        self._head_forward(hs, extra, q, B * T)

    def planes(self, get, shape):
        """the ``planes_cls`` of an unroll of ``shape`` = (B, T, N, H) in buffers from ``get(name, shape)`` (the learner's scratch)"""
        return self.planes_cls(get("hs", shape), self._extra_plane(get, "%s_%s" % (self.head_name, self.extra), shape[0], shape[1]))

    def backward(self, db, saved, planes, dlogits, buf):
        """The backward of the ``unroll`` that wrote ``planes`` (and ``saved``), on the batch's current observations: the head's
        backward (dhs and the head's gradients), BPTT through the front with dhs as the gradient on the hidden states (the
        gradients of ``front_cell`` and dxp; a pair of zeros for dq, the dummy fc2's gradients go to scratch), ``_after_bptt``
        and the encoder's weight gradient over the virtual input - accumulated into the .grad views."""
        B, T, N = db.B, db.T, db.N
        H = self.args.rnn_hidden_dim
        M = B * T * N
        if M == 0:
            return
        if not isinstance(planes, self.planes_cls) or tuple(planes.hs.shape) != (B, T, N, H):
            raise TypeError("%s.backward reads the %s (B, T, N, H) its unroll was given" % (type(self).__name__, self.planes_cls.__name__))
        hs, extra = planes.hs, getattr(planes, self.extra)
        ag, dev = self.agent, hs.device
        dhs = buf.get(self.head_name + "_dhs", (B, T, N, H), dev)
        self._head_backward(hs, extra, dlogits, dhs, B * T)
        dxp = buf.get("dxp", (B, T, N, H), dev)
        # the BPTT entry wants one form of dq: a sparse pair of zeros; the dummy fc2's gradients go to scratch
        zi, zv = self._scratch("dq_idx", (M,), torch.int32, zero=True), self._scratch("dq_val", (M,), zero=True)
        cell, rows = getattr(ag, self.front_cell), self.front_rows or self.n_actions
        grads = {"rnn.weight_ih": cell.weight_ih.grad, "rnn.weight_hh": cell.weight_hh.grad,
                 "rnn.bias_ih": cell.bias_ih.grad, "rnn.bias_hh": cell.bias_hh.grad,
                 "fc2.weight": self._scratch("d_dummy_w", (rows, H)), "fc2.bias": self._scratch("d_dummy_b", (rows,))}
        ops.agent_unroll_bwd(ag.front_weights(), None, dhs, saved, None, dxp, None, grads, B, T, N, rows, dq_idx=zi, dq_val=zv, x6=False)
        self._after_bptt(dxp, extra)
        obs, obs_bs, obs_t0 = db.o_cur
        x = self._input(obs, (T * N, obs_bs, obs_t0 * N), db.u_fed, (T * N, db.u_bs, -N), getattr(db, "o_map", None))
        ops.linear_wgrad(dxp.view(M, H), x, ag.encoding.weight.grad, ag.encoding.bias.grad, M, H, self._get_input_shape(), bf16=False)


def commnet_k_of(args, n_agents=None, n_actions=None):
    """args.k as the head kernels take it; anything they do not cover is an error.  ``n_agents`` / ``n_actions``: instead of the
    namespace's (the launcher checks k alone before it knows them)"""
    k = getattr(args, "k", None)
    N = args.n_agents if n_agents is None else n_agents
    A = args.n_actions if n_actions is None else n_actions
    if isinstance(k, bool) or not isinstance(k, int) or not ops.commnet_supported(N, A, k):
        raise ValueError("CommNet: k = %r rounds with %d agents and %d actions is outside the head kernels' range "
                         "(marl_commnet_supported)" % (k, N, A))
    return k


class CommNetPlanes:
    """What CommNetMAC.backward reads of the unroll it follows, in buffers the caller owns: the hidden states ``hs`` and the encoder's
    output ``e``, both (B, T, N, H).  Passed to ``unroll`` in the place of ``hs`` and then to ``backward``: an unroll that is not given
    these planes cannot write them."""

    def __init__(self, hs, e):
        assert hs.shape == e.shape and hs.is_contiguous() and e.is_contiguous()
        self.hs, self.e = hs, e


class CommNetMAC(GroupHeadMAC):
    """GroupHeadMAC over a CommNetAgent (network/commnet.py; the project's own definition - DESIGN section 9).  The front is the
    encoder (ops.linear + the sigmoid kernel, into the plane ``e``) and the agent unroll over the identity front layer (h_t =
    f_obs(e_t, h_{t-1})), so BPTT's dxp is the gradient on e and the sigmoid's backward follows it; the head is the communication head
    (csrc/commnet.hip).

    Padded steps: the encoder reads the stored observation rows (no zero padding at t >= ep_len), so logits there are finite and
    deterministic but are not the float64 restatement's; every loss masks them and the recurrence runs forward only."""

    head_name = "commnet"
    planes_cls, extra, couples = CommNetPlanes, "e", "communication"
    front_cell, front_rows = "f_obs", FRONT_A

    def __init__(self, args):
        self.k = commnet_k_of(args)          # raises before anything is built
        GroupHeadMAC.__init__(self, args)

    def _build_agents(self, input_shape):
        self.agent = CommNetAgent(input_shape, self.args)

    def _encode(self, x, e, M):
        """e (M, 64) = sigmoid(encoding(x))"""
        ag = self.agent
        ops.linear(x, ag.encoding.weight, ag.encoding.bias, e.view(M, -1), M, self.args.rnn_hidden_dim, self._get_input_shape())
        ops.commnet_sigmoid_fwd(e)

    def rollout_step(self, w, rec, t, h, q, E):
        N, T, A, H = self.n_agents, rec.T, self.n_actions, self.args.rnn_hidden_dim
        if E == 0:
            return
        x = self._input(rec.obs, (N, (T + 1) * N, t * N), rec.u, (N, T * N, (t - 1) * N))
        e = self._scratch("step_e", (E, 1, N, H))
        self._encode(x, e, E * N)
        ops.agent_unroll_fwd(self.agent.front_weights(), e, N, 0, None, 0, 0, h, self._scratch("step_q", (E, 1, N, FRONT_A)),
                             None, h, None, E, 1, N, H, FRONT_A, False, False)
        ops.commnet_head_fwd(self.agent.head_weights(), h, q, E, N, A, self.k)

    def _extra_plane(self, get, name, B, T):
        return get(name, (B, T, self.n_agents, self.args.rnn_hidden_dim))

    def _front_forward(self, src, B, T, e, h0, hs, h_last, saved, ep_len=None, ep_map=None, cu_budget=0):
        """``ep_len`` is not applied to the encoder (class docstring)"""
        obs, obs_bs, obs_t0, ufed, u_bs, u_t0 = src
        N, H = self.n_agents, self.args.rnn_hidden_dim
        self._encode(self._input(obs, (T * N, obs_bs, obs_t0 * N), ufed, (T * N, u_bs, u_t0 * N), ep_map), e, B * T * N)
        ops.agent_unroll_fwd(self.agent.front_weights(), e, T * N, 0, None, 0, 0, h0, self._scratch("q0", (B, T, N, FRONT_A)),
                             hs, h_last, saved, B, T, N, H, FRONT_A, False, False, cu_budget=cu_budget)

    def _head_forward(self, hs, e, q, G):
        ops.commnet_head_fwd(self.agent.head_weights(), hs, q, G, self.n_agents, self.n_actions, self.k)

    def _head_backward(self, hs, e, dlogits, dhs, G):
        """dhs and the gradients of f_comm and decoding"""
        ag = self.agent
        ops.commnet_head_bwd(ag.head_weights(), ag.head_grads(), hs, dlogits, dhs, G, self.n_agents, self.n_actions, self.k)

    def _after_bptt(self, de, e):
        ops.commnet_sigmoid_bwd(de, e, de)


def g2anet_shape_of(args, n_agents=None, n_actions=None):
    """(hard, tau) of a +g2anet namespace as the head kernels take them; a shape they do not cover is an error.  ``n_agents`` /
    ``n_actions``: instead of the namespace's"""
    N = args.n_agents if n_agents is None else n_agents
    A = args.n_actions if n_actions is None else n_actions
    hard = bool(getattr(args, "hard", True))
    tau = tau_of(args)
    if not ops.g2anet_supported(N, A, hard):
        raise ValueError("G2ANet: %d agents and %d actions are outside the head kernels' range (marl_g2anet_supported)" % (N, A))
    return hard, tau


G2ANET_UPDATE_SALT = 0x5BD1E995      # the learner's update noise is keyed by args.seed ^ this: never the rollout's (seed, env, step)


class G2ANetPlanes:
    """What G2ANetMAC.backward reads of the unroll it follows, in buffers the caller owns: the hidden states ``hs`` (B, T, N, H) and
    the hard attention's noise ``noise`` (B, T, N, N-1) the unroll's head ran on.  Passed to ``unroll`` in the place of ``hs`` and then
    to ``backward``: an unroll that is not given these planes cannot write them."""

    def __init__(self, hs, noise):
        assert hs.is_contiguous() and noise.is_contiguous() and tuple(noise.shape) == tuple(hs.shape[:3]) + (hs.shape[2] - 1,)
        self.hs, self.noise = hs, noise


class G2ANetMAC(GroupHeadMAC):
    """GroupHeadMAC over a G2ANetAgent (network/g2anet.py; the project's own definition - DESIGN section 9).  The front is the agent
    unroll over the observation with fc1 = encoding, rnn = h and a zero fc2; the head is the hard and the soft attention
    (csrc/g2anet.hip), run on the plane ``noise`` (B, T, N, N-1) that an unroll only reads.

    Noise (as published: drawn in every pass, evaluation included): a rollout step's is keyed by (seed, environment, global step),
    an update's by (args.seed ^ G2ANET_UPDATE_SALT, episode index in the batch, train_step * episode_limit + t) - fresh every update,
    the same after a resume, never the rollout's.  ``set_train_step`` tells the controller the update it is in."""

    head_name = "g2anet"
    planes_cls, extra, couples = G2ANetPlanes, "noise", "attention"
    front_cell = "h"                 # front_rows: n_actions

    def __init__(self, args):
        self.hard, self.tau = g2anet_shape_of(args)      # raises before anything is built
        GroupHeadMAC.__init__(self, args)
        self.train_step = 0

    def _build_agents(self, input_shape):
        self.agent = G2ANetAgent(input_shape, self.args)

    def set_train_step(self, train_step):
        self.train_step = int(train_step)

    def update_noise(self, noise, B, T):
        """noise (B, T, N, N-1) <- the draws of the update ``self.train_step`` (not read with hard off: left alone)"""
        if self.hard and B * T > 0:
            ops.g2anet_noise(getattr(self.args, "seed", 0) ^ G2ANET_UPDATE_SALT, 0, self.train_step * self.args.episode_limit, noise,
                             B, T, self.n_agents)

    def rollout_step(self, w, rec, t, h, q, E):
        """h_t of lock-step t (the T = 1 unroll reading slot t of the record in place); q is written by ``rollout_head``"""
        N, T, A, a = self.n_agents, rec.T, self.n_actions, self.args
        if E == 0:
            return
        ops.agent_unroll_fwd(self.agent.front_weights(), rec.obs, (T + 1) * N, t, rec.u, T * N, t - 1, h, self._scratch("step_q", (E, 1, N, A)),
                             None, h, None, E, 1, N, self.obs_shape, A, a.last_action, a.reuse_network)

    def rollout_head(self, h, q, rec, t, E, evaluate, rseed, env):
        """q (E,1,N,A) is WRITTEN with the head's logits on h; the step's noise is the counter hash of (rseed, environment, global
        step), exploring or evaluating"""
        N, A = self.n_agents, self.n_actions
        if E == 0:
            return
        noise = None
        if self.hard:
            noise = self._scratch("step_noise", (E, 1, N, N - 1))
            ops.g2anet_noise(rseed, env.env0, env.global_step(t), noise, E, 1, N)
        ops.g2anet_head_fwd(self.agent.head_weights(), h, noise, q, E, N, A, self.hard, self.tau)

    def _extra_plane(self, get, name, B, T):
        """the noise of the update ``self.train_step``, drawn into the plane"""
        N = self.n_agents
        noise = get(name, (B, T, N, N - 1))
        self.update_noise(noise, B, T)
        return noise

    def _front_forward(self, src, B, T, noise, h0, hs, h_last, saved, ep_len=None, ep_map=None, cu_budget=0):
        N, A, a = self.n_agents, self.n_actions, self.args
        ops.agent_unroll_fwd(self.agent.front_weights(), *src, h0, self._scratch("q0", (B, T, N, A)),
                             hs, h_last, saved, B, T, N, self.obs_shape, A, a.last_action, a.reuse_network, ep_len=ep_len,
                             ep_map=ep_map, cu_budget=cu_budget)

    def _head_forward(self, hs, noise, q, G):
        ops.g2anet_head_fwd(self.agent.head_weights(), hs, noise if self.hard else None, q, G, self.n_agents, self.n_actions,
                            self.hard, self.tau)

    def _head_backward(self, hs, noise, dlogits, dhs, G):
        """on the unroll's noise: dhs and the sixteen head gradients"""
        ag = self.agent
        ops.g2anet_head_bwd(ag.head_weights(), ag.head_grads(), hs, noise if self.hard else None, dlogits, dhs, G, self.n_agents,
                            self.n_actions, self.hard, self.tau)


class MAVENMAC(SharedMAC):
    """SharedMAC over a MavenAgent (network/maven.py; the project's own definition - DESIGN section 9).  Every pass is the agent unroll
    followed by the noise-conditioned head (csrc/maven.hip), which adds (noise_w[k_b] + id_w[n]) h + noise_b[k_b] + id_b[n] to q.
    Every episode carries one noise index k_b in [0, noise_dim): a batched rollout draws it at its first lock-step from the counter hash
    keyed by (seed, environment, the rollout's first global step) - exploring or evaluating - keeps it in ``self.noise`` and leaves it
    on the record (``rec.noise``), from where the replay ring and the learner's batch carry it.  The serial ``choose_action`` path has no
    episode to hang the draw on and is not provided."""

    head_name = "MAVEN"

    def __init__(self, args):
        self.noise_dim, _ = maven_shape_of(args)       # raises before anything is built
        SharedMAC.__init__(self, args)
        self.noise = None             # (E,) int32: the noise indices of the rollout in progress

    def _build_agents(self, input_shape):
        self.agent = MavenAgent(input_shape, self.args)

    def choose_action(self, obs, last_action, agent_num, avail_actions, epsilon, evaluate=False):
        raise NotImplementedError("MAVENMAC.choose_action: the noise index is drawn once per episode of a batched rollout - use a "
                                  "batched rollout")

    def _step_head(self, h_out, q, obs_full, avail, evaluate):
        raise NotImplementedError("MAVENMAC has no serial step: the noise index is drawn once per episode of a batched rollout")

    def rollout_head(self, h, q, rec, t, E, evaluate, rseed, env):
        """at t = 0 the episodes' noise is drawn and left on the record; at every step q (E,1,N,A) += the head's term on h"""
        if E == 0:
            return
        if t == 0:
            self.noise = torch.empty(E, dtype=torch.int32, device=h.device)      # a fresh array: the last record keeps its own
            ops.maven_noise(rseed, env.env0, env.global_step(0), self.noise_dim, self.noise, E)
            rec.noise = self.noise
        ops.maven_head_fwd(self.agent.maven_weights(), h, self.noise, q, E, 1, self.n_agents, self.n_actions, self.noise_dim)

    def head(self, hs, noise, q, B, T):
        """q (B,T,N,A) += the head's term from hs (B,T,N,64) and the episodes' noise (B,) int32"""
        ops.maven_head_fwd(self.agent.maven_weights(), hs, noise, q, B, T, self.n_agents, self.n_actions, self.noise_dim)

    def _maven_q_values(self, batch, T, which):
        if not dict.__contains__(batch, "noise"):
            raise ValueError("MAVENMAC needs the batch's noise indices (batch['noise'], one per episode)")
        q, hs = self._batch_unroll(batch, T, which)
        noise = to_dev(batch["noise"], q.device, torch.int32).view(q.shape[0])
        self.head(hs, noise, q, q.shape[0], T)
        return q, hs

    def get_current_q_values(self, batch, max_episode_len):
        """q (B,T,N,A) with the head's term for batch['noise'], and hs (B,T,N,H)"""
        return self._maven_q_values(batch, max_episode_len, "cur")

    def get_next_q_values(self, batch, max_episode_len):
        """as get_current_q_values on (o_next, u_onehot[t])"""
        return self._maven_q_values(batch, max_episode_len, "next")


class RTWMAC(SharedMAC):
    """reference controller/share_params.py:612-804: SharedMAC over an RTWAgent.  Inference only: choose_action (act mode,
    :641-677) and get_current_q_values (given mode, :730-764) run the agent unroll followed by the reflection head
    (csrc/rtw_head.hip).  get_next_q_values fails with the reference's TypeError (RTWAgent.forward target=True), so
    RTWQLearner.train cannot run - in the reference either."""

    head_name = "RTW"
    choose_action_inputs = "avail_all"

    def _build_agents(self, input_shape):
        self.agent = RTWAgent(input_shape, self.args)

    def not_self_model(self):
        return bool(getattr(self.args, "not_self_model", True))

    def _step_head(self, h_out, q, obs_full, avail, evaluate):
        """q += the reflection term (reference :641-677).  The head reads row agent_num's h and o and every agent's
        availability (rollout.py:73-74); the other rows of the tile are discarded."""
        N, A, O = self.n_agents, self.n_actions, self.obs_shape
        ops.rtw_head_act(self.agent.rtw_weights(), h_out, obs_full, N, 0, to_dev(avail, h_out.device), N, 0, q,
                         1, N, O, A, self.not_self_model())

    def rollout_head(self, h, q, rec, t, E, evaluate, rseed, env):
        """q += the reflection term from slot t of the record: choose_action for every agent of every environment"""
        N, A, O, T = self.n_agents, self.n_actions, self.obs_shape, rec.T
        ops.rtw_head_act(self.agent.rtw_weights(), h, rec.obs, (T + 1) * N, t, rec.avail, (T + 1) * N, t, q, E, N, O, A,
                         self.not_self_model())

    def get_current_q_values(self, batch, max_episode_len):
        """(q, hs, 0.0, 0.0) - reference :730-764: the unroll, then the given-mode head with the taken actions and o_next."""
        T = max_episode_len
        q, hs = self._batch_unroll(batch, T, "cur")
        dev = q.device
        N, A, O = self.n_agents, self.n_actions, self.obs_shape
        B = q.shape[0]
        o = to_dev(batch["o"][:, :T], dev)
        on = to_dev(batch["o_next"][:, :T], dev)
        u = to_dev(batch["u"][:, :T], dev, torch.int32).view(B, T, N)
        ops.rtw_head_given(self.agent.rtw_weights(), hs, o, T * N, 0, on, T * N, 0, u, T * N, 0, q, B, T, N, O, A,
                           self.not_self_model())
        return q, hs, 0.0, 0.0

    def get_next_q_values(self, batch, max_episode_len):
        """reference :766-789 passes obs_next = None and u = None into RTWAgent.forward, which fails (RTW.py:178)."""
        raise TypeError("RTWMAC.get_next_q_values: the reference's target pass concatenates obs with obs_next = None "
                        "(network/RTW.py:178); RTW training is not defined")


class MAICMAC(SharedMAC):
    """SharedMAC over a MAICAgent (reference network/MAIC.py).  The reference ships the agent without a controller, so this
    class is the project's own, shaped like RTWMAC / SharedMACWithState.  Every pass is the agent unroll followed by the
    message head (csrc/maic_head.hip); ``head_over`` / ``head_backward`` are what MAICTDLearner trains through
    (MAICQLearner.train still raises).

    BatchNorm follows ``self.agent.training``.  ``self.agent.eval()``: running statistics, every environment on its own.
    Training mode (a freshly built agent; the reference never leaves it): the statistics of ALL rows of a head call and
    the running statistics move with every call, so the environments of a call are coupled - a batched rollout of E
    environments is NOT E serial rollouts, and ``get_current_q_values`` evaluates the head once per transition index t (the
    rows a reference-shaped loop would hand to one MAICAgent.forward call) instead of once for all t."""

    head_name = "MAIC"
    choose_action_inputs = "all"

    def _build_agents(self, input_shape):
        self.agent = MAICAgent(input_shape, self.args)
        self._step_q = None
        self._eps = None              # the batched rollout's noise buffer, kept per E

    def load_state(self, other_mac):
        """parameters as SharedMAC, plus the BatchNorm buffers (not part of the flat parameter buffer)"""
        SharedMAC.load_state(self, other_mac)
        src = dict(other_mac.agent.named_buffers())
        for k, b in self.agent.named_buffers():
            b.copy_(src[k])

    def choose_action(self, obs, last_action, agent_num, avail_actions, epsilon, evaluate=False):
        """One agent of one env, but ``obs`` (N, O), ``last_action`` (N, A) and ``avail_actions`` (N, A) cover EVERY agent
        (rollout.py passes them whole for this controller): agent j's Q values need the hidden state of every agent of the
        step.  The step is evaluated once, when agent 0 asks (test_mode = evaluate); agents 1 .. N-1 are served from it.
        Same numpy draw order as SharedMAC: one uniform per call, one choice only when exploring."""
        dev = self.device()
        N, A, O = self.n_agents, self.n_actions, self.obs_shape
        avail_all = np.asarray(avail_actions, dtype=np.float32).reshape(N, A)
        if agent_num == 0:
            obs_full = to_dev(np.asarray(obs, dtype=np.float32).reshape(1, 1, N, O), dev)
            ufed = torch.full((1, 1, N), -1, dtype=torch.int32, device=dev)
            if self.args.last_action:
                la = np.asarray(last_action, dtype=np.float32).reshape(N, A)
                idx = np.where(la.any(axis=1), la.argmax(axis=1), -1).astype(np.int32)
                ufed[0, 0] = to_dev(idx, dev, torch.int32)
            q, h_out = self._agent_step_one(obs_full, ufed)
            self._step_head(h_out, q, obs_full, avail_all, evaluate)
            self.hidden_states = h_out.view(1, N, -1)
            self._step_q = q.view(N, A).cpu()
        return self._draw(self._step_q[agent_num].clone(), avail_all[agent_num], epsilon)

    def _step_head(self, h_out, q, obs_full, avail, evaluate):
        self.agent.head(h_out, q.view(self.n_agents, self.n_actions), 1, bool(evaluate))

    def rollout_head(self, h, q, rec, t, E, evaluate, rseed, env):
        """q += the gated messages: choose_action for every agent of every environment; exploring, the latents' noise is
        the counter hash of (rseed, environment, global step)"""
        N, A = self.n_agents, self.n_actions
        eps = None
        if not evaluate:
            if self._eps is None or self._eps.shape[0] != E * N:
                self._eps = torch.empty(E * N, N * self.args.latent_dim, device=h.device)
            eps = self._eps
            ops.maic_noise(rseed, env.env0, env.global_step(t), eps, E, N)
        self.agent.head(h, q.view(E * N, A), E, bool(evaluate), eps)

    def head_over(self, hs, q, B, T, test_mode, eps):
        """q (B,T,N,A) += the gated messages from hs (B,T,N,64), in place.  ``self.agent.eval()``: one head call over all B*T*N
        rows.  Training mode: batch statistics are per call, so one call per transition index t over the B*N rows of that
        index (the running statistics move T times).  eps (B,T,N,N*latent_dim) or None."""
        N, A = self.n_agents, self.n_actions
        NL = N * self.args.latent_dim
        if not self.agent.training:
            self.agent.head(hs.view(B * T * N, -1), q.view(B * T * N, A), B * T, test_mode,
                            None if eps is None else eps.view(B * T * N, NL))
            return
        for t in range(T):
            qt = q[:, t].contiguous()
            self.agent.head(hs[:, t].contiguous().view(B * N, -1), qt.view(B * N, A), B, test_mode,
                            None if eps is None else eps[:, t].contiguous().view(B * N, NL))
            q[:, t] = qt

    def head_backward(self, hs, u_act, dq_val, B, T, test_mode, eps, dhs, buf, q=None, aux=None):
        """The backward counterpart of ``head_over``, over the same rows per call: dhs (B,T,N,64) is written with the head's
        contribution to the gradient on hs for the sparse pairs u_act, dq_val (B,T,N); the head's weight gradients
        accumulate into the agent's .grad views.
        ``aux`` = (mi_out, ent_out, den): the agent's MI and entropy losses as well (MAICAgent.aux_backward), over the same rows
        per call, with ``q`` (B,T,N,A) the Q values ``head_over`` returned.  The sum over the transition indices of the two
        losses is added into mi_out / ent_out (eval mode: the one call's losses times T - the same number, every index has B
        rows), the gradients are those of that sum times den[0] / T, and dhs carries both parts."""
        N, A = self.n_agents, self.n_actions
        NL = N * self.args.latent_dim
        H = hs.shape[-1]
        if not self.agent.training:
            R = B * T * N
            e = None if eps is None else eps.view(R, NL)
            plane = None
            if aux is not None:
                plane = buf.get("maic_aux_dpar", (R, 2 * NL), hs.device, hs.dtype)
                dh_aux = buf.get("maic_aux_dh", (R, H), hs.device, hs.dtype)
                self.agent.aux_backward(hs.view(R, H), q.view(R, A), B * T, test_mode, e, plane, dh_aux, aux[0], aux[1],
                                        den=aux[2], dscale=1.0 / T, weight_scale=float(T))
            self.agent.head_backward(hs.view(R, H), u_act.reshape(-1), dq_val.reshape(-1), B * T, test_mode, e, dhs.view(R, H),
                                     dpar_extra=plane)
            if aux is not None:
                dhs.view(R, H).add_(dh_aux)
            return
        # the rows of one index, made contiguous in scratch buffers (buf: the learner's Scratch) that every index uses again
        g = lambda name, src: buf.get("maic_bwd_" + name, (B, N) + tuple(src.shape[3:]), src.device, src.dtype)
        u_act, dq_val = u_act.view(B, T, N), dq_val.view(B, T, N)
        ht, ut, vt, dh = g("h", hs), g("u", u_act), g("v", dq_val), g("dh", dhs)
        et = None if eps is None else g("eps", eps)
        plane = None
        if aux is not None:
            qt, dh_aux = g("q", q), g("dh_aux", dhs)
            plane = buf.get("maic_aux_dpar", (B * N, 2 * NL), hs.device, hs.dtype)
        for t in range(T):
            ht.copy_(hs[:, t])
            ut.copy_(u_act[:, t])
            vt.copy_(dq_val[:, t])
            if et is not None:
                et.copy_(eps[:, t])
            e = None if et is None else et.view(B * N, NL)
            if aux is not None:
                qt.copy_(q[:, t])
                self.agent.aux_backward(ht.view(B * N, H), qt.view(B * N, A), B, test_mode, e, plane, dh_aux.view(B * N, H),
                                        aux[0], aux[1], den=aux[2], dscale=1.0 / T)
            self.agent.head_backward(ht.view(B * N, H), ut.view(-1), vt.view(-1), B, test_mode, e, dh.view(B * N, H),
                                     dpar_extra=plane)
            if aux is not None:
                dh.add_(dh_aux)
            dhs[:, t] = dh

    def _maic_q_values(self, batch, T, which, test_mode, eps):
        q, hs = self._batch_unroll(batch, T, which)
        B, N = q.shape[0], self.n_agents
        if eps is not None:
            eps = to_dev(eps, q.device).view(B, T, N, N * self.args.latent_dim)
        self.head_over(hs, q, B, T, test_mode, eps)
        return q, hs, {}

    def get_current_q_values(self, batch, max_episode_len, test_mode=False, eps=None):
        """(q (B,T,N,A) with the gated messages added, hs (B,T,N,H), {}): the unroll, then the head over all B*T*N rows.
        ``eps`` (B,T,N,N*latent_dim): the noise of the sampled latents (test_mode False); drawn with torch.randn if absent."""
        return self._maic_q_values(batch, max_episode_len, "cur", bool(test_mode), eps)

    def get_next_q_values(self, batch, max_episode_len, test_mode=False, eps=None):
        """as get_current_q_values on (o_next, u_onehot[t])"""
        return self._maic_q_values(batch, max_episode_len, "next", bool(test_mode), eps)
