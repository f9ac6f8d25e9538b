"""Thin Python wrappers over the C ABI: torch tensors in, raw device pointers out.

torch is used only for device memory and the stream handle (plumbing); every computation
below is a hand-written HIP kernel from marl_amd/csrc.
"""
from __future__ import annotations

import collections
import ctypes as C

import torch

from . import _lib
from ._lib import (MarlSrc, MarlGroup, MarlAgentWeights, MarlAgentGrads, MarlQmixWeights, MarlMlp3Weights,
                   MarlQtranWeights, MarlRtwWeights, MarlWorldWeights, MarlWorldGrads, MarlMaicWeights, MarlMaicGrads, MarlMaicInfer,
                   MarlMaicInferGrads, MarlCommnetWeights, MarlCommnetGrads, MarlG2anetWeights, MarlG2anetGrads, MarlRecord,
                   MarlMavenWeights, MarlMavenGrads, MarlMavenDisc, MarlMavenDiscGrads, check)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t):
    assert t.dtype == torch.float32 and t.is_cuda, "expected a CUDA float32 tensor"
    return t


def _i32(t):
    assert t.dtype == torch.int32 and t.is_cuda, "expected a CUDA int32 tensor"
    return t


def _dense_on_device(t, dtype=torch.float32, align=1):
    """t is a contiguous device tensor of `dtype` that starts on an `align`-byte boundary"""
    return t is not None and t.is_contiguous() and t.dtype == dtype and t.is_cuda and t.data_ptr() % align == 0


def _linear_fields(keys):
    return [(short + suf, name + key, torch.float32) for short, name in keys for suf, key in (("_w", ".weight"), ("_b", ".bias"))]


def _fill_struct(cls, tensors, fields):
    """cls() with every (field, tensor name, dtype) of `fields` set to the data pointer of tensors[name]"""
    w = cls()
    for field, name, dt in fields:
        t = tensors[name]
        assert _dense_on_device(t, dt), name
        setattr(w, field, t.data_ptr())
    w._keep = tensors
    return w


class Workspace:
    """Grow-only scratch buffers keyed by name (no allocation in steady state).  ``gen`` counts (re)allocations:
    a captured hipGraph holds raw pointers into these buffers, so its owner records ``gen`` at capture time, keeps
    ``snapshot()`` alive (the old storage cannot be freed and handed to somebody else under the graph) and drops
    the graph when ``gen`` has moved (algorithm/common.py:GraphedUpdate)."""

    def __init__(self):
        self.bufs = {}
        self.gen = 0

    def get(self, name, nbytes, device):
        n = (int(nbytes) + 3) // 4
        b = self.bufs.get(name)
        if b is None or b.numel() < n or b.device != device:
            b = torch.empty(max(n, 1), dtype=torch.float32, device=device)
            self.bufs[name] = b
            self.retire()
        return b

    def retire(self):
        """a buffer whose address a captured graph may hold has been replaced, here or in a hostutil.Scratch.get_flat"""
        self.gen += 1

    def snapshot(self):
        return list(self.bufs.values())


WS = Workspace()


class Rows:
    """A 2-D row source read through a row remap (rpe, bs, off) - e.g. the (T+1)-slot state storage - and
    optionally an int32 episode map (replay samples read in place from the ring)."""

    def __init__(self, t, remap, emap=None):
        self.t, self.remap, self.emap = t, remap, emap
        self.device = t.device


def src(x0=None, x1=None, idx=None, nhot=0, hot_w=0, nid=0, gate=None, remap0=None, remapi=None, k0=None, emap0=None):
    """Build a marl_src_t.  x0/x1: 2-D (rows, k) float32 views with unit inner stride (x0 may be Rows)."""
    s = MarlSrc()
    keep = []
    if isinstance(x0, Rows):
        x0, remap0, emap0 = x0.t, x0.remap, x0.emap
    if x0 is not None:
        _f32(x0); assert x0.dim() == 2 and x0.stride(1) == 1
        s.p0, s.ld0, s.k0 = x0.data_ptr(), x0.stride(0), (x0.shape[1] if k0 is None else k0)
        keep.append(x0)
    if x1 is not None:
        _f32(x1); assert x1.dim() == 2 and x1.stride(1) == 1
        s.p1, s.ld1, s.k1 = x1.data_ptr(), x1.stride(0), x1.shape[1]
        keep.append(x1)
    if idx is not None:
        _i32(idx)
        s.idx, s.nhot, s.hot_w = idx.data_ptr(), nhot, hot_w
        keep.append(idx)
    s.nid = nid
    if gate is not None:
        _f32(gate); assert gate.dim() == 2 and gate.stride(1) == 1
        s.m0, s.ldm0 = gate.data_ptr(), gate.stride(0)
        keep.append(gate)
    if remap0 is not None:
        s.rpe0, s.bs0, s.off0 = remap0
    if emap0 is not None:
        assert remap0 is not None and emap0.dtype == torch.int32 and emap0.is_contiguous()
        s.emap0 = emap0.data_ptr()
        keep.append(emap0)
    if remapi is not None:
        s.rpei, s.bsi, s.offi = remapi
    s._keep = keep
    return s


def agent_input_src(args, N, A, O, obs, remap0, ufed, remapi, emap):
    """the agent's virtual input rows [obs | one-hot(u_{t-1}) | agent id] (args.last_action / args.reuse_network permitting) as a
    row source: obs read through (remap0, emap), the fed action indices ufed through remapi"""
    kw = {}
    if args.last_action:
        kw.update(idx=ufed.reshape(-1, 1), nhot=1, hot_w=A, remapi=remapi)
    return src(obs.reshape(-1, O), nid=N if args.reuse_network else 0, remap0=remap0, emap0=emap, **kw)


def src_width(s):
    return s.k0 + s.k1 + s.nhot * s.hot_w + s.nid


def group(groups, x0=0, x1=0, w=0, b=0, y=0, m0=0):
    return MarlGroup(groups, x0, x1, w, b, y, m0)


def linear(x, W, bias, Y, M, N, K, act=0, beta=0.0, w_kmajor=False, ldw=None, grp=None, bf16=False):
    """Y[M,N] = act(X W^T + b) (+beta*Y).  W: (N,K) view, or (K,N) when w_kmajor.  bf16: round both operands to
    bf16 and use the bf16 matrix cores with fp32 accumulation (per call; the mixers pass their args.mixer_dtype)."""
    lib = _lib.load()
    if bf16:
        act |= 0x100
    if ldw is None:
        ldw = W.stride(0) if W.dim() == 2 else (N if w_kmajor else K)
    ldy = Y.stride(0) if Y.dim() == 2 else N
    assert src_width(x) == K, (src_width(x), K)
    check(lib.marl_linear(C.byref(x), _p(_f32(W)), ldw, 1 if w_kmajor else 0, _p(bias), _p(_f32(Y)), ldy,
                          M, N, K, act, float(beta), C.byref(grp) if grp is not None else None, _stream()),
          "marl_linear")


def linear_wgrad(dY, x, dW, db, M, N, K, Yact=None, grp=None, lddw=None, bf16=False):
    """dW[N,K] += (dY * (Yact>0))^T X ; db[N] += column sums."""
    lib = _lib.load()
    flags = 1 if bf16 else 0
    g = grp.groups if grp is not None else 1
    nbytes = lib.marl_linear_wgrad_workspace(M, N, K, g)
    ws = WS.get("wgrad", nbytes, dY.device)
    if lddw is None:
        lddw = dW.stride(0) if dW.dim() == 2 else K
    assert src_width(x) == K, (src_width(x), K)
    check(lib.marl_linear_wgrad(_p(_f32(dY)), dY.stride(0) if dY.dim() == 2 else N,
                                _p(Yact), (Yact.stride(0) if Yact.dim() == 2 else N) if Yact is not None else 0,
                                C.byref(x), _p(_f32(dW)), lddw, _p(db), M, N, K, flags,
                                C.byref(grp) if grp is not None else None, _p(ws), ws.numel() * 4, _stream()),
          "marl_linear_wgrad")


LINEAR_PATHS = ("element", "vector", "dword")                                     # plan[0] of marl_linear_plan (include/marl_hip.h)
WGRAD_FAMILIES = ("generic", "full", "direct", "passes", "tall", "thin")          # plan[0] of marl_linear_wgrad_plan
LinearPlan = collections.namedtuple("LinearPlan", "path tiles gate kmajor bf16 wvec grid")
WgradPlan = collections.namedtuple("WgradPlan", "family inst passes slabs gvec xvec c_rest")


def _pv(t):
    """a pointer argument of a plan query: a tensor, an integer standing for a pointer (only its alignment is read) or None"""
    if t is None:
        return None
    return C.c_void_p(int(t) if isinstance(t, int) else t.data_ptr())


def linear_plan(x, W, ldw, ldy, M, N, K, act=0, w_kmajor=False, grp=None, bf16=False, bias=None):
    """The launch plan of linear() for these arguments, from the host function the launch itself decides with - no GPU:
    LinearPlan(path in LINEAR_PATHS, column tiles, gate, kmajor, bf16, wvec, grid), or None where marl_linear refuses the call.
    x: a MarlSrc; W / bias: tensors or integers standing for pointers."""
    plan = (C.c_int * 9)()
    if _lib.load().marl_linear_plan(C.byref(x), _pv(W), ldw, 1 if w_kmajor else 0, _pv(bias), ldy, M, N, K, act | (0x100 if bf16 else 0),
                                    C.byref(grp) if grp is not None else None, plan) != 0:
        return None
    p = tuple(plan)
    return LinearPlan(LINEAR_PATHS[p[0]], p[1], bool(p[2]), bool(p[3]), bool(p[4]), bool(p[5]), p[6:9])


def linear_wgrad_plan(dY, lddy, x, M, N, K, Yact=None, ldya=0, grp=None, bf16=False, ws_bytes=None):
    """The launch plan of linear_wgrad(): WgradPlan(family in WGRAD_FAMILIES, (instantiation), passes, slabs per pass, gvec, xvec,
    c_rest), or None where marl_linear_wgrad refuses the call.  ws_bytes None: what linear_wgrad() would pass now - the shared
    grow-only buffer, grown to this call's need."""
    lib = _lib.load()
    if ws_bytes is None:
        ws_bytes = lib.marl_linear_wgrad_workspace(M, N, K, grp.groups if grp is not None else 1)
        have = WS.bufs.get("wgrad")
        if have is not None:
            ws_bytes = max((ws_bytes + 3) // 4 * 4, have.numel() * 4)
    plan = (C.c_int * 8)()
    if lib.marl_linear_wgrad_plan(_pv(dY), lddy, _pv(Yact), ldya, C.byref(x), M, N, K, 1 if bf16 else 0,
                                  C.byref(grp) if grp is not None else None, ws_bytes, plan) != 0:
        return None
    p = tuple(plan)
    return WgradPlan(WGRAD_FAMILIES[p[0]], (p[1], p[2]), p[3], p[4], bool(p[5]), bool(p[6]), p[7])


_AGENT_FIELDS = _linear_fields((("fc1", "fc1"), ("fc2", "fc2"))) + [
    (field, "rnn." + name, torch.float32) for field, name in (("w_ih", "weight_ih"), ("w_hh", "weight_hh"), ("b_ih", "bias_ih"), ("b_hh", "bias_hh"))]


def agent_weights(params):
    """params: dict name -> tensor with RNNQNet keys."""
    w = _fill_struct(MarlAgentWeights, params, _AGENT_FIELDS)
    w.H = params["rnn.weight_hh"].shape[1]
    return w


def agent_unroll_fwd(w, obs, obs_bs, obs_t0, ufed, u_bs, u_t0, h0, q, hs, h_last, saved,
                     B, T, N, O, A, last_action=True, reuse_network=True, ep_len=None, ep_map=None, cu_budget=0, gi_out=None,
                     gi_in=None):
    """cu_budget: CUs (= workgroups) a T > 1 launch spreads its rows over (0 / 256 = the whole chip); 128 lets two
    independent unrolls run side by side on two streams (PairedUnroll).  A per-call argument, no process state.
    gi_out / gi_in: (T, B*N, 3, 64) buffer of input-side gate sums written by one unroll and read by a later unroll of the
    same weights whose step t input is the earlier one's step t+1 input (include/marl_hip.h)."""
    lib = _lib.load()
    check(lib.marl_agent_unroll_fwd(C.byref(w), _p(_f32(obs)), obs_bs, obs_t0, _p(ufed), u_bs, u_t0, _p(ep_len),
                                    _p(_i32(ep_map)) if ep_map is not None else None, _p(h0),
                                    _p(_f32(q)), _p(hs), _p(h_last), _p(saved), B, T, N, O, A,
                                    1 if last_action else 0, 1 if reuse_network else 0, int(cu_budget),
                                    _p(_f32(gi_out)) if gi_out is not None else None,
                                    _p(_f32(gi_in)) if gi_in is not None else None, _stream()),
          "marl_agent_unroll_fwd")


def agent_unroll_x6_supported(B, T, N, O, A, last_action=True, reuse_network=True):
    return bool(_lib.load().marl_agent_unroll_x6_supported(B, T, N, O, A, 1 if last_action else 0, 1 if reuse_network else 0))


def agent_unroll_x6_plain_r6(B, T, N, O, A, last_action=True, reuse_network=True, cu_budget=0):
    """a non-saving split unroll of this batch runs on csrc/agent_x6p.hip (the round-6 decomposition): no gate sums are kept for it"""
    return bool(_lib.load().marl_agent_unroll_x6_plain_r6(B, T, N, O, A, 1 if last_action else 0, 1 if reuse_network else 0, int(cu_budget)))


def agent_unroll_fwd_x6(w, obs, obs_bs, obs_t0, ufed, u_bs, u_t0, h0, q, hs, h_last, saved, B, T, N, O, A, last_action=True,
                        reuse_network=True, ep_len=None, ep_map=None, cu_budget=0, gi_out=None, gi_in=None):
    """the unroll on the bf16x6 split kernels (csrc/agent_x6.hip; opt-in args.gemm_mode = "bf16x6"): same arguments as
    agent_unroll_fwd, same `saved` layout (the fp32 BPTT kernel reads it); gi_out / gi_in hold plain sums here, so a storing and a
    reading launch must both be this one"""
    if saved is None and gi_in is None and hs is None and agent_unroll_x6_plain_r6(B, T, N, O, A, last_action, reuse_network, cu_budget):
        # csrc/agent_x6p.hip addresses the observations and the fed actions with 32-bit byte offsets against a uniform base
        assert obs.numel() < 2 ** 30 and (ufed is None or ufed.numel() < 2 ** 30), "observation storage beyond 4 GB: set MARL_UNROLL_R6=0"
    check(_lib.load().marl_agent_unroll_fwd_x6(C.byref(w), _p(_f32(obs)), obs_bs, obs_t0, _p(ufed), u_bs, u_t0, _p(ep_len),
                                               _p(_i32(ep_map)) if ep_map is not None else None, _p(h0), _p(_f32(q)), _p(hs),
                                               _p(h_last), _p(saved), B, T, N, O, A, 1 if last_action else 0,
                                               1 if reuse_network else 0, int(cu_budget),
                                               _p(_f32(gi_out)) if gi_out is not None else None,
                                               _p(_f32(gi_in)) if gi_in is not None else None, _stream()),
          "marl_agent_unroll_fwd_x6")


UNROLL_FAMILIES = ("f32-pipe", "f32-multi", "x6", "x6-r6")          # plan[0] of marl_agent_unroll_fwd_plan (include/marl_hip.h)
UNROLL_INPUT_PATHS = ("element", "vector", "half", "w2l")            # plan[6]


def agent_unroll_fwd_plan(x6, B, T, N, O, A, last_action=True, reuse_network=True, cu_budget=0, saved=False, gi_out=False,
                          gi_in=False, hs=True, obs_aligned=True, h_aligned=True):
    """The launch plan of agent_unroll_fwd (x6 False) / agent_unroll_fwd_x6 (x6 True), from the host function the launch itself
    calls - no GPU: (family, row tiles per workgroup, workgroups, workgroups holding that many tiles, action tiles, fc1 chunks,
    input path, reads gi_in), or None where the entry point refuses the call.  The keywords say what the caller would pass."""
    flags = (1 if saved else 0) | (2 if gi_out else 0) | (4 if gi_in else 0) | (8 if hs else 0) | (16 if obs_aligned else 0) | (32 if h_aligned else 0)
    plan = (C.c_int * 8)()
    if _lib.load().marl_agent_unroll_fwd_plan(1 if x6 else 0, B, T, N, O, A, 1 if last_action else 0, 1 if reuse_network else 0,
                                              int(cu_budget), flags, plan) != 0:
        return None
    return tuple(plan)


def saved_shape(T, B, N, planes=6, H=64):
    """Shape of the activation buffer an unroll saves for BPTT (planes = 6) or of its input-side gate sums (planes = 3):
    the kernels use a tile layout [T][16-row tile][plane][column tile][lane][4] (csrc/agent.hip: sv_off), so the row count is
    rounded up to whole tiles.  The buffer is opaque to the host; `saved_plane` decodes one plane."""
    return (T + (1 if planes == 6 else 0), (B * N + 15) // 16 * 16, planes, H)     # (+ the hidden state after the last step)


def saved_plane(saved, plane, rows):
    """(T, rows, 64) view-copy of one plane of a buffer in the tile layout (tests / debugging)."""
    T, R16, P, H = saved.shape
    t = saved.reshape(T, R16 // 16, P, 4, 4, 16, 4)[:, :, plane]          # (T, tile, c, q, m, i)
    return t.permute(0, 1, 3, 5, 2, 4).reshape(T, R16, H)[:, :rows]       # row = 16 tile + 4 q + i ; column = 16 c + m  (T+1 slabs for 6 planes)


def agent_unroll_reuse_supported(B, T, N, O, A, cu_budget=0):
    return bool(_lib.load().marl_agent_unroll_reuse_supported(B, T, N, O, A, int(cu_budget)))


def agent_unroll_bwd_x6_supported(B, T, N, A, sparse_dq=True):
    return bool(_lib.load().marl_agent_unroll_bwd_x6_supported(B, T, N, A, 1 if sparse_dq else 0))


def agent_unroll_bwd(w, dq, dhs, saved, hs, dxp, dh0, grads, B, T, N, A, dq_idx=None, dq_val=None, dq_idx2=None,
                     dq_val2=None, dq_gdiv=1, x6=False):
    """grads: dict name -> gradient tensor for rnn.weight_ih/hh, rnn.bias_ih/hh, fc2.weight/bias (accumulated)."""
    lib = _lib.load()
    g = MarlAgentGrads()
    g.w_ih, g.w_hh = grads["rnn.weight_ih"].data_ptr(), grads["rnn.weight_hh"].data_ptr()
    g.b_ih, g.b_hh = grads["rnn.bias_ih"].data_ptr(), grads["rnn.bias_hh"].data_ptr()
    g.fc2_w, g.fc2_b = grads["fc2.weight"].data_ptr(), grads["fc2.bias"].data_ptr()
    for v in grads.values():
        assert v.is_contiguous() and v.dtype == torch.float32 and v.is_cuda
    if x6:      # the split kernels (csrc/agent_bwd_x6.hip; opt-in args.gemm_mode = "bf16x6"): sparse dq only
        assert dq is None and dq_idx is not None and dq_val is not None and dq_idx.is_contiguous() and dq_val.is_contiguous()
        _i32(dq_idx); _f32(dq_val)
        if dq_idx2 is not None:
            assert dq_val2 is not None and dq_idx2.is_contiguous() and dq_val2.is_contiguous()
            _i32(dq_idx2); _f32(dq_val2)
        ws = WS.get("agent_bwd_x6", lib.marl_agent_bwd_x6_workspace(B, N, A), saved.device)
        check(lib.marl_agent_unroll_bwd_x6(C.byref(w), _p(dq_idx), _p(dq_val), _p(dq_idx2), _p(dq_val2), int(dq_gdiv), _p(dhs),
                                           _p(_f32(saved)), _p(_f32(dxp)), _p(dh0), C.byref(g), _p(ws), ws.numel() * 4, B, T, N, A,
                                           _stream()), "marl_agent_unroll_bwd_x6")
        return
    ws = WS.get("agent_bwd", lib.marl_agent_bwd_workspace(B, N, A), saved.device)
    if dq_idx is not None:
        assert dq is None and dq_val is not None and dq_idx.is_contiguous() and dq_val.is_contiguous()
        _i32(dq_idx); _f32(dq_val)
    if dq_idx2 is not None:
        assert dq_idx is not None and dq_val2 is not None and dq_idx2.is_contiguous() and dq_val2.is_contiguous()
        _i32(dq_idx2); _f32(dq_val2)
    check(lib.marl_agent_unroll_bwd(C.byref(w), _p(_f32(dq)) if dq is not None else None, _p(dq_idx), _p(dq_val),
                                    _p(dq_idx2), _p(dq_val2), int(dq_gdiv), _p(dhs),
                                    _p(_f32(saved)), _p(hs), _p(_f32(dxp)),
                                    _p(dh0), C.byref(g), _p(ws), ws.numel() * 4, B, T, N, A, _stream()),
          "marl_agent_unroll_bwd")


def q_gather(q, idx, out, rows, A, avail=None, mask_val=0.0):
    check(_lib.load().marl_q_gather(_p(_f32(q)), _p(_i32(idx)), _p(avail), float(mask_val), _p(_f32(out)), rows, A,
                                    _stream()), "marl_q_gather")


def q_masked_max(q, avail, mask_val, out_max, out_arg, rows, A):
    check(_lib.load().marl_q_masked_max(_p(_f32(q)), _p(avail), float(mask_val), _p(out_max), _p(out_arg), rows, A,
                                        _stream()), "marl_q_masked_max")


def q_double_select(q_sel, q_val, avail, mask_val, out_val, out_arg, rows, A):
    check(_lib.load().marl_q_double_select(_p(_f32(q_sel)), _p(_f32(q_val)), _p(avail), float(mask_val), _p(_f32(out_val)),
                                           _p(out_arg), rows, A, _stream()), "marl_q_double_select")


def q_scatter(dq, idx1, g1, idx2, g2, rows, A, gdiv=1):
    check(_lib.load().marl_q_scatter(_p(_f32(dq)), _p(idx1), _p(g1), _p(idx2), _p(g2), rows, A, gdiv, _stream()),
          "marl_q_scatter")


def vec_add(a, b, out, n):
    check(_lib.load().marl_vec_add(_p(_f32(a)), _p(_f32(b)), _p(_f32(out)), n, _stream()), "marl_vec_add")


def _ld(t, D):
    """row stride of a (rows, D) view (padded intermediates), D for flat / differently shaped tensors"""
    return t.stride(0) if (t.dim() == 2 and t.shape[1] == D and t.stride(1) == 1) else D


def agent_sum(inp, out, rows, N, D):
    check(_lib.load().marl_agent_sum(_p(_f32(inp)), _ld(inp, D), _p(_f32(out)), _ld(out, D), rows, N, D, _stream()),
          "marl_agent_sum")


def agent_bcast(inp, out, rows, N, D, accumulate=False):
    check(_lib.load().marl_agent_bcast(_p(_f32(inp)), _ld(inp, D), _p(_f32(out)), _ld(out, D), rows, N, D,
                                       1 if accumulate else 0, _stream()), "marl_agent_bcast")


def qmix_mix_fwd(hy, b2, q, q_tot, rows, N, E, w22=None, b22=None):
    """b2 None: formed in the kernel from hy's relu'd fourth block with hyper_b2.2's weight w22 (E) and bias b22 (1)"""
    check(_lib.load().marl_qmix_mix_fwd(_p(_f32(hy)), hy.stride(0), _p(b2), _p(w22), _p(b22), _p(_f32(q)), _p(_f32(q_tot)), rows,
                                        N, E, _stream()), "marl_qmix_mix_fwd")


def qmix_mix_bwd(hy, q, dq_tot, dhy, db2, dq, rows, N, E, w22=None):
    """w22 given: the fourth block of dhy (d hb through hyper_b2.2 and the relu) is written here too"""
    assert dhy.stride(0) == hy.stride(0)
    check(_lib.load().marl_qmix_mix_bwd(_p(_f32(hy)), hy.stride(0), _p(_f32(q)), _p(_f32(dq_tot)), _p(w22), _p(_f32(dhy)),
                                        _p(_f32(db2)), _p(_f32(dq)), rows, N, E, _stream()), "marl_qmix_mix_bwd")


def qmix_tail_supported(S, E, s):
    return E == 32 and qtran_state_parts_supported(S, s)


def qmix_tail_fwd(s, rows, S, b1_w, b1_b, h_w, h_b, hy, c_b1, c_h):
    """hy[:, c_b1:c_b1+32] = hyper_b1(s), hy[:, c_h:c_h+32] = relu(hyper_b2.0(s)) in one pass over s (Rows or dense)"""
    assert b1_w.stride(1) == 1 and h_w.stride(1) == 1 and b1_w.stride(0) == h_w.stride(0) and hy.stride(1) == 1
    x = src(s)
    check(_lib.load().marl_qmix_tail_fwd(C.byref(x), rows, S, _p(_f32(b1_w)), b1_w.stride(0), _p(_f32(b1_b)), _p(_f32(h_w)),
                                         h_w.stride(0), _p(_f32(h_b)), _p(_f32(hy)), hy.stride(0), c_b1, c_h, _stream()),
          "marl_qmix_tail_fwd")


def qplex_mix_fwd(w_raw, v, q, max_q, key, ag, ac, v_tot, a_tot, lam_out, rows, N, K, weighted, minus_one):
    check(_lib.load().marl_qplex_mix_fwd(_p(w_raw), _p(v), _p(q), _p(max_q), _p(key), _p(ag), _p(ac), _p(v_tot),
                                         _p(a_tot), _p(lam_out), rows, N, K, int(weighted), int(minus_one), _stream()),
          "marl_qplex_mix_fwd")


def qplex_mix_bwd(w_raw, q, max_q, key, ag, ac, g, dq, dw_raw, dv, dkey, dag, dac, rows, N, K, weighted, minus_one):
    check(_lib.load().marl_qplex_mix_bwd(_p(w_raw), _p(q), _p(max_q), _p(key), _p(ag), _p(ac), _p(g), _p(dq),
                                         _p(dw_raw), _p(dv), _p(dkey), _p(dag), _p(dac), rows, N, K, int(weighted),
                                         int(minus_one), _stream()), "marl_qplex_mix_bwd")


def qatten_supported(s, N, U, H):
    """csrc/qatten.hip covers the shape (N <= 16, U <= 64, H <= 8) and the source s (a marl_src_t, Rows or a dense 2-D tensor)"""
    x = s if isinstance(s, MarlSrc) else src(s)
    return bool(_lib.load().marl_qatten_supported(C.byref(x), N, U, H))


def qatten_plan(rows, N, U, H):
    """(rows of a workgroup's tile, workgroups, LDS bytes, tiles the busiest workgroup walks) of the Qatten row kernel"""
    plan = (C.c_int * 4)()
    check(_lib.load().marl_qatten_plan(rows, N, U, H, plan), "marl_qatten_plan")
    return tuple(plan)


def qatten_mix_fwd(s, hy, q, scale, q_tot, rows, N, U, H):
    """q_tot of the Qatten mixer; hy (rows, >= H U + H + 1): [p | w_raw | c] per row, s: the states (marl_src_t)"""
    check(_lib.load().marl_qatten_mix_fwd(C.byref(s), _p(_f32(hy)), hy.stride(0), _p(_f32(q)), float(scale), _p(_f32(q_tot)), rows,
                                          N, U, H, _stream()), "marl_qatten_mix_fwd")


def qatten_mix_bwd(s, hy, q, scale, dq_tot, dq, dhy, rows, N, U, H):
    """dq (rows, N) and dhy (rows, >= H U + H): [dp | dw_raw] per row, from dq_tot; the softmax weights are recomputed"""
    check(_lib.load().marl_qatten_mix_bwd(C.byref(s), _p(_f32(hy)), hy.stride(0), _p(_f32(q)), float(scale), _p(_f32(dq_tot)),
                                          _p(_f32(dq)), _p(_f32(dhy)), dhy.stride(0), rows, N, U, H, _stream()), "marl_qatten_mix_bwd")


def qatten_loss_bwd(s, hy, q, scale, q_tot_tgt, r, term, padded, gamma, q_tot, dq, dhy, dq_tot, out2, rows, N, U, H):
    """Qatten forward + TD loss + backward in one launch (include/marl_hip.h); out2: 2-element device view written,
    q_tot optional"""
    lib = _lib.load()
    ws = WS.get("loss", lib.marl_loss_workspace(rows), q.device)
    check(lib.marl_qatten_loss_bwd(C.byref(s), _p(_f32(hy)), hy.stride(0), _p(_f32(q)), float(scale), _p(_f32(q_tot_tgt)),
                                   _p(_f32(r)), _p(_f32(term)), _p(_f32(padded)), float(gamma), _p(q_tot), _p(_f32(dq)),
                                   _p(_f32(dhy)), dhy.stride(0), _p(_f32(dq_tot)), _p(_f32(out2)), _p(ws), rows, N, U, H, _stream()),
          "marl_qatten_loss_bwd")


def lica_supported(N, A, E):
    """csrc/lica.hip covers the shape: N <= 16, A <= 32, E <= 64"""
    return bool(_lib.load().marl_lica_supported(N, A, E))


def lica_plan(rows, N, A, E):
    """(rows of a workgroup's tile, workgroups, LDS bytes, tiles the busiest workgroup walks) of the LICA row kernel"""
    plan = (C.c_int * 4)()
    check(_lib.load().marl_lica_plan(rows, N, A, E, plan), "marl_lica_plan")
    return tuple(plan)


def _lica_in(x, u):
    return _p(None if x is None else _f32(x)), _p(None if u is None else _i32(u))


def lica_mix_fwd(hy, x, u, q, rows, N, A, E):
    """Q (rows) of LICA's mixing critic; hy (rows, >= K E + 2 E + 1): [W1 | b1 | wf | b2] per row; the input is dense x (rows, K) or
    the taken actions u (rows N) int32 - exactly one of them, the other None"""
    px, pu = _lica_in(x, u)
    check(_lib.load().marl_lica_mix_fwd(_p(_f32(hy)), hy.stride(0), px, pu, _p(_f32(q)), rows, N, A, E, _stream()), "marl_lica_mix_fwd")


def lica_mix_bwd(hy, x, u, dq, dhy, dx, rows, N, A, E):
    """dhy (rows, >= K E + 2 E): [dW1 | db1 | dwf] per row and dx (rows, K) from dq (rows); either output may be None, not both"""
    px, pu = _lica_in(x, u)
    check(_lib.load().marl_lica_mix_bwd(_p(_f32(hy)), hy.stride(0), px, pu, _p(_f32(dq)), _p(None if dhy is None else _f32(dhy)),
                                        0 if dhy is None else dhy.stride(0), _p(None if dx is None else _f32(dx)), rows, N, A, E,
                                        _stream()), "marl_lica_mix_bwd")


def lica_loss_bwd(hy, u, q_tgt, r, term, padded, gamma, q, dhy, dq_tot, out2, rows, N, A, E):
    """LICA's critic on the taken actions + TD loss + backward to dhy in one row launch (include/marl_hip.h); out2: 2-element
    device view written"""
    lib = _lib.load()
    ws = WS.get("loss", lib.marl_loss_workspace(rows), hy.device)
    check(lib.marl_lica_loss_bwd(_p(_f32(hy)), hy.stride(0), _p(_i32(u)), _p(_f32(q_tgt)), _p(_f32(r)), _p(_f32(term)),
                                 _p(_f32(padded)), float(gamma), _p(_f32(q)), _p(_f32(dhy)), dhy.stride(0), _p(_f32(dq_tot)),
                                 _p(_f32(out2)), _p(ws), rows, N, A, E, _stream()), "marl_lica_loss_bwd")


# ---- MAVEN (csrc/maven.hip): the episode noise, the noise-conditioned agent head, the MI pass
MAVEN_TABLES = ("noise_w", "id_w", "noise_b", "id_b")
MAVEN_DISC = (("w1", "l1.weight"), ("b1", "l1.bias"), ("w2", "l2.weight"), ("b2", "l2.bias"))


def maven_supported(N, A, K, S, D=64):
    """csrc/maven.hip covers the shape: N <= 16, A <= 32, K <= 32, D = 64 and N A + S within a 16-step tile of x in LDS"""
    return bool(_lib.load().marl_maven_supported(int(N), int(A), int(K), int(S), int(D)))


def maven_plan(B, T, N, A, K, S):
    """(head tiles per (episode, agent), head forward workgroups, head backward slabs, MI tiles, MI workgroups = slabs, MI LDS bytes,
    tiles the busiest MI workgroup walks, LDS pitch of x) - include/marl_hip.h: marl_maven_plan"""
    plan = (C.c_int * 8)()
    check(_lib.load().marl_maven_plan(int(B), int(T), int(N), int(A), int(K), int(S), plan), "marl_maven_plan")
    return tuple(plan)


def maven_weights(tensors, prefix="maven."):
    """tensors: dict name -> tensor holding <prefix>noise_w (K,A,64), id_w (N,A,64), noise_b (K,A), id_b (N,A) -> marl_maven_weights_t"""
    return _fill_struct(MarlMavenWeights, tensors, [(f, prefix + f, torch.float32) for f in MAVEN_TABLES])


def maven_grads(grads, prefix="maven."):
    """the gradient destinations of the same four tables -> marl_maven_grads_t"""
    return _fill_struct(MarlMavenGrads, grads, [(f, prefix + f, torch.float32) for f in MAVEN_TABLES])


def maven_disc(tensors):
    """tensors: dict with l1.weight (64, N A + S), l1.bias, l2.weight (K, 64), l2.bias -> marl_maven_disc_t"""
    return _fill_struct(MarlMavenDisc, tensors, [(f, name, torch.float32) for f, name in MAVEN_DISC])


def maven_disc_grads(grads):
    return _fill_struct(MarlMavenDiscGrads, grads, [(f, name, torch.float32) for f, name in MAVEN_DISC])


def maven_noise(rseed, env0, tg0, K, noise, E):
    """noise (E,) int32 <- hkey(rseed, stream 24, env0 + e, tg0, 0) % K"""
    assert _i32(noise).is_contiguous() and noise.numel() >= E
    check(_lib.load().marl_maven_noise(int(rseed) & 0xFFFFFFFF, int(env0), int(tg0) & 0xFFFFFFFF, int(K), _p(noise), int(E), _stream()),
          "marl_maven_noise")


def maven_head_fwd(w, hs, noise, q, B, T, N, A, K):
    """q (B,T,N,A) += (noise_w[k_b] + id_w[n]) h + noise_b[k_b] + id_b[n] from hs (B,T,N,64) and noise (B,) int32; an episode whose
    index is outside [0, K) is left alone"""
    assert hs.is_contiguous() and q.is_contiguous() and hs.numel() >= B * T * N * 64 and q.numel() >= B * T * N * A
    assert _i32(noise).is_contiguous() and noise.numel() >= B
    check(_lib.load().marl_maven_head_fwd(C.byref(w), _p(_f32(hs)), _p(noise), _p(_f32(q)), int(B), int(T), int(N), int(A), int(K),
                                          _stream()), "marl_maven_head_fwd")


def maven_head_bwd(w, g, hs, noise, dq_idx, dq_val, dq_dense, dq_out, dhs, B, T, N, A, K):
    """dq_out (B,T,N,A) = scatter(dq_idx, dq_val) + dq_dense (either may be None) and dhs (B,T,N,64) written; the four table
    gradients added into g (slabs of episodes, summed in slab order)"""
    lib = _lib.load()
    R = B * T * N
    assert hs.is_contiguous() and dq_out.is_contiguous() and dhs.is_contiguous() and dq_out.numel() >= R * A and dhs.numel() >= R * 64
    assert _i32(noise).is_contiguous() and noise.numel() >= B
    assert (dq_idx is None) == (dq_val is None)
    if dq_idx is not None:
        assert _i32(dq_idx).is_contiguous() and _f32(dq_val).is_contiguous() and dq_idx.numel() >= R and dq_val.numel() >= R
    if dq_dense is not None:
        assert _f32(dq_dense).is_contiguous() and dq_dense.numel() >= R * A
    ws = WS.get("maven_bwd", lib.marl_maven_bwd_workspace(int(B), int(N), int(A), int(K)), hs.device)
    check(lib.marl_maven_head_bwd(C.byref(w), C.byref(g), _p(_f32(hs)), _p(noise), _p(dq_idx), _p(dq_val), _p(dq_dense),
                                  _p(_f32(dq_out)), _p(_f32(dhs)), _p(ws), ws.numel() * 4, int(B), int(T), int(N), int(A), int(K),
                                  _stream()), "marl_maven_head_bwd")


def maven_mi(d, g, q, avail, avail_bs, state, state_ld, state_bs, ep_map, noise, padded, lambda_mi, dq_dense, ce, stats2,
             B, T, N, A, S, K):
    """The MI pass over the B T steps (include/marl_hip.h: marl_maven_mi): stats2 += {sum m ce, sum m hit}, the discriminator's
    gradients added into g, dq_dense (B,T,N,A) and ce (B T) written.  avail / state are read in place: episode b lies at
    ep_map[b] (None: b) with strides avail_bs (floats per episode) and state_bs (rows per episode) x state_ld (floats per row)"""
    lib = _lib.load()
    assert q.is_contiguous() and dq_dense.is_contiguous() and dq_dense.numel() >= B * T * N * A and ce.numel() >= B * T
    assert _i32(noise).is_contiguous() and noise.numel() >= B and _f32(padded).is_contiguous() and padded.numel() >= B * T
    assert ep_map is None or (_i32(ep_map).is_contiguous() and ep_map.numel() >= B)
    assert stats2.numel() == 2 and stats2.is_contiguous()
    ws = WS.get("maven_mi", lib.marl_maven_mi_workspace(int(B) * int(T), int(N), int(A), int(K), int(S)), q.device)
    check(lib.marl_maven_mi(C.byref(d), C.byref(g), _p(_f32(q)), _p(_f32(avail)), int(avail_bs), _p(_f32(state)), int(state_ld),
                            int(state_bs), _p(ep_map), _p(noise), _p(padded), float(lambda_mi), _p(_f32(dq_dense)), _p(_f32(ce)),
                            _p(_f32(stats2)), _p(ws), ws.numel() * 4, int(B), int(T), int(N), int(A), int(S), int(K), _stream()),
          "marl_maven_mi")


_FT_OUT = {}


def replay_gather(idx, src, out):
    """src / out: objects with u, r, term, padded, length, won (+ src.avail, out.o_map, out.u_act, out.avail_next and, when the
    learner masks current-step actions, out.avail_cur)."""
    assert idx.dtype == torch.int64 and idx.is_cuda and idx.is_contiguous()
    B, T, N, A = int(idx.numel()), src.T, src.N, src.A
    for t in (src.u, src.r, src.term, src.padded, src.length, src.won, src.avail, out.u, out.u_act, out.r, out.term, out.padded,
              out.length, out.won, out.avail_next, out.o_map):
        assert t.is_cuda and t.is_contiguous()
    assert src.u.dtype == torch.int32 and src.length.dtype == torch.int32 and src.won.dtype == torch.int32
    check(_lib.load().marl_replay_gather(_p(idx), B, T, N, A, _p(src.u), _p(_f32(src.r)), _p(_f32(src.term)), _p(_f32(src.padded)),
                                         _p(src.length), _p(src.won), _p(_f32(src.avail)), _p(_i32(out.o_map)), _p(_i32(out.u)),
                                         _p(_i32(out.u_act)), _p(_f32(out.r)), _p(_f32(out.term)), _p(_f32(out.padded)),
                                         _p(_i32(out.length)), _p(_i32(out.won)), _p(_f32(out.avail_next)),
                                         _p(getattr(out, "avail_cur", None)), _stream()),
          "marl_replay_gather")


def first_terminated_len(term, T):
    """max over episodes of (first terminated step + 1) within the first T steps as a 1-element int32 device tensor
    (0 = no episode terminates).  term: (E, >=T[, 1]) CUDA float32 with unit inner stride."""
    t2 = term.reshape(term.shape[0], -1)
    assert t2.dtype == torch.float32 and t2.is_cuda and t2.stride(1) == 1
    ring = _FT_OUT.get(t2.device)
    if ring is None:         # a ring of output words: an asynchronous read-back of one call may still be pending at the next
        ring = _FT_OUT[t2.device] = [torch.zeros(8, dtype=torch.int32, device=t2.device), 0]
    out = ring[0][ring[1] % 8:ring[1] % 8 + 1]
    ring[1] += 1
    check(_lib.load().marl_first_terminated_len(_p(t2), t2.stride(0), t2.shape[0], min(T, t2.shape[1]), _p(out), _stream()),
          "marl_first_terminated_len")
    return out


def td_loss(q_tot, q_tgt, r, term, padded, gamma, dq_tot, out2, rows):
    lib = _lib.load()
    ws = WS.get("loss", lib.marl_loss_workspace(rows), q_tot.device)
    check(lib.marl_td_loss(_p(_f32(q_tot)), _p(_f32(q_tgt)), _p(_f32(r)), _p(_f32(term)), _p(_f32(padded)),
                           float(gamma), _p(_f32(dq_tot)), _p(_f32(out2)), _p(ws), rows, _stream()), "marl_td_loss")


def qtran_loss(jq, jq_tgt, v, jq_hat, qs_opt, qs_nopt, r, term, padded, gamma, lam_opt, lam_nopt,
               d_jq, d_v, d_qso, d_qsn, out4, rows):
    lib = _lib.load()
    ws = WS.get("loss", lib.marl_loss_workspace(rows), jq.device)
    check(lib.marl_qtran_loss(_p(jq), _p(jq_tgt), _p(v), _p(jq_hat), _p(qs_opt), _p(qs_nopt), _p(r), _p(term),
                              _p(padded), float(gamma), float(lam_opt), float(lam_nopt), _p(d_jq), _p(d_v), _p(d_qso),
                              _p(d_qsn), _p(out4), _p(ws), rows, _stream()), "marl_qtran_loss")


def td_lambda_returns(q_next_tot, r, term, padded, gamma, lam, out, B, T):
    """TD(lambda) returns of B episodes over T steps (csrc/td_lambda.hip; reference utils/rl_utils.py:4-14 with the terminal
    flag masked by the padding).  All arrays hold B*T contiguous floats; ``out`` may not alias an input."""
    lib = _lib.load()
    for t in (q_next_tot, r, term, padded, out):
        assert _f32(t).is_contiguous() and t.numel() >= B * T, "td_lambda_returns: contiguous (B, T) float32 arrays"
    check(lib.marl_td_lambda_returns(_p(q_next_tot), _p(r), _p(term), _p(padded), float(gamma), float(lam), _p(out),
                                     int(B), int(T), _stream()), "marl_td_lambda_returns")
    return out


def _iql_rows(B, T, N, A, per_row_a, per_row, per_step):
    R = B * T * N
    for t, n in [(x, R * A) for x in per_row_a] + [(x, R) for x in per_row] + [(x, B * T) for x in per_step]:
        assert t is None or (t.is_cuda and t.is_contiguous() and t.numel() >= n), "iql: contiguous device arrays of the rows' sizes"


def iql_loss_bwd(q, u, q_sel, q_tgt, avail_next, ret, r, term, padded, gamma, mask_val, dq_val, out2, B, T, N, A,
                 q_taken=None, q_next=None):
    """Independent Q-learning's loss tail over the R = B T N agent rows (csrc/iql.hip): the taken actions' Qs, the double-Q
    selection (q_sel None: the masked max of q_tgt), the one-step target, out2 = {sum m td^2, N sum m} and the sparse gradient
    dq_val = -2 m td in one row pass; with ``ret`` (B, N, T) the target is ret and no selection runs."""
    lib = _lib.load()
    _iql_rows(B, T, N, A, (q, q_sel, q_tgt, avail_next), (u, ret, dq_val, q_taken, q_next), (r, term, padded))
    ws = WS.get("loss", lib.marl_loss_workspace(B * T * N), q.device)
    check(lib.marl_iql_loss_bwd(_p(_f32(q)), _p(_i32(u)), _p(q_sel), _p(q_tgt), _p(avail_next), _p(ret), _p(r), _p(term),
                                _p(_f32(padded)), float(gamma), float(mask_val), _p(_f32(dq_val)), _p(q_taken), _p(q_next),
                                _p(_f32(out2)), _p(ws), int(B), int(T), int(N), int(A), _stream()), "marl_iql_loss_bwd")
    return dq_val


def iql_select(q, u, q_sel, q_tgt, avail_next, padded, mask_val, q_taken, q_next_bnt, B, T, N, A):
    """the selection half of iql_loss_bwd alone: q_taken (R, optional) and q_next in (B, N, T) layout, the one
    td_lambda_returns scans on B N sequences"""
    _iql_rows(B, T, N, A, (q, q_sel, q_tgt, avail_next), (u, q_taken, q_next_bnt), (padded,))
    check(_lib.load().marl_iql_select(_p(_f32(q)), _p(_i32(u)), _p(q_sel), _p(_f32(q_tgt)), _p(avail_next), _p(_f32(padded)),
                                      float(mask_val), _p(q_taken), _p(_f32(q_next_bnt)), int(B), int(T), int(N), int(A),
                                      _stream()), "marl_iql_select")
    return q_next_bnt


def wqmix_supported(N, A):
    return bool(_lib.load().marl_wqmix_supported(int(N), int(A)))


def wqmix_select(q, qc, u, avail, q_en, qc_tgt, avail_next, padded, mask_val, q_taken, qc_taken, u_next, qc_next, B, T, N, A,
                 u_greedy=None, qc_greedy=None):
    """Weighted QMIX's selections in one pass over the R = B T N agent rows (csrc/wqmix.hip): the taken action's Q of the eval and
    of the central agent, the double-Q greedy next action by q_en with the target central agent's masked Q there and - for CW, when
    u_greedy / qc_greedy are given - the current greedy action by q with the central agent's Q there."""
    _iql_rows(B, T, N, A, (q, qc, avail, q_en, qc_tgt, avail_next), (u, q_taken, qc_taken, u_next, qc_next, u_greedy, qc_greedy),
              (padded,))
    check(_lib.load().marl_wqmix_select(_p(_f32(q)), _p(_f32(qc)), _p(_i32(u)), _p(avail), _p(_f32(q_en)), _p(_f32(qc_tgt)),
                                        _p(avail_next), _p(_f32(padded)), float(mask_val), _p(_f32(q_taken)), _p(_f32(qc_taken)),
                                        _p(u_greedy), _p(qc_greedy), _p(_i32(u_next)), _p(_f32(qc_next)), int(B), int(T), int(N),
                                        int(A), _stream()), "marl_wqmix_select")


def wqmix_loss(q_tot, qc, qc_g, qc_next_tot, r, term, padded, gamma, u, u_greedy, alpha, dq_tot, dqc, out4, rows, N, w=None):
    """Weighted QMIX's loss over the B T rows (csrc/wqmix.hip): the target of the target central mixer's value, the OW (qc_g None)
    or CW weight, dq_tot = -2 w m (m td), dqc = -2 m (m tdc) and out4 = {sum w (m td)^2, sum m, sum (m tdc)^2, sum m [w == 1]}."""
    lib = _lib.load()
    for t, n in [(x, rows) for x in (q_tot, qc, qc_g, qc_next_tot, r, term, padded, dq_tot, dqc, w)] + \
                [(x, rows * N) for x in (u, u_greedy)]:
        assert t is None or (t.is_cuda and t.is_contiguous() and t.numel() >= n), "wqmix_loss: contiguous device arrays of the rows' sizes"
    ws = WS.get("loss", lib.marl_loss_workspace(rows), q_tot.device)
    check(lib.marl_wqmix_loss(_p(_f32(q_tot)), _p(_f32(qc)), _p(qc_g), _p(_f32(qc_next_tot)), _p(_f32(r)), _p(_f32(term)),
                              _p(_f32(padded)), float(gamma), _p(u), _p(u_greedy), float(alpha), _p(_f32(dq_tot)), _p(_f32(dqc)),
                              _p(w), _p(_f32(out4)), _p(ws), int(rows), int(N), _stream()), "marl_wqmix_loss")


def policy_probs(logits, avail, eps, pi, rows, A):
    """pi (rows, A) of the stochastic policy (csrc/policy.hip): softmax of the logits, mixed with eps of the uniform policy over the
    available actions, renormalised over them; a row without an available action is all zeros"""
    for t in (logits, avail, pi):
        assert _f32(t).is_contiguous() and t.numel() >= rows * A
    check(_lib.load().marl_policy_probs(_p(logits), _p(avail), float(eps), _p(pi), rows, A, _stream()), "marl_policy_probs")
    return pi


def policy_loss_bwd(logits, avail, u, G, v, padded, eps, dlogits, logp, out2, rows, N, A):
    """The actor loss of rows = B*T*N agent steps: logp (rows), out2 = {- sum m (G - v) logp, N sum m} and dlogits (rows, A), the
    un-normalised gradient of out2[0] by the logits - the dense dq of agent_unroll_bwd."""
    lib = _lib.load()
    for t, n in ((logits, rows * A), (avail, rows * A), (dlogits, rows * A), (logp, rows), (G, rows // N), (v, rows // N),
                 (padded, rows // N)):
        assert _f32(t).is_contiguous() and t.numel() >= n
    assert _i32(u).is_contiguous() and u.numel() >= rows and out2.numel() >= 2
    ws = WS.get("loss", lib.marl_loss_workspace(rows), logits.device)
    check(lib.marl_policy_loss_bwd(_p(logits), _p(avail), _p(u), _p(G), _p(v), _p(padded), float(eps), _p(dlogits), _p(logp),
                                   _p(_f32(out2)), _p(ws), rows, N, A, _stream()), "marl_policy_loss_bwd")


def policy_loss_bwd_ex(logits, avail, u, G, v, padded, eps, beta, dlogits, logp, ent, out3, rows, N, A):
    """policy_loss_bwd without a baseline (``v`` None: Adv = G) and with the entropy bonus ``beta`` >= 0 of the policy the actions
    were drawn from: out3 = {- sum m Adv logp - beta sum m H, N sum m, sum m H}, ent (rows) = H or None, and
    dlogits = - m Adv dlogp/dz - beta m dH/dz.  beta = 0 with v: policy_loss_bwd's dlogits, logp and statistics bit for bit."""
    lib = _lib.load()
    for t, n in ((logits, rows * A), (avail, rows * A), (dlogits, rows * A), (logp, rows), (G, rows // N), (padded, rows // N)) + \
            (() if v is None else ((v, rows // N),)) + (() if ent is None else ((ent, rows),)):
        assert _f32(t).is_contiguous() and t.numel() >= n
    assert _i32(u).is_contiguous() and u.numel() >= rows and out3.numel() >= 3
    ws = WS.get("loss", lib.marl_loss_workspace(rows), logits.device)
    check(lib.marl_policy_loss_bwd_ex(_p(logits), _p(avail), _p(u), _p(G), _p(v), _p(padded), float(eps), float(beta), _p(dlogits),
                                      _p(logp), _p(ent), _p(_f32(out3)), _p(ws), rows, N, A, _stream()), "marl_policy_loss_bwd_ex")


def policy_probs_bwd(logits, avail, gpi, q_pi, padded, eps, beta, dlogits, ent, out3, rows, N, A):
    """LICA's actor pass (csrc/policy.hip): dlogits (rows, A) = J^T gpi - beta m dH/dz, the transpose-Jacobian of the policy by its
    logits applied to gpi = dL/dpi; ent (rows) = H or None; out3 = {- sum m q_pi - beta sum m H, N sum m, sum m H} with q_pi
    (rows / N) or None.  dlogits may be logits or gpi."""
    lib = _lib.load()
    for t, n in ((logits, rows * A), (avail, rows * A), (gpi, rows * A), (dlogits, rows * A), (padded, rows // N)) + \
            (() if q_pi is None else ((q_pi, rows // N),)) + (() if ent is None else ((ent, rows),)):
        assert _f32(t).is_contiguous() and t.numel() >= n
    assert out3.numel() >= 3
    ws = WS.get("loss", lib.marl_loss_workspace(rows), logits.device)
    check(lib.marl_policy_probs_bwd(_p(logits), _p(avail), _p(gpi), _p(q_pi), _p(padded), float(eps), float(beta), _p(dlogits),
                                    _p(ent), _p(_f32(out3)), _p(ws), rows, N, A, _stream()), "marl_policy_probs_bwd")


def ppo_loss_bwd(logits, avail, u, adv, logp_old, padded, eps, beta, clip, dlogits, logp, ent, out4, rows, N, A):
    """policy_loss_bwd_ex's pass under PPO's clipped surrogate (csrc/policy.hip): ``adv`` (rows / N) in the place of G - v,
    ``logp_old`` (rows) or None (rho = 1 exactly: the batch's first pass), ``clip`` = c in (0, 1).  out4 = {- sum m min(rho adv,
    clamp(rho, 1 - c, 1 + c) adv) - beta sum m H, N sum m, sum m H, sum m [clipped]}, ent (rows) = H or None, and
    dlogits = - m (clipped ? 0 : adv rho) dlogp/dz - beta m dH/dz.  logp_old None: policy_loss_bwd_ex's dlogits, logp and ent with
    G = adv and no v, bit for bit."""
    lib = _lib.load()
    for t, n in ((logits, rows * A), (avail, rows * A), (dlogits, rows * A), (logp, rows), (adv, rows // N), (padded, rows // N)) + \
            (() if logp_old is None else ((logp_old, rows),)) + (() if ent is None else ((ent, rows),)):
        assert _f32(t).is_contiguous() and t.numel() >= n
    assert _i32(u).is_contiguous() and u.numel() >= rows and out4.numel() >= 4
    ws = WS.get("loss", lib.marl_loss_workspace(rows), logits.device)
    check(lib.marl_ppo_loss_bwd(_p(logits), _p(avail), _p(u), _p(adv), _p(logp_old), _p(padded), float(eps), float(beta), float(clip),
                                _p(dlogits), _p(logp), _p(ent), _p(_f32(out4)), _p(ws), rows, N, A, _stream()), "marl_ppo_loss_bwd")


def masked_standardize(x, padded, out, stats3, rows):
    """out = m (x - mean) / (sqrt(var) + 1e-5) over the live rows (m = 1 - padded; csrc/ppo.hip): exact zeros on padded rows, all
    zeros when none is live; stats3 = {mean, var, sum m}.  ``out`` may be ``x``."""
    lib = _lib.load()
    for t in (x, padded, out):
        assert _f32(t).is_contiguous() and t.numel() >= rows
    assert _f32(stats3).numel() >= 3
    ws = WS.get("loss", lib.marl_loss_workspace(rows), x.device)
    check(lib.marl_masked_standardize(_p(x), _p(padded), _p(out), _p(stats3), _p(ws), rows, _stream()), "marl_masked_standardize")
    return out


def policy_sample(logits, avail, avail_es, alive, eps, rseed, env0, tg, tg0, act_out, act_es, E, N, A):
    """select_actions' arguments; draws every live agent's action from the stochastic policy"""
    check(_lib.load().marl_policy_sample(_p(_f32(logits)), _p(_f32(avail)), avail_es, _p(alive), float(eps),
                                         int(rseed) & 0xFFFFFFFF, env0, _p(tg), tg0, _p(_i32(act_out)), act_es,
                                         E, N, A, _stream()), "marl_policy_sample")


def _dense(t, n):
    assert _f32(t).is_contiguous() and t.numel() >= n
    return _p(t)


def coma_onehot_cols(W, col0, Wt, C, D):
    """Wt (C, D) = the K-major copy of columns [col0, col0 + C) of the row-major weight W (D, K) (csrc/coma.hip)"""
    assert W.dim() == 2 and W.stride(1) == 1 and W.shape[0] == D and col0 + C <= W.shape[1]
    check(_lib.load().marl_coma_onehot_cols(_p(_f32(W)), W.stride(0), col0, _dense(Wt, C * D), C, D, _stream()),
          "marl_coma_onehot_cols")


def coma_fc1_fwd(pre_s, Wt, u, h1, B, T, N, A, D):
    """h1 (R, D) holds the observation block's product on entry and relu(h1 + pre_s[step] + the gathered one-hot columns) on return:
    the COMA critic's first layer without its (R, K) input (include/marl_hip.h)"""
    R = B * T * N
    assert _i32(u).is_contiguous() and u.numel() >= R
    check(_lib.load().marl_coma_fc1_fwd(_dense(pre_s, B * T * D), _dense(Wt, (2 * N * A + N) * D), _p(u), _dense(h1, R * D),
                                        B, T, N, A, D, _stream()), "marl_coma_fc1_fwd")


def coma_fc1_bwd(dh1, h1, u, dpre, dsum, dW, col0, B, T, N, A, D):
    """dpre = dh1 (h1 > 0), dsum = its per-step agent sum, and the one-hot columns' gradient added into dW[:, col0:col0 + 2NA + N]
    (dW: the (D, K) gradient view of fc1.weight)"""
    lib = _lib.load()
    R = B * T * N
    assert _i32(u).is_contiguous() and u.numel() >= R
    assert dW.dim() == 2 and dW.stride(1) == 1 and dW.shape[0] == D and col0 + 2 * N * A + N <= dW.shape[1]
    ws = WS.get("coma_fc1", lib.marl_coma_fc1_bwd_workspace(B, T, N, A, D), dh1.device)
    check(lib.marl_coma_fc1_bwd(_dense(dh1, R * D), _dense(h1, R * D), _p(u), _dense(dpre, R * D), _dense(dsum, B * T * D),
                                _p(_f32(dW)), dW.stride(0), col0, _p(ws), ws.numel() * 4, B, T, N, A, D, _stream()),
          "marl_coma_fc1_bwd")


def coma_q_taken(q, u, out, shift, B, T, N, A):
    """out (B, N, T): the taken action's Q at step t + shift, 0 past the window"""
    R = B * T * N
    assert _i32(u).is_contiguous() and u.numel() >= R
    check(_lib.load().marl_coma_q_taken(_dense(q, R * A), _p(u), _dense(out, R), int(shift), B, T, N, A, _stream()),
          "marl_coma_q_taken")


def coma_loss_bwd(logits, avail, q, u, G, padded, eps, beta, dlogits, dq, logp, ent, adv, q_taken, out_c2, out_a3, B, T, N, A):
    """COMA's two losses of one critic pass (include/marl_hip.h): G (B, N, T); out_c2 = {critic numerator, N M},
    out_a3 = {actor numerator, N M, sum m H}; dlogits / dq (R, A) un-normalised"""
    lib = _lib.load()
    R = B * T * N
    assert _i32(u).is_contiguous() and u.numel() >= R and out_c2.numel() >= 2 and out_a3.numel() >= 3
    ws = WS.get("loss", lib.marl_loss_workspace(R), logits.device)
    check(lib.marl_coma_loss_bwd(_dense(logits, R * A), _dense(avail, R * A), _dense(q, R * A), _p(u), _dense(G, R),
                                 _dense(padded, B * T), float(eps), float(beta), _dense(dlogits, R * A), _dense(dq, R * A),
                                 _dense(logp, R), _dense(ent, R), _dense(adv, R), _dense(q_taken, R), _p(_f32(out_c2)),
                                 _p(_f32(out_a3)), _p(ws), B, T, N, A, _stream()), "marl_coma_loss_bwd")


# ---- CommNet communication head (csrc/commnet.hip)
_COMMNET_KEYS = (("w_ih", "f_comm.weight_ih"), ("w_hh", "f_comm.weight_hh"), ("b_ih", "f_comm.bias_ih"), ("b_hh", "f_comm.bias_hh"),
                 ("dec_w", "decoding.weight"), ("dec_b", "decoding.bias"))
_COMMNET_FIELDS = [(field, name, torch.float32) for field, name in _COMMNET_KEYS]


def commnet_supported(N, A, K):
    return bool(_lib.load().marl_commnet_supported(int(N), int(A), int(K)))


def commnet_groups_per_workgroup(N):
    """whole groups (environment-steps) in one 16-row tile of the head kernels"""
    return int(_lib.load().marl_commnet_groups_per_workgroup(int(N)))


def commnet_weights(tensors):
    """tensors: dict name -> tensor with CommNetAgent's keys (f_comm.*, decoding.*)"""
    return _fill_struct(MarlCommnetWeights, tensors, _COMMNET_FIELDS)


def commnet_grads(grads):
    """grads: dict of the same keys -> gradient tensors (accumulated into)"""
    return _fill_struct(MarlCommnetGrads, grads, _COMMNET_FIELDS)


def commnet_head_fwd(w, hs, logits, G, N, A, K):
    """logits (G,N,A) <- hs (G,N,64): K rounds of f_comm over each group's N rows, then decoding"""
    assert hs.is_contiguous() and logits.is_contiguous()
    check(_lib.load().marl_commnet_head_fwd(C.byref(w), _p(_f32(hs)), _p(_f32(logits)), int(G), int(N), int(A), int(K), _stream()),
          "marl_commnet_head_fwd")


def commnet_head_bwd(w, g, hs, dlogits, dhs, G, N, A, K):
    """dhs (G,N,64) written; f_comm's and decoding's gradients added into g (fixed-order slab reduction)"""
    lib = _lib.load()
    assert hs.is_contiguous() and dlogits.is_contiguous() and dhs.is_contiguous()
    ws = WS.get("commnet_bwd", lib.marl_commnet_bwd_workspace(int(G), int(N), int(A), int(K)), hs.device)
    check(lib.marl_commnet_head_bwd(C.byref(w), C.byref(g), _p(_f32(hs)), _p(_f32(dlogits)), _p(_f32(dhs)), _p(ws), ws.numel() * 4,
                                    int(G), int(N), int(A), int(K), _stream()), "marl_commnet_head_bwd")


def commnet_sigmoid_fwd(x):
    """x <- sigmoid(x) in place (any contiguous float32 view)"""
    assert x.is_contiguous()
    check(_lib.load().marl_commnet_sigmoid_fwd(_p(_f32(x)), x.numel(), _stream()), "marl_commnet_sigmoid_fwd")


def commnet_sigmoid_bwd(de, e, dxp):
    """dxp = de * e * (1 - e); dxp may be de"""
    assert de.is_contiguous() and e.is_contiguous() and dxp.is_contiguous() and de.numel() == e.numel() == dxp.numel()
    check(_lib.load().marl_commnet_sigmoid_bwd(_p(_f32(de)), _p(_f32(e)), _p(_f32(dxp)), de.numel(), _stream()),
          "marl_commnet_sigmoid_bwd")


# ---- G2ANet attention head (csrc/g2anet.hip)
_G2ANET_KEYS = (("gf_w_ih", "hard_bi_GRU.weight_ih_l0"), ("gf_w_hh", "hard_bi_GRU.weight_hh_l0"), ("gf_b_ih", "hard_bi_GRU.bias_ih_l0"),
                ("gf_b_hh", "hard_bi_GRU.bias_hh_l0"), ("gr_w_ih", "hard_bi_GRU.weight_ih_l0_reverse"),
                ("gr_w_hh", "hard_bi_GRU.weight_hh_l0_reverse"), ("gr_b_ih", "hard_bi_GRU.bias_ih_l0_reverse"),
                ("gr_b_hh", "hard_bi_GRU.bias_hh_l0_reverse"), ("he_w", "hard_encoding.weight"), ("he_b", "hard_encoding.bias"),
                ("q_w", "q.weight"), ("k_w", "k.weight"), ("v_w", "v.weight"), ("v_b", "v.bias"), ("dec_w", "decoding.weight"),
                ("dec_b", "decoding.bias"))
_G2ANET_FIELDS = [(field, name, torch.float32) for field, name in _G2ANET_KEYS]
G2ANET_HEAD_PARAMS = tuple(name for _, name in _G2ANET_KEYS)


def g2anet_supported(N, A, hard=True):
    return bool(_lib.load().marl_g2anet_supported(int(N), int(A), 1 if hard else 0))


def g2anet_groups_per_workgroup(N):
    """whole groups (environment-steps) in one 16-row tile of the head kernels"""
    return int(_lib.load().marl_g2anet_groups_per_workgroup(int(N)))


def g2anet_weights(tensors):
    """tensors: dict name -> tensor with G2ANetAgent's head keys (G2ANET_HEAD_PARAMS)"""
    return _fill_struct(MarlG2anetWeights, tensors, _G2ANET_FIELDS)


def g2anet_grads(grads):
    """grads: dict of the same keys -> gradient tensors (accumulated into)"""
    return _fill_struct(MarlG2anetGrads, grads, _G2ANET_FIELDS)


def g2anet_head_fwd(w, hs, noise, logits, G, N, A, hard, tau):
    """logits (G,N,A) <- hs (G,N,64), noise (G,N,N-1) or None (l = 0): hard attention, soft attention, decoding"""
    assert hs.is_contiguous() and logits.is_contiguous() and (noise is None or (_f32(noise).is_contiguous() and noise.numel() >= G * N * (N - 1)))
    check(_lib.load().marl_g2anet_head_fwd(C.byref(w), _p(_f32(hs)), _p(noise), _p(_f32(logits)), int(G), int(N), int(A),
                                           1 if hard else 0, float(tau), _stream()), "marl_g2anet_head_fwd")


def g2anet_head_bwd(w, g, hs, noise, dlogits, dhs, G, N, A, hard, tau):
    """dhs (G,N,64) written; the head's sixteen gradients added into g (fixed-order slab reductions)"""
    lib = _lib.load()
    assert hs.is_contiguous() and dlogits.is_contiguous() and dhs.is_contiguous()
    assert noise is None or (_f32(noise).is_contiguous() and noise.numel() >= G * N * (N - 1))
    ws = WS.get("g2anet_bwd", lib.marl_g2anet_bwd_workspace(int(G), int(N), int(A), 1 if hard else 0), hs.device)
    check(lib.marl_g2anet_head_bwd(C.byref(w), C.byref(g), _p(_f32(hs)), _p(noise), _p(_f32(dlogits)), _p(_f32(dhs)), _p(ws),
                                   ws.numel() * 4, int(G), int(N), int(A), 1 if hard else 0, float(tau), _stream()),
          "marl_g2anet_head_bwd")


def g2anet_noise(seed, env0, tg0, noise, E, T, N):
    """noise (E,T,N,N-1) <- the logistic draws of (seed, env0 + e, tg0 + t)"""
    assert _f32(noise).is_contiguous() and noise.numel() >= E * T * N * (N - 1)
    check(_lib.load().marl_g2anet_noise(int(seed) & 0xFFFFFFFF, int(env0), int(tg0) & 0xFFFFFFFF, _p(noise), int(E), int(T), int(N),
                                        _stream()), "marl_g2anet_noise")


def grad_sumsq(g, n, out1):
    lib = _lib.load()
    ws = WS.get("sumsq", lib.marl_sumsq_workspace(n), g.device)
    check(lib.marl_grad_sumsq(_p(_f32(g)), n, _p(_f32(out1)), _p(ws), _stream()), "marl_grad_sumsq")


def rmsprop_step(p, g, sq, n, lr, alpha, eps, clip, sumsq, den):
    check(_lib.load().marl_rmsprop_step(_p(_f32(p)), _p(_f32(g)), _p(_f32(sq)), n, float(lr), float(alpha), float(eps),
                                        float(clip), _p(sumsq), _p(den), _stream()), "marl_rmsprop_step")


def adam_step(p, g, m, v, n, lr, b1, b2, eps, bc1, bc2s, clip, sumsq, den):
    check(_lib.load().marl_adam_step(_p(_f32(p)), _p(_f32(g)), _p(_f32(m)), _p(_f32(v)), n, float(lr), float(b1),
                                     float(b2), float(eps), float(bc1), float(bc2s), float(clip), _p(sumsq), _p(den),
                                     _stream()), "marl_adam_step")


def select_actions(q, avail, avail_es, alive, eps, rseed, env0, tg, tg0, act_out, act_es, E, N, A):
    check(_lib.load().marl_select_actions(_p(_f32(q)), _p(_f32(avail)), avail_es, _p(alive), float(eps),
                                          int(rseed) & 0xFFFFFFFF, env0, _p(tg), tg0, _p(_i32(act_out)), act_es,
                                          E, N, A, _stream()), "marl_select_actions")


def synth_lengths(seed, env0, episode, length, won, E, T):
    check(_lib.load().marl_synth_lengths(int(seed) & 0xFFFFFFFF, env0, episode, _p(_i32(length)), _p(won), E, T,
                                         _stream()), "marl_synth_lengths")


_RECORD_FIELDS = (("obs", _f32), ("state", _f32), ("avail", _f32), ("u", _i32), ("r", _f32), ("term", _f32), ("padded", _f32),
                  ("length", _i32), ("won", _i32))
# where the fields are looked up: EpisodeRecord's `state` is a fresh view of state_store at every read (same pointer and row stride)
_RECORD_ATTRS = tuple("state_store" if f == "state" else f for f, _ in _RECORD_FIELDS)
_cached_struct = None       # hostutil.cached_struct, bound at the first use: hostutil imports this module


def record(rec, cache=True):
    """the MarlRecord of an object with EpisodeRecord's attributes (a field an entry does not read: None), by reference.  Kept on `rec`
    and rebuilt only when a field's storage moved: a launch-per-step rollout builds it once.  cache = False: built for this call alone
    (a whole rollout is ONE launch per record, usually a fresh view of the replay ring)"""
    global _cached_struct
    if _cached_struct is None:
        from .hostutil import cached_struct as _cached_struct
    ts = [getattr(rec, a, None) for a in _RECORD_ATTRS]
    st = ts[1] = ts[1] if ts[1] is not None else getattr(rec, "state", None)
    build = lambda: MarlRecord(state_ld=0 if st is None else st.stride(-2), E=rec.E, T=rec.T, N=rec.N, O=rec.O, S=rec.S, A=rec.A,
                               **{f: kind(t).data_ptr() for (f, kind), t in zip(_RECORD_FIELDS, ts) if t is not None})
    return C.byref(_cached_struct(rec, "record", [t for t in ts if t is not None], build) if cache else build())


def _entry(name, sample=False, x6=False):
    """(function, its exact name for check) of an entry point and its _sample / _x6 variants"""
    name += "_sample" if sample else "_x6" if x6 else ""
    return getattr(_lib.load(), name), name


def synth_observe(seed, env0, episode, t, rec):
    check(_lib.load().marl_synth_observe(int(seed) & 0xFFFFFFFF, env0, episode, t, record(rec), _stream()), "marl_synth_observe")


def synth_step(seed, env0, episode, t, act, rec, alive_next):
    check(_lib.load().marl_synth_step(int(seed) & 0xFFFFFFFF, env0, episode, t, _p(_i32(act)), record(rec), _p(alive_next),
                                      _stream()), "marl_synth_step")


def synth_fused_step(seed, rseed, env0, episode, t, eps, q, rec, sample=False):
    """sample: the actions are drawn from the stochastic policy of q (logits) with eps as its mixing epsilon (policy_sample's rule)"""
    fn, name = _entry("marl_synth_fused_step", sample)
    check(fn(int(seed) & 0xFFFFFFFF, int(rseed) & 0xFFFFFFFF, env0, episode, t, float(eps), _p(_f32(q)), record(rec), _stream()), name)


def battle_supported(n_allies, n_enemies, A):
    return bool(_lib.load().marl_battle_supported(n_allies, n_enemies, A))


def battle_reset(seed, env0, episode, types, shield, type_bits, units, rec, M):
    """start of an episode of the battle environment (csrc/battle.hip): unit state, length, won and slot 0 of the record"""
    check(_lib.load().marl_battle_reset(int(seed) & 0xFFFFFFFF, env0, episode, types, int(shield), type_bits, _p(_i32(units)),
                                        record(rec), M, _stream()), "marl_battle_reset")


def battle_step(types, shield, type_bits, scale, t, act, units, rec, alive_next, M):
    """lock-step t of the battle environment in one launch: step t of the record, the unit state and slot t + 1"""
    check(_lib.load().marl_battle_step(types, int(shield), type_bits, float(scale), t, _p(_i32(act)), _p(_i32(units)), record(rec),
                                       _p(alive_next), M, _stream()), "marl_battle_step")


def battle_fused_step(types, shield, type_bits, scale, rseed, env0, episode, t, eps, q, units, rec, M, sample=False):
    """the action choice (select_actions' rule and draws; sample: policy_sample's) and battle_step in one launch"""
    fn, name = _entry("marl_battle_fused_step", sample)
    check(fn(types, int(shield), type_bits, float(scale), int(rseed) & 0xFFFFFFFF, env0, episode, t, float(eps), _p(_f32(q)),
             _p(_i32(units)), record(rec), M, _stream()), name)


def battle_rollout_supported(N, O, A):
    return bool(_lib.load().marl_battle_rollout_supported(int(N), int(O), int(A)))


def battle_rollout_plan(E, N, O, A, last_action=True, reuse_network=True):
    """(workgroups, environments per workgroup, row tiles per workgroup, dynamic LDS bytes) of a whole battle rollout"""
    plan = (C.c_int * 4)()
    check(_lib.load().marl_battle_rollout_plan(int(E), int(N), int(O), int(A), 1 if last_action else 0, 1 if reuse_network else 0,
                                               plan), "marl_battle_rollout_plan")
    return tuple(plan)


def battle_rollout(w, seed, rseed, env0, episode, types, shield, type_bits, scale, units, rec, h_out, M, last_action,
                   reuse_network, stats, eps_sched, sample=False):
    """reset and all T lock-steps of the battle environment in ONE persistent launch (csrc/battle_rollout.hip): every field of rec,
    the final unit state, stats (3, E) = reward sum | won | length (or None) and h_out (or None).  eps_sched = (eps0, anneal,
    eps_min), evaluated inside the kernel in fp64; sample: the actions are drawn from the stochastic policy of the step's logits"""
    fn, name = _entry("marl_battle_rollout", sample)
    check(fn(C.byref(w), record(rec, cache=False), int(seed) & 0xFFFFFFFF, int(rseed) & 0xFFFFFFFF, env0, episode, types, int(shield),
             type_bits, float(scale), _p(_i32(units)), _p(h_out), _p(_f32(stats)) if stats is not None else None,
             *map(float, eps_sched), M, 1 if last_action else 0, 1 if reuse_network else 0, _stream()), name)


def hunt_supported(N, M, G, A):
    return bool(_lib.load().marl_hunt_supported(int(N), int(M), int(G), int(A)))


def hunt_reset(seed, env0, episode, G, M, units, rec):
    """start of an episode of the hunt environment (csrc/hunt.hip): unit state, length, won and slot 0 of the record"""
    check(_lib.load().marl_hunt_reset(int(seed) & 0xFFFFFFFF, env0, episode, G, M, _p(_i32(units)), record(rec), _stream()),
          "marl_hunt_reset")


def hunt_step(seed, env0, episode, G, pen4, t, act, units, rec, alive_next, M):
    """lock-step t of the hunt environment in one launch: step t of the record, the unit state and slot t + 1"""
    check(_lib.load().marl_hunt_step(int(seed) & 0xFFFFFFFF, env0, episode, G, pen4, t, _p(_i32(act)), _p(_i32(units)), record(rec),
                                     _p(alive_next), M, _stream()), "marl_hunt_step")


def hunt_fused_step(seed, rseed, env0, episode, G, pen4, t, eps, q, units, rec, M, sample=False):
    """the action choice (select_actions' rule and draws; sample: policy_sample's) and hunt_step in one launch"""
    fn, name = _entry("marl_hunt_fused_step", sample)
    check(fn(int(seed) & 0xFFFFFFFF, int(rseed) & 0xFFFFFFFF, env0, episode, G, pen4, t, float(eps), _p(_f32(q)), _p(_i32(units)),
             record(rec), M, _stream()), name)


def synth_rollout_supported(N, O, A):
    return bool(_lib.load().marl_synth_rollout_supported(N, O, A))


def synth_rollout_x6_supported(N, O, A, last_action=True, reuse_network=True):
    return bool(_lib.load().marl_synth_rollout_x6_supported_flags(N, O, A, 1 if last_action else 0, 1 if reuse_network else 0))


def synth_rollout_x6_plan(E, N, O, A, last_action=True, reuse_network=True):
    """(decomposition 1 / 2, workgroups, row tiles per workgroup, environments per workgroup, fc1 chunks) of a split whole rollout"""
    plan = (C.c_int * 5)()
    check(_lib.load().marl_synth_rollout_x6_plan(E, N, O, A, 1 if last_action else 0, 1 if reuse_network else 0, plan), "marl_synth_rollout_x6_plan")
    return tuple(plan)


def synth_rollout(w, seed, rseed, env0, episode, fixed_len, eps, rec, h_out, E, T, N, O, S, A, last_action, reuse_network,
                  stats=None, eps_sched=None, x6=False, sample=False):
    """E .. A: the record's sizes once more, by position - bench.py's roofline model reads them off this call.  eps: device (T,) epsilon
    per lock-step, or None with eps_sched = (eps0, anneal, eps_min): the per-step anneal of rollout.py:100-101 is then evaluated inside
    the kernel (fp64, like the host loop) and no schedule crosses PCIe.  x6: the agent step as bf16x6 split products.  sample: the
    actions are drawn from the stochastic policy of the step's logits, eps(t) its mixing epsilon; always the fp32 kernel (x6 is ignored)."""
    assert (eps is None) != (eps_sched is None) and (E, T, N, O, S, A) == (rec.E, rec.T, rec.N, rec.O, rec.S, rec.A)
    fn, name = _entry("marl_synth_rollout", sample, x6)
    check(fn(C.byref(w), record(rec, cache=False), int(seed) & 0xFFFFFFFF, int(rseed) & 0xFFFFFFFF, env0, episode, 1 if fixed_len else 0,
             _p(_f32(eps)) if eps is not None else None, _p(h_out), _p(_f32(stats)) if stats is not None else None,
             *map(float, eps_sched or (0.0, 0.0, 0.0)), 1 if last_action else 0, 1 if reuse_network else 0, _stream()), name)


def qmix_fused_supported(N, S, E):
    return bool(_lib.load().marl_qmix_fused_supported(N, S, E))


def qmix_weights(t):
    """t: dict with tensors w1,w1_b,b1,b1_b,w2,w2_b,h,h_b,b2_w,b2_b (weights or their gradients)."""
    return _fill_struct(MarlQmixWeights, t, [(k, k, torch.float32) for k, _ in MarlQmixWeights._fields_])


def qmix_fused_fwd(w, s, q, q_tot, rows, N, S, E, x6=False):
    """x6: the bf16x6 split variant of the kernel (args.gemm_mode = "bf16x6"; same arguments)"""
    lib = _lib.load()
    fn = lib.marl_qmix_fused_fwd_x6 if x6 else lib.marl_qmix_fused_fwd
    check(fn(C.byref(w), C.byref(s), _p(_f32(q)), _p(_f32(q_tot)), rows, N, S, E, _stream()), "marl_qmix_fused_fwd")


def qmix_fused_bwd(w, s, q, dq_tot, dq, grads, rows, N, S, E, x6=False):
    lib = _lib.load()
    ws = WS.get("qmix_fused", lib.marl_qmix_fused_workspace(rows, N, S), q.device)
    fn = lib.marl_qmix_fused_bwd_x6 if x6 else lib.marl_qmix_fused_bwd
    check(fn(C.byref(w), C.byref(s), _p(_f32(q)), _p(_f32(dq_tot)), _p(_f32(dq)), C.byref(grads),
             _p(ws), ws.numel() * 4, rows, N, S, E, _stream()), "marl_qmix_fused_bwd")


def qmix_fused_loss_bwd(w, s, q, q_tot_tgt, r, term, padded, gamma, q_tot, dq, grads, loss2, rows, N, S, E, x6=False):
    """fused QMIX backward with the TD loss folded in (include/marl_hip.h); loss2: 2-element device view accumulated into"""
    lib = _lib.load()
    ws = WS.get("qmix_fused", lib.marl_qmix_fused_workspace(rows, N, S), q.device)
    check((lib.marl_qmix_fused_loss_bwd_x6 if x6 else lib.marl_qmix_fused_loss_bwd)(C.byref(w), C.byref(s), _p(_f32(q)), _p(_f32(q_tot_tgt)), _p(_f32(r)), _p(_f32(term)),
                                       _p(_f32(padded)), float(gamma), _p(q_tot), _p(_f32(dq)), C.byref(grads), _p(_f32(loss2)),
                                       _p(ws), ws.numel() * 4, rows, N, S, E, _stream()), "marl_qmix_fused_loss_bwd")


def _wide_flags(bf16, wgrad_bf16):
    """flags of the wide-state QMIX entry points: bit 0 = bf16 operands of the hypernet GEMM, bit 1 = bf16 operands of the
    weight-gradient GEMM too (its own bit: a C-ABI caller that sets only bit 0 keeps fp32 weight gradients)"""
    return (1 if bf16 else 0) | (2 if (bf16 and (wgrad_bf16 is None or wgrad_bf16)) else 0)


def qmix_wide_loss_bwd(w, s, q, q_tot_tgt, r, term, padded, gamma, q_tot, dq, grads, loss2, rows, N, S, E, bf16=False, wgrad_bf16=None):
    """wide-state fused QMIX backward with the TD loss folded in (include/marl_hip.h); wgrad_bf16: None = follow bf16"""
    lib = _lib.load()
    ws = WS.get("qmix_wide", lib.marl_qmix_wide_workspace(rows, N, S, 1), q.device)
    check(lib.marl_qmix_wide_loss_bwd(C.byref(w), C.byref(s), _p(_f32(q)), _p(_f32(q_tot_tgt)), _p(_f32(r)), _p(_f32(term)),
                                      _p(_f32(padded)), float(gamma), _p(q_tot), _p(_f32(dq)), C.byref(grads), _p(_f32(loss2)),
                                      _p(ws), ws.numel() * 4, rows, N, S, E, _wide_flags(bf16, wgrad_bf16), _stream()), "marl_qmix_wide_loss_bwd")


def qmix_wide_fwd_kernel(rows, N, S, bf16=False):
    """name prefix (rocprofv3 kernel trace) of the forward kernel qmix_wide_fwd launches for this shape"""
    return _lib.load().marl_qmix_wide_fwd_kernel(rows, N, S, 1 if bf16 else 0).decode()


def qmix_wide_supported(N, S, E):
    return bool(_lib.load().marl_qmix_wide_supported(N, S, E))


def qmix_wide_fwd(w, s, q, q_tot, rows, N, S, E, bf16=False):
    lib = _lib.load()
    ws = WS.get("qmix_wide", lib.marl_qmix_wide_workspace(rows, N, S, 0), q.device)
    check(lib.marl_qmix_wide_fwd(C.byref(w), C.byref(s), _p(_f32(q)), _p(_f32(q_tot)), _p(ws), ws.numel() * 4, rows, N, S, E,
                                 1 if bf16 else 0, _stream()), "marl_qmix_wide_fwd")


def qmix_wide_bwd(w, s, q, dq_tot, dq, grads, rows, N, S, E, bf16=False, wgrad_bf16=None):
    lib = _lib.load()
    ws = WS.get("qmix_wide", lib.marl_qmix_wide_workspace(rows, N, S, 1), q.device)
    check(lib.marl_qmix_wide_bwd(C.byref(w), C.byref(s), _p(_f32(q)), _p(_f32(dq_tot)), _p(_f32(dq)), C.byref(grads), _p(ws),
                                 ws.numel() * 4, rows, N, S, E, _wide_flags(bf16, wgrad_bf16), _stream()), "marl_qmix_wide_bwd")


def uniform_stride(ts, align):
    """element stride between consecutive heads' fp32 tensors (one flat parameter buffer; 0 for a single head), None if it is
    not uniform, not positive or not a multiple of `align` bytes: 16 for the fused heads (vector loads), 4 for grouped marl_linear"""
    if len(ts) == 1:
        return 0
    d = [ts[i + 1].data_ptr() - ts[i].data_ptr() for i in range(len(ts) - 1)]
    if any(x != d[0] for x in d) or d[0] <= 0 or d[0] % align != 0:
        return None
    return d[0] // 4


def mlp3_weights(heads, grad=False):
    """heads: per head the nn.Linear layers of a Linear-ReLU-Linear-ReLU-Linear stack (or the two of a
    Linear-ReLU-Linear stack: w2 = NULL).  Returns the marl_mlp3_weights_t of head 0 + per-tensor head strides, or
    None when the heads are not laid out at constant strides / not 16-byte aligned (the caller then composes
    marl_linear)."""
    pick = (lambda p: p.grad) if grad else (lambda p: p.data)
    w = MarlMlp3Weights()
    keep = []
    names = (("w1", "b1"), ("w2", "b2"), ("w3", "b3")) if len(heads[0]) == 3 else (("w1", "b1"), ("w3", "b3"))
    for li, (wn, bn) in enumerate(names):
        for name, attr in ((wn, "weight"), (bn, "bias")):
            ts = [pick(getattr(h[li], attr)) for h in heads]
            if not _dense_on_device(ts[0], align=16) or not all(_dense_on_device(t) for t in ts):
                return None
            st = uniform_stride(ts, 16)
            if st is None:
                return None
            setattr(w, name, ts[0].data_ptr())
            setattr(w, "gs_" + name, st)
            keep.append(ts)
    w._keep = keep
    return w


def mlp3_wide_head(l0, l2, grad=False):
    """A two-layer head Linear(K1, 64) - ReLU - Linear(64, N3) with more outputs than one launch group holds (160), as
    ``groups`` column blocks that share layer 1: returns (marl_mlp3_weights_t, groups, outputs per group) or None."""
    pick = (lambda p: p.grad) if grad else (lambda p: p.data)
    ts = [pick(l0.weight), pick(l0.bias), pick(l2.weight), pick(l2.bias)]
    if not all(_dense_on_device(t, align=16) for t in ts):
        return None
    N3 = l2.out_features
    G = (N3 + 159) // 160
    if N3 % (4 * G) or l0.out_features != 64 or l2.in_features != 64:
        return None
    w = MarlMlp3Weights()
    w.w1, w.b1, w.w3, w.b3 = (t.data_ptr() for t in ts)
    w.gs_w1 = w.gs_b1 = 0
    w.gs_w3, w.gs_b3 = (N3 // G) * 64, N3 // G
    w._keep = ts
    return w, G, N3 // G


def mlp3_supported(x, K1, H1, H2, N3, groups):
    return bool(_lib.load().marl_mlp3_supported(C.byref(x), K1, H1, H2, N3, groups))


def mlp3_needs_kept(x, K1, N3=1):
    """True when the fused backward of this shape exists only for kept activations (K1 > 192 or more than 16 outputs)."""
    return bool(_lib.load().marl_mlp3_needs_kept(C.byref(x), K1, N3))


def _head_layout(Y, M, N3, groups):
    """(ld, group stride) of the head outputs: (M, groups*N3) with head g in columns [g*N3, (g+1)*N3), or
    (groups, M, N3) with one contiguous (M, N3) block per head."""
    if Y.dim() == 3:
        assert Y.shape == (groups, M, N3) and Y.is_contiguous()
        return N3, M * N3
    assert Y.dim() == 2 and Y.stride(1) == 1 and Y.shape[1] == groups * N3
    return Y.stride(0), N3


def mlp3_x6_supported(x, K1, H1, H2, N3, groups):
    """the bf16x6 split pair (csrc/mlp3_x6.hip) exists for this head shape"""
    return bool(_lib.load().marl_mlp3_x6_supported(C.byref(x), K1, H1, H2, N3, groups))


def mlp3_save_floats(M, three, groups):
    """floats of the kept-activation buffer of one fused head family (layout private to the kernels; the fp32 and the
    bf16x6 pair share it)."""
    return int(_lib.load().marl_mlp3_save_floats(M, 1 if three else 0, groups))


def mlp3_fwd(w, x, Y, M, K1, N3, groups, hsave=None, x6=False):
    """hsave (float32, >= mlp3_save_floats): keep the hidden activations for mlp3_bwd instead of recomputing them.
    x6: the bf16x6 split kernels (fp32-accurate products on the bf16 matrix cores; opt-in args.gemm_mode = "bf16x6")."""
    ld, gs = _head_layout(Y, M, N3, groups)
    assert src_width(x) == K1
    hp, hn = (_p(_f32(hsave)), hsave.numel()) if hsave is not None else (None, 0)
    fn = _lib.load().marl_mlp3_x6_fwd_save if x6 else _lib.load().marl_mlp3_fwd_save
    check(fn(C.byref(w), C.byref(x), _p(_f32(Y)), ld, gs, hp, hn, M, K1, N3, groups, _stream()),
          "marl_mlp3_x6_fwd" if x6 else "marl_mlp3_fwd")


def mlp3_bwd(w, x, dY, grads, M, K1, N3, groups, hsave=None, x6=False):
    lib = _lib.load()
    ld, gs = _head_layout(dY, M, N3, groups)
    assert src_width(x) == K1
    ws = WS.get("mlp3", lib.marl_mlp3_bwd_workspace(M, K1, N3, groups), dY.device)
    hp, hn = (_p(_f32(hsave)), hsave.numel()) if hsave is not None else (None, 0)
    fn = lib.marl_mlp3_x6_bwd_saved if x6 else lib.marl_mlp3_bwd_saved
    check(fn(C.byref(w), C.byref(x), _p(_f32(dY)), ld, gs, C.byref(grads), _p(ws), ws.numel() * 4,
             hp, hn, M, K1, N3, groups, _stream()), "marl_mlp3_x6_bwd" if x6 else "marl_mlp3_bwd")


MLP3_CALLS = ("fwd", "bwd", "x6_fwd", "x6_bwd")          # `what` of marl_mlp3_plan (include/marl_hip.h)
Mlp3Plan = collections.namedtuple("Mlp3Plan", "KC CF CFT kpad KV three wide n3t kept KH passes wgpc nst per grid lds yvec slabs")


def mlp3_plan(what, w, x, M, K1, N3, groups, Y=0, ld=None, gs=None, grads=None, hsave=None, hsave_floats=None, ws_bytes=None):
    """The launch plan of mlp3_fwd / mlp3_bwd (`what` in MLP3_CALLS) for these arguments, from the host functions the launches
    themselves decide with - no GPU.  None where the entry point refuses the call.  w / grads: MarlMlp3Weights (pointer fields may
    be integers standing for addresses); Y (dY for the backwards) / hsave: tensors or such integers; ld / gs default to the
    (M, groups * N3) layout; hsave_floats to mlp3_save_floats where hsave is given; ws_bytes to what mlp3_bwd() would pass now -
    the shared grow-only buffer, grown to this call's need."""
    lib = _lib.load()
    k = MLP3_CALLS.index(what)
    three = bool(w.w2)
    if ld is None or gs is None:
        ld0, gs0 = (_head_layout(Y, M, N3, groups) if isinstance(Y, torch.Tensor) else (groups * N3, N3))
        ld, gs = (ld0 if ld is None else ld), (gs0 if gs is None else gs)
    if hsave is not None and hsave_floats is None:
        hsave_floats = hsave.numel() if isinstance(hsave, torch.Tensor) else lib.marl_mlp3_save_floats(M, 1 if three else 0, groups)
    if ws_bytes is None:
        ws_bytes = lib.marl_mlp3_bwd_workspace(M, K1, N3, groups)
        have = WS.bufs.get("mlp3")
        if have is not None:
            ws_bytes = max((ws_bytes + 3) // 4 * 4, have.numel() * 4)
    plan = (C.c_int * 19)()
    if grads is None:
        grads = w
    if lib.marl_mlp3_plan(k, C.byref(w), C.byref(x), _pv(Y), ld, gs, C.byref(grads), ws_bytes, _pv(hsave), hsave_floats or 0,
                          M, K1, N3, groups, plan) != 0:
        return None
    p = tuple(plan)
    return Mlp3Plan(p[1], p[2], p[3], p[4], p[5], bool(p[6]), bool(p[7]), p[8], bool(p[9]), p[10], p[11], p[12], p[13], p[14],
                    p[15], p[16], bool(p[17]), p[18])


# ---- fused QTRAN-base heads (csrc/qtran_fused.hip)
def qtran_supported(N, A, AE):
    return bool(_lib.load().marl_qtran_supported(N, A, AE))


QTRAN_FIELDS = _linear_fields((k, k) for k in ("enc0", "enc2", "q2", "q4")) + [("q0_w", "q0.weight", torch.float32)]


def qtran_weights(t, S):
    """t: dict with the tensors of QTRAN_FIELDS - enc0 / enc2: hidden(_action)_encoding.{0,2}; q0 / q2 / q4: q.{0,2,4} (or
    hidden_encoding / v); q.0 gives its weight only -> marl_qtran_weights_t"""
    w = _fill_struct(MarlQtranWeights, t, QTRAN_FIELDS)
    w.q0_ld, w.q0_s = t["q0.weight"].shape[1], S
    return w


def qtran_head_fwd(w, hidden, u, sp, out, s1, e2, y1, y2, BT, N, A, AE):
    check(_lib.load().marl_qtran_head_fwd(C.byref(w), _p(_f32(hidden)), _p(u), _p(_f32(sp)), _p(_f32(out)), _p(s1), _p(e2),
                                          _p(y1), _p(y2), BT, N, A, AE, _stream()), "marl_qtran_head_fwd")


def _state_rows_ok(s):
    t = s.t if isinstance(s, Rows) else s
    return t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0 and t.dtype == torch.float32


def qtran_state_parts_supported(S, s=None):
    return bool(_lib.load().marl_qtran_state_parts_supported(S)) and (s is None or _state_rows_ok(s))


def qtran_state_parts(s, BT, S, sets):
    """sets: one or two (weight (64, >= S) row-major, bias (64), out (BT, 64)) triples evaluated on the same rows of s"""
    (W0, b0, o0), (W1, b1, o1) = sets[0], (sets[1] if len(sets) > 1 else (None, None, None))
    for W in (W0, W1):
        assert W is None or (W.stride(1) == 1 and W.dtype == torch.float32)
    x = src(s)
    check(_lib.load().marl_qtran_state_parts(C.byref(x), BT, S, len(sets), _p(W0), W0.stride(0), _p(_f32(b0)), _p(_f32(o0)),
                                             _p(W1), W1.stride(0) if W1 is not None else 0, _p(b1), _p(o1), _stream()),
          "marl_qtran_state_parts")


def qtran_wgrad_rows_supported(S, AE, s=None):
    return bool(_lib.load().marl_qtran_wgrad_rows_supported(S, AE)) and (s is None or _state_rows_ok(s))


def qtran_wgrad_rows(s, s1, e2, y1, y2, d_out, dy1, dy2, de2, d_q0_w, d_q0_b, d_q2_w, d_q2_b, d_q4_w, d_q4_b, d_enc2_w,
                     BT, S, AE):
    lib = _lib.load()
    ws = WS.get("qtran_wg", lib.marl_qtran_wgrad_rows_workspace(S, AE), s.device)
    assert d_q0_w.stride(1) == 1 and d_q2_w.is_contiguous() and d_enc2_w.is_contiguous()
    x = src(s)
    check(lib.marl_qtran_wgrad_rows(C.byref(x), _p(_f32(s1)), _p(_f32(e2)), _p(_f32(y1)), _p(_f32(y2)), _p(_f32(d_out)),
                                    _p(_f32(dy1)), _p(_f32(dy2)), _p(_f32(de2)), _p(d_q0_w), d_q0_w.stride(0), _p(_f32(d_q0_b)),
                                    _p(_f32(d_q2_w)), _p(_f32(d_q2_b)), _p(_f32(d_q4_w)), _p(_f32(d_q4_b)), _p(_f32(d_enc2_w)),
                                    _p(ws), ws.numel() * 4, BT, S, AE, _stream()), "marl_qtran_wgrad_rows")


QTRAN_PLANS = ("fwd", "fwd2", "bwd", "state_parts", "qmix_tail", "wgrad_rows")          # `what` of marl_qtran_plan (include/marl_hip.h)
QtranHeadPlan = collections.namedtuple("QtranHeadPlan", "FT hot dual grid lds rounds slabs lds_agents")
QtranStatePlan = collections.namedtuple("QtranStatePlan", "KCT nsets grid lds rounds")
QtranWgradPlan = collections.namedtuple("QtranWgradPlan", "FT SMAX ntiles grid lds rounds slabs")


def qtran_plan(what, BT, N=1, A=0, AE=64, S=4, nsets=1):
    """The launch plan of a qtran_fused.hip entry point (`what` in QTRAN_PLANS) for these sizes, from the host functions the launches
    themselves decide with - no GPU.  None where the entry point refuses the sizes.
      fwd / fwd2 / bwd (BT, N, A, AE)            QtranHeadPlan(FT, hot, dual, grid, lds, rounds, slabs, lds_agents)
      state_parts (BT, S, nsets) / qmix_tail    QtranStatePlan(KCT, nsets, grid, lds, rounds)
      wgrad_rows (BT, S, AE)                     QtranWgradPlan(FT, SMAX, ntiles, grid, lds, rounds, slabs)"""
    k = QTRAN_PLANS.index(what)
    plan = (C.c_int * 8)()
    if _lib.load().marl_qtran_plan(k, BT, N, A, AE, S, nsets, plan) != 0:
        return None
    p = tuple(plan)
    if k <= 2:
        return QtranHeadPlan(p[0], bool(p[1]), bool(p[2]), p[3], p[4], p[5], p[6], p[7])
    if k <= 4:
        return QtranStatePlan(p[0], p[1], p[3], p[4], p[5])
    return QtranWgradPlan(p[0], p[1], p[2], p[3], p[4], p[5], p[6])


def qtran_head_fwd2(w, hidden, u, u2, sp, out, out2, s1, e2, y1, y2, BT, N, A, AE):
    check(_lib.load().marl_qtran_head_fwd2(C.byref(w), _p(_f32(hidden)), _p(_i32(u)), _p(_i32(u2)), _p(_f32(sp)), _p(_f32(out)),
                                           _p(_f32(out2)), _p(s1), _p(e2), _p(y1), _p(y2), BT, N, A, AE, _stream()),
          "marl_qtran_head_fwd2")


def qtran_head_bwd(w, hidden, u, d_out, y1, y2, dy1, dy2, de2, dhidden, accumulate, d_enc0_w, d_enc0_b, d_enc2_b,
                   BT, N, A, AE):
    lib = _lib.load()
    ws = WS.get("qtran", lib.marl_qtran_bwd_workspace(BT, AE), hidden.device)
    check(lib.marl_qtran_head_bwd(C.byref(w), _p(_f32(hidden)), _p(u), _p(_f32(d_out)), _p(_f32(y1)), _p(_f32(y2)),
                                  _p(_f32(dy1)), _p(_f32(dy2)), _p(_f32(de2)), _p(_f32(dhidden)), 1 if accumulate else 0,
                                  _p(_f32(d_enc0_w)), _p(_f32(d_enc0_b)), _p(_f32(d_enc2_b)), _p(ws), ws.numel() * 4,
                                  BT, N, A, AE, _stream()), "marl_qtran_head_bwd")


# ---- RTW reflection head (csrc/rtw_head.hip)
RTW_KEYS = (("t0", "teammate_net.0"), ("t2", "teammate_net.2"), ("w0", "world_net.0"), ("w2", "world_net.2"),
            ("wq", "w_q"), ("wk", "w_k"), ("v0", "w_v.0"), ("v2", "w_v.2"))


def rtw_supported(N, O, A, H=64, hidden_dim=64, attn_dim=64):
    return bool(_lib.load().marl_rtw_supported(N, O, A, H, hidden_dim, attn_dim))


def rtw_weights(params):
    """params: dict name -> tensor with RTWAgent keys (network/RTW.py:24-56) -> marl_rtw_weights_t."""
    return _fill_struct(MarlRtwWeights, params, _linear_fields(RTW_KEYS))


def rtw_head_act(w, h, obs, obs_bs, obs_t0, avail, av_bs, av_t0, q, E, N, O, A, not_self_model=True, a_out=None,
                 ohat_out=None):
    """q (E*N, A) += the act-mode reflection term (RTWAgent.forward test_mode=True, network/RTW.py:70-119)."""
    check(_lib.load().marl_rtw_head_act(C.byref(w), _p(_f32(h)), _p(_f32(obs)), obs_bs, obs_t0, _p(_f32(avail)), av_bs, av_t0,
                                        _p(_f32(q)), _p(_i32(a_out)) if a_out is not None else None,
                                        _p(_f32(ohat_out)) if ohat_out is not None else None, E, N, O, A,
                                        1 if not_self_model else 0, _stream()), "marl_rtw_head_act")


def rtw_head_given(w, hs, obs, obs_bs, obs_t0, obs_next, on_bs, on_t0, u, u_bs, u_t0, q, B, T, N, O, A, not_self_model=True):
    """q (B,T,N,A) += the given-mode reflection term (RTWAgent.forward target=False, network/RTW.py:121-203)."""
    check(_lib.load().marl_rtw_head_given(C.byref(w), _p(_f32(hs)), _p(_f32(obs)), obs_bs, obs_t0, _p(_f32(obs_next)), on_bs,
                                          on_t0, _p(_i32(u)), u_bs, u_t0, _p(_f32(q)), B, T, N, O, A,
                                          1 if not_self_model else 0, _stream()), "marl_rtw_head_given")


# ---- world-model head (csrc/world_head.hip)
WORLD_KEYS = (("h0", "world.hidden_embd.0"), ("h2", "world.hidden_embd.2"), ("r", "world.r_out"), ("o", "world.o_out"),
              ("t", "world.terminate_out"))


def world_supported(N, O, A, H=64):
    return bool(_lib.load().marl_world_supported(N, O, A, H))


def world_weights(params):
    """params: dict name -> tensor with world_model.Agent keys (network/world_model.py:12-19) -> marl_world_weights_t."""
    return _fill_struct(MarlWorldWeights, params, _linear_fields(WORLD_KEYS))


def world_grads(grads):
    """grads: dict name -> gradient tensor with the same keys (terminate_out not needed) -> marl_world_grads_t."""
    return _fill_struct(MarlWorldGrads, grads, _linear_fields(WORLD_KEYS[:4]))


def world_head_fwd(w, h, q, B, T, N, O, A, r_out=None, ohat_out=None, tau_out=None, obs=None, obs_bs=0, obs_t0=0,
                   ep_len=None, ep_map=None, loss=None):
    """q (B*T*N, A) += r (network/world_model.py:71; q may be None).  With `loss` (a one-float device view, e.g. a slot of the
    loss statistics): train mode, loss += sum (o_hat - o_next)^2 with o_next read through (obs, obs_bs, obs_t0, ep_len, ep_map)."""
    lib = _lib.load()
    ws = None
    if loss is not None:
        ws = WS.get("world_fwd", lib.marl_world_fwd_workspace(B, T, N), h.device)
    check(lib.marl_world_head_fwd(C.byref(w), _p(_f32(h)), _p(_f32(q)) if q is not None else None, _p(r_out), _p(ohat_out),
                                  _p(tau_out), _p(_f32(obs)) if obs is not None else None, obs_bs, obs_t0,
                                  _p(_i32(ep_len)) if ep_len is not None else None,
                                  _p(_i32(ep_map)) if ep_map is not None else None, _p(_f32(loss)) if loss is not None else None,
                                  _p(ws), 0 if ws is None else ws.numel() * 4, B, T, N, O, A, _stream()),
          "marl_world_head_fwd")


def world_head_bwd(w, g, hs, dq_idx, dq_val, obs, obs_bs, obs_t0, den, dscale, dhs, B, T, N, O, A, ep_len=None, ep_map=None):
    """dhs (B*T*N, 64) = gradient on hs; the head's weight gradients accumulate into `g` (marl_world_grads_t)."""
    lib = _lib.load()
    ws = WS.get("world_bwd", lib.marl_world_bwd_workspace(B, T, N, O, A), hs.device)
    check(lib.marl_world_head_bwd(C.byref(w), C.byref(g), _p(_f32(hs)), _p(_i32(dq_idx)) if dq_idx is not None else None,
                                  _p(_f32(dq_val)) if dq_val is not None else None, _p(_f32(obs)), obs_bs, obs_t0,
                                  _p(_i32(ep_len)) if ep_len is not None else None,
                                  _p(_i32(ep_map)) if ep_map is not None else None, _p(_f32(den)) if den is not None else None,
                                  float(dscale), _p(_f32(dhs)), _p(ws), ws.numel() * 4, B, T, N, O, A, _stream()),
          "marl_world_head_bwd")


# ---- MAIC message head (csrc/maic_head.hip, csrc/maic_head_bwd.hip)
MAIC_KEYS = (("e0", "embed_net.0"), ("e3", "embed_net.3"), ("m0", "msg_net.0"), ("m2", "msg_net.2"), ("k", "w_key"),
             ("q", "w_query"))
MAIC_BN = (("bn_w", "embed_net.1.weight", torch.float32), ("bn_b", "embed_net.1.bias", torch.float32),
           ("bn_rm", "embed_net.1.running_mean", torch.float32), ("bn_rv", "embed_net.1.running_var", torch.float32),
           ("bn_nbt", "embed_net.1.num_batches_tracked", torch.int64))


def maic_supported(N, O, A, H=64, NH=64, L=8, D=32):
    return bool(_lib.load().marl_maic_supported(N, O, A, H, NH, L, D))


def maic_weights(tensors):
    """tensors: dict name -> tensor with MAICAgent's parameter and buffer keys (network/MAIC.py:19-47) -> marl_maic_weights_t."""
    return _fill_struct(MarlMaicWeights, tensors, _linear_fields(MAIC_KEYS) + list(MAIC_BN))


def maic_head_fwd(w, h, q, bs, N, A, test_mode=True, bn_batch=False, eps=None, var_floor=0.002, bn_eps=1e-5, bn_momentum=0.1,
                  mean_out=None, var_out=None, lat_out=None, alpha_out=None, msg_out=None):
    """q (bs*N, A) += the gated messages of MAICAgent.forward (network/MAIC.py:58-87) from h (bs*N, 64).  ``eps`` (bs*N, N*8):
    the noise of the sampled latents (test_mode False).  ``bn_batch``: BatchNorm on the statistics of this call's rows, with
    the running statistics in ``w`` updated, instead of on the running statistics."""
    lib = _lib.load()
    if not lib.marl_maic_supported(N, 1, A, 64, 64, 8, 32):
        raise ValueError("the gfx950 MAIC head covers N <= 16 and A <= 32 (N %d, A %d)" % (N, A))
    if not test_mode and eps is None:
        raise ValueError("sampled latents (test_mode=False) need eps")
    if bn_batch and bs * N < 2:
        raise ValueError("Expected more than 1 value per channel when training, got %d row(s)" % (bs * N))
    for t, cols in ((h, 64), (q, A)):
        assert t.is_contiguous() and t.numel() == bs * N * cols
    if eps is not None:
        assert eps.is_contiguous() and eps.numel() == bs * N * N * 8
    ws = WS.get("maic", lib.marl_maic_workspace(bs, N), h.device) if bn_batch else None
    opt = [None if t is None else _p(_f32(t)) for t in (mean_out, var_out, lat_out, alpha_out, msg_out)]
    check(lib.marl_maic_head_fwd(C.byref(w), _p(_f32(h)), _p(_f32(q)), _p(_f32(eps)) if eps is not None else None, *opt,
                                 _p(ws), 0 if ws is None else ws.numel() * 4, bs, N, A, 1 if test_mode else 0,
                                 1 if bn_batch else 0, float(var_floor), float(bn_eps), float(bn_momentum), _stream()),
          "marl_maic_head_fwd")


def maic_grads(grads):
    """grads: dict name -> gradient tensor with MAICAgent's parameter keys (the head's layers; inference_net not needed) ->
    marl_maic_grads_t."""
    return _fill_struct(MarlMaicGrads, grads, _linear_fields(MAIC_KEYS) + list(MAIC_BN[:2]))


def maic_head_bwd(w, g, h, u_act, dq_val, dh, bs, N, A, test_mode=False, bn_batch=False, eps=None, var_floor=0.002, bn_eps=1e-5,
                  dpar_extra=None):
    """Backward of maic_head_fwd for the sparse gradient (u_act, dq_val) on return_q, one pair per row (csrc/maic_head_bwd.hip):
    dh (bs*N, 64) = the head's contribution to the gradient on h; the head's weight gradients accumulate into ``g``
    (marl_maic_grads_t).  ``eps`` and the mode flags as the forward call had them; the running statistics are not moved.
    ``dpar_extra`` (bs*N, 2*N*8): a further gradient on embed_net's post-clamp [mean | var] planes (maic_aux's), carried through
    the same embed_net backward; rows without a TD pair still receive it."""
    lib = _lib.load()
    if not lib.marl_maic_supported(N, 1, A, 64, 64, 8, 32):
        raise ValueError("the gfx950 MAIC head covers N <= 16 and A <= 32 (N %d, A %d)" % (N, A))
    if not test_mode and eps is None:
        raise ValueError("sampled latents (test_mode=False) need the eps of the forward call")
    if bn_batch and bs * N < 2:
        raise ValueError("Expected more than 1 value per channel when training, got %d row(s)" % (bs * N))
    for t, cols in ((h, 64), (dh, 64), (u_act, 1), (dq_val, 1)):
        assert t.is_contiguous() and t.numel() == bs * N * cols
    if eps is not None:
        assert eps.is_contiguous() and eps.numel() == bs * N * N * 8
    ws = WS.get("maic_bwd", lib.marl_maic_bwd_workspace(bs, N, A), h.device)
    e = _p(_f32(eps)) if eps is not None and not test_mode else None
    tail = (_p(_f32(dh)), _p(ws), ws.numel() * 4, bs, N, A, 1 if test_mode else 0, 1 if bn_batch else 0, float(var_floor),
            float(bn_eps), _stream())
    if dpar_extra is None:
        check(lib.marl_maic_head_bwd(C.byref(w), C.byref(g), _p(_f32(h)), e, _p(_i32(u_act)), _p(_f32(dq_val)), *tail),
              "marl_maic_head_bwd")
        return
    assert dpar_extra.is_contiguous() and dpar_extra.numel() == bs * N * 2 * N * 8
    check(lib.marl_maic_head_bwd_ex(C.byref(w), C.byref(g), _p(_f32(h)), e, _p(_i32(u_act)), _p(_f32(dq_val)),
                                    _p(_f32(dpar_extra)), *tail), "marl_maic_head_bwd_ex")


# ---- MAIC auxiliary losses (csrc/maic_aux.hip)
MAIC_INFER_KEYS = (("i0", "inference_net.0"), ("i3", "inference_net.3"))
MAIC_INFER_BN = (("ibn_w", "inference_net.1.weight", torch.float32), ("ibn_b", "inference_net.1.bias", torch.float32),
                 ("ibn_rm", "inference_net.1.running_mean", torch.float32), ("ibn_rv", "inference_net.1.running_var", torch.float32),
                 ("ibn_nbt", "inference_net.1.num_batches_tracked", torch.int64))


def maic_infer_weights(tensors):
    """tensors: dict name -> tensor with MAICAgent's inference_net parameter and buffer keys -> marl_maic_infer_t."""
    return _fill_struct(MarlMaicInfer, tensors, _linear_fields(MAIC_INFER_KEYS) + list(MAIC_INFER_BN))


def maic_infer_grads(grads):
    """grads: dict name -> gradient tensor with inference_net's parameter keys -> marl_maic_infer_grads_t."""
    return _fill_struct(MarlMaicInferGrads, grads, _linear_fields(MAIC_INFER_KEYS) + list(MAIC_INFER_BN[:2]))


def maic_aux(w, iw, g, ig, h, return_q, bs, N, A, mi_weight, entropy_weight, mi_out, ent_out, dpar, dh, test_mode=False,
             bn_batch=False, eps=None, den=None, dscale=1.0, var_floor=0.002, bn_eps=1e-5, bn_momentum=0.1):
    """The MI and the entropy loss of MAICAgent (network/MAIC.py:88-123) with their gradients, one call (csrc/maic_aux.hip).
    mi_out / ent_out (one-float device views, e.g. slots of the loss statistics) += the two weighted losses; dpar
    (bs*N, 2*N*8) = the MI gradient on embed_net's post-clamp [mean | var] planes (-> maic_head_bwd's dpar_extra); dh (bs*N, 64) =
    the MI gradient on h through inference_net's input; inference_net's gradients accumulate into ``ig``, the entropy term's
    into w_key / w_query of ``g``.  Gradients are scaled by den[0] * dscale (den None: dscale).  ``h``, ``eps`` and the mode flags
    as the head's forward call had them, ``return_q`` its output.  bn_batch: inference_net.1's running statistics move once
    (mi_weight > 0); embed_net.1's are never written."""
    lib = _lib.load()
    if not lib.marl_maic_supported(N, 1, A, 64, 64, 8, 32):
        raise ValueError("the gfx950 MAIC head covers N <= 16 and A <= 32 (N %d, A %d)" % (N, A))
    if not test_mode and eps is None:
        raise ValueError("sampled latents (test_mode=False) need the eps of the forward call")
    if bn_batch and bs * N < 2:
        raise ValueError("Expected more than 1 value per channel when training, got %d row(s)" % (bs * N))
    for t, cols in ((h, 64), (dh, 64), (return_q, A), (dpar, 2 * N * 8)):
        assert t.is_contiguous() and t.numel() == bs * N * cols
    if eps is not None:
        assert eps.is_contiguous() and eps.numel() == bs * N * N * 8
    ws = WS.get("maic_aux", lib.marl_maic_aux_workspace(bs, N, A), h.device)
    check(lib.marl_maic_aux(C.byref(w), C.byref(iw), C.byref(g), C.byref(ig), _p(_f32(h)),
                            _p(_f32(eps)) if eps is not None and not test_mode else None, _p(_f32(return_q)), float(mi_weight),
                            float(entropy_weight), _p(_f32(den)) if den is not None else None, float(dscale), _p(_f32(mi_out)),
                            _p(_f32(ent_out)), _p(_f32(dpar)), _p(_f32(dh)), _p(ws), ws.numel() * 4, bs, N, A,
                            1 if test_mode else 0, 1 if bn_batch else 0, float(var_floor), float(bn_eps), float(bn_momentum),
                            _stream()), "marl_maic_aux")


def maic_noise(rseed, env0, tg, eps, E, N):
    """eps (E*N, N*8) <- the standard-normal draws of lock-step ``tg`` (counter hash + Box-Muller, csrc/maic_head.hip)"""
    assert eps.is_contiguous() and eps.numel() == E * N * N * 8
    check(_lib.load().marl_maic_noise(rseed & 0xFFFFFFFF, env0, tg & 0xFFFFFFFF, _p(_f32(eps)), E, N, _stream()),
          "marl_maic_noise")
