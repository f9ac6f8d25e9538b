"""MAVEN on the MI355X against tests/maven_oracle.py.  Needs a real MI355X: ``pytest -m gpu``.

Kernel level (csrc/maven.hip): the noise draw against its restatement; the head forward and backward and the MI pass against float64
at the issue's shapes - NaN in what an entry may not read, sentinels after every output, gradients accumulated onto a random base, two
calls to equal bits -, parity.close at 1e-4 * max|ref|; refusals that launch nothing.  Learner level: two updates of MAVENLearner
beside the oracle learner on 2s3z-, MMM2- and matrix-shaped batches with the bounds of tests/test_gpu_learners.py (the tensors
maven_oracle.F32_EXCEPTIONS lists: four times their CPU figure), the bit-for-bit start from QLearner(qmix, no_loss_fold), and the
launcher end to end on the synthetic and the battle environment."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest
import torch

from oracle import seeded, learners
import maven_oracle as mo
import parity

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 777.0
INVALID = 1          # hipErrorInvalidValue
TAIL = 5             # sentinel elements after every output
up = lambda x: torch.tensor(np.ascontiguousarray(x), device=DEV)
t32 = lambda d: {k: torch.tensor(x) for k, x in d.items()}


def out_buf(n, dtype=torch.float32):
    """n elements followed by TAIL sentinels, all holding the sentinel"""
    return torch.full((n + TAIL,), SENT, dtype=dtype, device=DEV)


def tail_ok(buf, n):
    return bool((buf[n:] == SENT).all())


def scaled_base(base, ref):
    """the random base a gradient is accumulated onto, scaled to the float64 gradient's size (max|base| = max|ref|): got - base is then
    held to 1e-4 * max|ref| itself, the base's own fp32 rounding being 2^-24 of that.  A gradient that is all zeros keeps the base as
    drawn: adding nothing to it must give it back exactly"""
    out = {}
    for k, b in base.items():
        m = float(np.abs(ref[k]).max())
        out[k] = (b * (m / float(np.abs(b).max()))).astype(np.float32) if m > 0 else b
    return out


# ------------------------------------------------------------------------------------------------ noise
@pytest.mark.parametrize("E", [1, 5, 257])
@pytest.mark.parametrize("K", [1, 3, 16, 32])
def test_noise_draw(E, K):
    from marl_amd import ops
    for rseed, env0, tg0 in ((123, 0, 0), (0xDEADBEEF, 7, 121 * 3)):
        buf = out_buf(E, torch.int32)
        ops.maven_noise(rseed, env0, tg0, K, buf, E)
        torch.cuda.synchronize()
        assert np.array_equal(buf[:E].cpu().numpy(), mo.noise_draw(rseed, env0, tg0, K, E)) and tail_ok(buf, E)


# ------------------------------------------------------------------------------------------------ head
def _head_setup(c):
    from marl_amd import ops
    tab = {"maven." + k: up(v) for k, v in c.tables.items()}
    grads = {"maven." + k: up(v) for k, v in c.base.items()}
    return ops, ops.maven_weights(tab), ops.maven_grads(grads), grads


@pytest.mark.parametrize("shape", mo.HEAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_head_forward_and_backward_vs_float64(shape):
    B, T, N, A, K = shape
    c = mo.head_case(*shape)
    o = mo.head_oracle(c)
    ops, w, g, grads = _head_setup(c)
    case = "maven_head:%s" % "x".join(map(str, shape))
    R = B * T * N
    hs, noise = up(c.hs), up(c.noise)
    # ---- forward: q += the term; the rows of an episode with noise out of range are untouched
    runs = []
    for _ in range(2):
        q = out_buf(R * A)
        q[:R * A] = up(c.q).reshape(-1)
        ops.maven_head_fwd(w, hs, noise, q, B, T, N, A, K)
        torch.cuda.synchronize()
        assert tail_ok(q, R * A)
        runs.append(q[:R * A].clone())
    assert torch.equal(runs[0], runs[1])
    got = runs[0].view(B, T, N, A).cpu().numpy()
    parity.close(case, "q", got, o.q_out)
    assert np.array_equal(got[c.skipped], c.q[c.skipped])
    # ---- backward: with and without the dense part
    for dense in (True, False):
        od = o if dense else mo.head_oracle(c, dense=False)
        base = scaled_base(c.base, od.grads)
        runs = []
        for _ in range(2):
            for k, v in base.items():
                grads["maven." + k].copy_(up(v))
            dq_out, dhs = out_buf(R * A), out_buf(R * 64)
            ops.maven_head_bwd(w, g, hs, noise, up(c.dq_idx), up(c.dq_val), up(c.dq_dense) if dense else None, dq_out, dhs, B, T, N, A, K)
            torch.cuda.synchronize()
            assert tail_ok(dq_out, R * A) and tail_ok(dhs, R * 64)
            runs.append([dq_out[:R * A].clone(), dhs[:R * 64].clone()] + [grads["maven." + k].clone() for k in mo.TABLES])
        assert all(torch.equal(x, y) for x, y in zip(*runs))
        tag = "" if dense else "/sparse"
        parity.close(case, "dq_out" + tag, runs[0][0].view(B, T, N, A).cpu().numpy(), od.g)
        parity.close(case, "dhs" + tag, runs[0][1].view(B, T, N, 64).cpu().numpy(), od.dhs)
        assert bool((runs[0][1].view(B, T, N, 64)[torch.tensor(c.skipped)] == 0).all())
        for k, x in zip(mo.TABLES, runs[0][2:]):
            ref = od.grads[k]
            parity.close(case, "grad " + k + tag, x.cpu().numpy().astype(np.float64) - base[k], ref)
    plan = ops.maven_plan(B, T, N, A, K, 8)
    assert plan[0] == (T + 15) // 16 and plan[1] == B * N * plan[0] and plan[2] == min(B, 256)


def test_head_forward_with_zero_tables_leaves_q_alone():
    c = mo.head_case(3, 17, 5, 11, 16)
    c.tables = {k: np.zeros_like(v) for k, v in c.tables.items()}
    c.hs = np.nan_to_num(c.hs)
    c.noise[-1] = 2
    ops, w, _, _ = _head_setup(c)
    q = up(c.q)
    ops.maven_head_fwd(w, up(c.hs), up(c.noise), q, 3, 17, 5, 11, 16)
    assert bool((q.cpu() == torch.tensor(c.q)).all())


# ------------------------------------------------------------------------------------------------ MI pass
def _mi_call(ops, c, d, g, lam, dq, ce, stats, **over):
    a = dict(q=up(c.q), avail=up(c.avail_store), avail_bs=c.Ts * c.N * c.A, state=up(c.state_store).view(-1, c.ld), state_ld=c.ld,
             state_bs=c.Ts, ep_map=up(c.ep_map), noise=up(c.noise), padded=up(c.padded).view(-1))
    a.update(over)
    ops.maven_mi(d, g, a["q"], a["avail"], a["avail_bs"], a["state"], a["state_ld"], a["state_bs"], a["ep_map"], a["noise"], a["padded"],
                 lam, dq, ce, stats, c.B, c.T, c.N, c.A, c.S, c.K)


@pytest.mark.parametrize("lam", [0.001, 1.0])
@pytest.mark.parametrize("shape", mo.MI_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mi_pass_vs_float64(shape, lam):
    """Slabs: a workgroup owns one slab and a 16-step tile is the unit of work, so a case has min(ceil(B T / 16), 256) slabs.  Of the
    issue's five shapes 1x1, 2x7 and 1x3 have at most 16 steps - one tile, one slab: they cannot take the reduce over several slabs;
    3x17 (four slabs) and 2x9 (two) do, and test_mi_pass_many_slabs_and_tiles walks 256 slabs of several tiles each."""
    from marl_amd import ops
    B, T, N, A, S, K = shape
    c = mo.mi_case(*shape)
    o = mo.mi_oracle(c, lam)
    case = "maven_mi:%s/lam%g" % ("x".join(map(str, shape)), lam)
    names = [k for k, _ in mo.disc_shapes(N, A, S, K)]
    disc = {k: up(c.disc[k]) for k in names}
    grads = {k: up(c.base[k]) for k in names}
    d, g = ops.maven_disc(disc), ops.maven_disc_grads(grads)
    plan = ops.maven_plan(B, T, N, A, K, S)
    assert plan[3] == (B * T + 15) // 16 and plan[4] == min(plan[3], 256) and (B * T <= 16 or plan[4] >= 2)      # two slabs where two tiles
    assert c.ld > S and c.ep_map.tolist() != list(range(B))
    R = B * T * N * A
    base = scaled_base(c.base, o.grads)
    runs = []
    for _ in range(2):
        for k in names:
            grads[k].copy_(up(base[k]))
        dq, ce, stats = out_buf(R), out_buf(B * T), out_buf(2)
        stats[:2] = up(c.stats_base)
        _mi_call(ops, c, d, g, lam, dq, ce, stats[:2])
        torch.cuda.synchronize()
        assert tail_ok(dq, R) and tail_ok(ce, B * T) and tail_ok(stats, 2)
        runs.append([dq[:R].clone(), ce[:B * T].clone(), stats[:2].clone()] + [grads[k].clone() for k in names])
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    dq, ce, stats = (x.cpu().numpy() for x in runs[0][:3])
    dq, dead = dq.reshape(B, T, N, A), c.padded == 1
    assert np.isfinite(dq).all() and np.isfinite(ce).all()
    assert (dq[dead] == 0).all() and (dq[(np.nan_to_num(c.avail) == 0) & ~dead[..., None, None]] == 0).all()      # exact zeros
    assert (dq[0, 0, 0] == 0).all()                                                                             # one available action
    parity.close(case, "ce", ce.reshape(B, T), o.ce)
    parity.close(case, "sum m ce", stats[0] - c.stats_base[0], o.stats[0])
    assert stats[1] - c.stats_base[1] == o.stats[1]
    parity.close(case, "dq_dense", dq, o.dq_dense)
    for k, x in zip(names, runs[0][3:]):
        ref = o.grads[k]
        parity.close(case, "grad " + k, x.cpu().numpy().astype(np.float64) - base[k], ref)


def test_mi_pass_many_slabs_and_tiles():
    """B T = 4112 steps: 257 tiles on the 256-slab cap, so workgroup 0 walks two tiles and every slab enters the reduce"""
    from marl_amd import ops
    B, T, N, A, S, K = shape = (16, 257, 2, 3, 5, 3)
    c = mo.mi_case(*shape, seed=3)       # (of seeds 0 .. 7 the one whose smallest live |ReLU pre-activation| is largest: 1.2e-5, float64)
    o = mo.mi_oracle(c, 1.0)
    plan = ops.maven_plan(B, T, N, A, K, S)
    assert plan[3] == 257 and plan[4] == 256 and plan[6] == 2
    names = [k for k, _ in mo.disc_shapes(N, A, S, K)]
    base = scaled_base(c.base, o.grads)
    grads = {k: up(base[k]) for k in names}
    dq, ce, stats = out_buf(B * T * N * A), out_buf(B * T), torch.zeros(2, device=DEV)
    _mi_call(ops, c, ops.maven_disc({k: up(c.disc[k]) for k in names}), ops.maven_disc_grads(grads), 1.0, dq, ce, stats)
    case = "maven_mi:many_slabs"
    parity.close(case, "sum m ce", stats[0].item(), o.stats[0])
    assert stats[1].item() == o.stats[1]
    parity.close(case, "dq_dense", dq[:B * T * N * A].view(B, T, N, A).cpu().numpy(), o.dq_dense)
    for k in names:
        parity.close(case, "grad " + k, grads[k].cpu().numpy().astype(np.float64) - base[k], o.grads[k])


def test_mi_pass_on_dense_inputs_without_a_map():
    """the layout a dict batch has: dense availability and state, no episode map"""
    from marl_amd import ops
    B, T, N, A, S, K = shape = (3, 17, 5, 11, 120, 16)
    c = mo.mi_case(*shape)
    o = mo.mi_oracle(c, 1.0)
    names = [k for k, _ in mo.disc_shapes(N, A, S, K)]
    grads = {k: torch.zeros_like(up(c.base[k])) for k in names}
    dq, ce, stats = out_buf(B * T * N * A), out_buf(B * T), torch.zeros(2, device=DEV)
    _mi_call(ops, c, ops.maven_disc({k: up(c.disc[k]) for k in names}), ops.maven_disc_grads(grads), 1.0, dq, ce, stats,
             avail=up(c.avail), avail_bs=T * N * A, state=up(c.state).view(B * T, S), state_ld=S, state_bs=T, ep_map=None)
    parity.close("maven_mi:dense", "dq_dense", dq[:B * T * N * A].view(B, T, N, A).cpu().numpy(), o.dq_dense)
    for k in names:
        parity.close("maven_mi:dense", "grad " + k, grads[k].cpu().numpy(), o.grads[k])


# ------------------------------------------------------------------------------------------------ refusals
def _ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def test_refusals_launch_nothing():
    from marl_amd import ops, _lib
    lib = _lib.load()
    # ---- head
    c = mo.head_case(3, 17, 5, 11, 16)
    c.hs = np.nan_to_num(c.hs)
    _, w, g, grads = _head_setup(c)
    R = 3 * 17 * 5
    hs, noise, q = up(c.hs), up(c.noise), out_buf(R * 11)
    dq_out, dhs = out_buf(R * 11), out_buf(R * 64)
    ws = out_buf(lib.marl_maven_bwd_workspace(3, 5, 11, 16) // 4)
    idx, val = up(c.dq_idx), up(c.dq_val)

    def fwd(**o):
        a = dict(w=C.byref(w), hs=_ptr(hs), noise=_ptr(noise), q=_ptr(q), B=3, T=17, N=5, A=11, K=16)
        a.update(o)
        return lib.marl_maven_head_fwd(a["w"], a["hs"], a["noise"], a["q"], a["B"], a["T"], a["N"], a["A"], a["K"], None)

    def bwd(**o):
        a = dict(w=C.byref(w), g=C.byref(g), hs=_ptr(hs), noise=_ptr(noise), idx=_ptr(idx), val=_ptr(val), dense=None, dq_out=_ptr(dq_out),
                 dhs=_ptr(dhs), ws=_ptr(ws), wsb=(ws.numel() - TAIL) * 4, B=3, T=17, N=5, A=11, K=16)
        a.update(o)
        return lib.marl_maven_head_bwd(a["w"], a["g"], a["hs"], a["noise"], a["idx"], a["val"], a["dense"], a["dq_out"], a["dhs"], a["ws"],
                                       C.c_size_t(a["wsb"]), a["B"], a["T"], a["N"], a["A"], a["K"], None)
    shapes_bad = [dict(N=0), dict(N=17), dict(A=0), dict(A=33), dict(K=0), dict(K=33), dict(B=1 << 15, T=1 << 15, N=2), dict(B=-1)]
    off = C.c_void_p(hs.data_ptr() + 4)                                # a base off its 16-byte boundary
    for o in shapes_bad + [dict(w=None), dict(hs=None), dict(noise=None), dict(q=None), dict(hs=off)]:
        assert fwd(**o) == INVALID, o
    for o in shapes_bad + [dict(w=None), dict(g=None), dict(hs=None), dict(noise=None), dict(dq_out=None), dict(dhs=None), dict(ws=None),
                           dict(wsb=16), dict(idx=None), dict(val=None), dict(hs=off)]:
        assert bwd(**o) == INVALID, o
    for o in (dict(B=0), dict(T=0)):
        assert fwd(**o) == 0 and bwd(**o) == 0, o
    base = {k: v.clone() for k, v in grads.items()}
    torch.cuda.synchronize()
    assert all(bool((x == SENT).all()) for x in (q, dq_out, dhs, ws)) and all(torch.equal(base[k], grads[k]) for k in base)
    assert fwd() == 0 and bwd() == 0                                   # and the same arguments, unchanged, run
    torch.cuda.synchronize()
    # (the last episode's noise is out of range: its q rows stay as they are)
    assert not bool((q[:2 * 17 * 5 * 11] == SENT).any()) and bool((q[2 * 17 * 5 * 11:] == SENT).all())
    assert not bool((dhs[:R * 64] == SENT).any()) and tail_ok(ws, ws.numel() - TAIL)
    # ---- noise
    nz = out_buf(5, torch.int32)
    for K in (0, 33, -1):
        assert lib.marl_maven_noise(1, 0, 0, K, _ptr(nz), 5, None) == INVALID
    assert lib.marl_maven_noise(1, 0, 0, 4, None, 5, None) == INVALID and lib.marl_maven_noise(1, 0, 0, 4, _ptr(nz), 0, None) == 0
    torch.cuda.synchronize()
    assert bool((nz == int(SENT)).all())
    # ---- MI pass
    B, T, N, A, S, K = shape = (2, 7, 2, 3, 5, 3)
    m = mo.mi_case(*shape)
    names = [k for k, _ in mo.disc_shapes(N, A, S, K)]
    disc, dg = {k: up(m.disc[k]) for k in names}, {k: up(m.base[k]) for k in names}
    d, gd = ops.maven_disc(disc), ops.maven_disc_grads(dg)
    t = dict(q=up(np.nan_to_num(m.q)), avail=up(np.nan_to_num(m.avail_store)), state=up(np.nan_to_num(m.state_store)), ep_map=up(m.ep_map),
             noise=up(m.noise), padded=up(m.padded), dq=out_buf(B * T * N * A), ce=out_buf(B * T), stats=out_buf(2),
             ws=out_buf(lib.marl_maven_mi_workspace(B * T, N, A, K, S) // 4))

    def mi(**o):
        a = dict(d=C.byref(d), g=C.byref(gd), avail_bs=m.Ts * N * A, state_ld=m.ld, state_bs=m.Ts, lam=1.0, wsb=(t["ws"].numel() - TAIL) * 4,
                 B=B, T=T, N=N, A=A, S=S, K=K, **{k: _ptr(v) for k, v in t.items()})
        a.update(o)
        return lib.marl_maven_mi(a["d"], a["g"], a["q"], a["avail"], C.c_long(a["avail_bs"]), a["state"], C.c_long(a["state_ld"]),
                                 C.c_long(a["state_bs"]), a["ep_map"], a["noise"], a["padded"], C.c_float(a["lam"]), a["dq"], a["ce"],
                                 a["stats"], a["ws"], C.c_size_t(a["wsb"]), a["B"], a["T"], a["N"], a["A"], a["S"], a["K"], None)
    bad = [dict(N=0), dict(N=17), dict(A=0), dict(A=33), dict(K=0), dict(K=33), dict(S=0), dict(S=5000), dict(B=1 << 15, T=1 << 15, N=2),
           dict(lam=-0.5), dict(lam=float("nan")), dict(state_ld=S - 1), dict(wsb=64), dict(avail_bs=-1)]
    bad += [{k: None} for k in ("d", "g", "q", "avail", "state", "noise", "padded", "dq", "ce", "stats", "ws")]
    for o in bad:
        assert mi(**o) == INVALID, o
    for o in (dict(B=0), dict(T=0)):
        assert mi(**o) == 0, o
    base = {k: v.clone() for k, v in dg.items()}
    torch.cuda.synchronize()
    assert all(bool((t[k] == SENT).all()) for k in ("dq", "ce", "stats", "ws")) and all(torch.equal(base[k], dg[k]) for k in base)
    assert mi() == 0 and mi(ep_map=None, avail_bs=m.Ts * N * A) == 0
    torch.cuda.synchronize()
    assert not bool((t["dq"][:B * T * N * A] == SENT).any()) and tail_ok(t["dq"], B * T * N * A) and tail_ok(t["ws"], t["ws"].numel() - TAIL)
    assert not ops.maven_supported(5, 11, 16, 120, 32) and lib.marl_maven_plan(3, 5, 17, 11, 16, 120, None) == INVALID


# ------------------------------------------------------------------------------------------------ the learner
def build_product(args, state, gemm_mode=None):
    """MAVENMAC + MAVENLearner with the oracle state's parameters"""
    from marl_amd.controller.share_params import MAVENMAC
    from marl_amd.algorithm.maven import MAVENLearner
    from marl_amd.network.mixer import QMixMixer
    args.cuda = True
    if gemm_mode is not None:
        args.gemm_mode = gemm_mode
    mac = MAVENMAC(args)
    f = lambda d: {k: x.detach().float() for k, x in d.items()}
    mac.agent.load_state_dict(f(state.agent))
    learner = MAVENLearner(mac, args)
    assert type(learner.mixer) is QMixMixer and learner.graphs is None and learner.n_stats == 4 and learner.den_slot == 1
    for net in (learner.mixer, learner.target_mixer):
        net.load_state_dict(f(state.mixer))
    learner.maven_discrim.load_state_dict(f(state.discrim))
    learner.target_net.agent.load_state_dict(f(state.agent))
    return mac, learner


def named(learner):
    return [(p + "." + k, x) for p, net in (("agent", learner.eval_net.agent), ("mixer", learner.mixer), ("discrim", learner.maven_discrim))
            for k, x in net.named_parameters()]


def with_noise(batch, noise):
    b = learners.clone_batch(batch)
    b["noise"] = np.asarray(noise).copy()
    return b


def two_updates(case, gemm_mode):
    args, st, batch_of, noise_of, lam = mo.learner_case(case)
    _, learner = build_product(mo.learner_case(case)[0], st, gemm_mode)
    for i, tol in enumerate(mo.LEARNER_TOL):
        batch, noise = batch_of(i), noise_of(i)
        loss = learner.train(with_noise(batch, noise), i)
        oloss, ograds, o = mo.train(st, learners.clone_batch(batch), noise, i, lam=lam)
        c = "maven_train:%s[%s]/step%d" % (case, gemm_mode, i)
        assert learner.max_episode_len == o["T"]
        stats = learner.last_stats.cpu().numpy().astype(np.float64)
        print(c, "loss", loss, oloss, "stats", stats, "oracle", [float(o[k].detach()) for k in ("num", "den", "ce_sum", "hits")])
        parity.close(c, "loss", loss, oloss, tol=tol)
        den = stats[1]
        assert den == float(o["den"])
        dbg = learner._dbg
        B, T = o["live"].shape
        for k in ("q_evals", "q_targets", "hs", "q_tot", "q_tot_target"):
            ref = o[k].detach().numpy()
            parity.close(c, k, dbg[k].cpu().numpy().reshape(ref.shape), ref, tol=tol)
        if args.lambda_mi > 0:
            parity.close(c, "sum m ce", stats[2], float(o["ce_sum"]), tol=tol)
            assert stats[3] == float(o["hits"])
            parity.close(c, "ce", dbg["ce"].cpu().numpy().reshape(B, T), o["ce"].detach().numpy(), tol=tol)
            parity.close(c, "dq_dense", dbg["dq_dense"].cpu().numpy(), o["dq_dense"].numpy(), tol=tol)
        else:
            assert dbg["ce"] is None and dbg["dq_dense"] is None and stats[2] == 0 and stats[3] == 0
        got, ref = named(learner), dict(st.named_params())
        assert [k for k, _ in got] == list(ref)
        for n, p in got:
            if i == 0:
                gref = ograds[n].numpy() if ograds[n] is not None else np.zeros(p.shape)
                parity.close(c, "grad " + n, p.grad.detach().cpu().numpy() / den, gref, tol=tol)
            exc = mo.F32_EXCEPTIONS.get((case, i, "param " + n))
            if exc is None:
                parity.close(c, "param " + n, p.detach().cpu().numpy(), ref[n].detach().numpy(), tol=tol)
            else:
                err = float(np.abs(p.detach().cpu().numpy().astype(np.float64) - ref[n].detach().numpy()).max())
                print(c, "param", n, "err %.3e against the listed float32-oracle figure %.3e" % (err, exc))
                assert err <= 4.0 * exc, (c, n, err, exc)
    return learner, st


@pytest.mark.parametrize("case", list(mo.LEARNER_CASES))
def test_two_updates_vs_oracle(case, gemm_mode):
    two_updates(case, gemm_mode)


def test_zero_tables_and_no_mi_start_from_qmix_bit_for_bit(gemm_mode):
    """with the tables zero and lambda_mi = 0 the first update's q_evals, q_tot and loss are QLearner(qmix, no_loss_fold)'s"""
    from marl_amd.controller.share_params import SharedMAC
    from marl_amd.algorithm.q_learner import QLearner
    margs, st, batch_of, noise_of, _ = mo.learner_case("2s3z", zero_tables=True, lambda_mi=0.0)
    _, maven = build_product(mo.learner_case("2s3z", zero_tables=True, lambda_mi=0.0)[0], st, gemm_mode)
    qargs = seeded.make_args("2s3z", "qmix", episode_limit=margs.episode_limit, no_loss_fold=True, cuda=True, gemm_mode=gemm_mode)
    mac = SharedMAC(qargs)
    plain = {k: x.detach().float() for k, x in st.agent.items() if not k.startswith("maven.")}
    mac.agent.load_state_dict(plain)
    qmix = QLearner(mac, qargs)
    for net in (qmix.mixer, qmix.target_mixer):
        net.load_state_dict({k: x.detach().float() for k, x in st.mixer.items()})
    qmix.target_net.agent.load_state_dict(plain)
    batch = batch_of(0)
    la = maven.train(with_noise(batch, noise_of(0)), 0)
    lb = qmix.train(learners.clone_batch(batch), 0)
    assert la == lb, (la, lb)
    for k in ("q_evals", "q_tot"):
        assert bool((maven._dbg[k] == qmix._dbg[k]).all()), k


def test_learner_refuses_a_batch_without_noise_and_syncs_targets(tmp_path):
    args, st, batch_of, noise_of, _ = mo.learner_case("2s3z", target_update_cycle=1, save_cycle=1, model_dir=str(tmp_path))
    _, a = build_product(args, st)
    before = a._flat.flat.clone()
    with pytest.raises(ValueError, match="noise"):
        a.train(learners.clone_batch(batch_of(0)), 0)
    a.train(with_noise(batch_of(0), noise_of(0)), 0)
    tables = lambda net: torch.cat([p.detach().reshape(-1) for k, p in net.named_parameters() if k.startswith("maven.")])
    assert not torch.equal(before, a._flat.flat) and not torch.equal(tables(a.eval_net.agent), tables(a.target_net.agent))
    a.train(with_noise(batch_of(1), noise_of(1)), 1)                      # the target copy covers the tables
    assert torch.equal(tables(a.eval_net.agent), tables(a.target_net.agent))
    # model files and the resume state: to equal bits, the discriminator in a file of its own
    a.save_models(7)
    d = a.model_dir
    assert sorted(os.listdir(d)) == ["7_maven_discrim_net_params.pkl", "7_mixer_net_params.pkl", "7_rnn_net_params.pkl"]
    for f in os.listdir(d):
        shutil.copy(os.path.join(d, f), os.path.join(d, f[2:]))           # load_models reads the un-numbered names
    a.save_resume(str(tmp_path / "resume.pt"))
    torch.manual_seed(5)
    args2, st2, *_ = mo.learner_case("2s3z", target_update_cycle=1, save_cycle=1, model_dir=str(tmp_path))
    from marl_amd.controller.share_params import MAVENMAC
    from marl_amd.algorithm.maven import MAVENLearner
    args2.cuda = True
    b = MAVENLearner(MAVENMAC(args2), args2)
    assert not torch.equal(a._flat.flat, b._flat.flat)
    b.load_models()
    assert torch.equal(a._flat.flat, b._flat.flat)
    b.load_resume(str(tmp_path / "resume.pt"))
    for k, x in a.resume_state().items():
        y = b.resume_state()[k]
        assert torch.equal(x, y) if isinstance(x, torch.Tensor) else (k == "optimizer" or x == y), k
    la, lb = (l.train(with_noise(batch_of(2), noise_of(2)), 2) for l in (a, b))
    assert la == lb and torch.equal(a._flat.flat, b._flat.flat)
    # the controller's batch interface takes the batch's noise
    mac = a.eval_net
    mac.init_hidden(4)
    q, hs = mac.get_current_q_values(with_noise(batch_of(0), noise_of(0)), args.episode_limit)
    mac.init_hidden(4)
    q2, _ = mac.get_next_q_values(with_noise(batch_of(0), (noise_of(0) + 1) % 16), args.episode_limit)
    assert q.shape == q2.shape == (4, args.episode_limit, 5, 11) and hs.shape[-1] == 64
    with pytest.raises(ValueError, match="noise"):
        mac.get_current_q_values(batch_of(0), args.episode_limit)


def test_matrix_game_table_per_noise_index():
    """get_q_and_q_tot_table(noise=k): the agents' Q rows and the 3x3 q_tot table of one noise index, against float64"""
    from oracle import nets
    args, st, *_ = mo.learner_case("matrix_mi0")
    _, learner = build_product(mo.learner_case("matrix_mi0")[0], st)
    tables = []
    for k in range(3):
        table, qi, qj = learner.get_q_and_q_tot_table(k) if k else learner.get_q_and_q_tot_table()
        with torch.no_grad():
            q0, hs, _ = nets.agent_unroll(st.agent, torch.ones(1, 1, 2, 1, dtype=torch.float64), torch.zeros(1, 1, 2, 3, dtype=torch.float64),
                                          torch.zeros(2, 64, dtype=torch.float64))
            q = q0 + mo.head_term(st.agent, hs, [k], "maven.")
            ref = np.array([[float(nets.qmix(st.mixer, torch.stack((q[0, 0, 0, i], q[0, 0, 1, j])).view(1, 1, 2),
                                             torch.ones(1, 1, 1, dtype=torch.float64), args)) for j in range(3)] for i in range(3)])
        c = "maven_table:noise%d" % k
        parity.close(c, "q_i", qi, q[0, 0, 0].numpy())
        parity.close(c, "q_j", qj, q[0, 0, 1].numpy())
        parity.close(c, "q_tot", table, ref)
        tables.append(table)
    assert not np.array_equal(tables[0], tables[1]) and not np.array_equal(tables[1], tables[2])
    for bad in (-1, 3, True, 1.0):
        with pytest.raises(ValueError, match="noise"):
            learner.get_q_and_q_tot_table(bad)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("argv", [["--env", "synthetic", "--map", "2s3z", "--n_envs", "8"],
                                  ["--env", "battle", "--map", "3m", "--battle_fused", "True", "--n_envs", "8"]], ids=["synthetic", "battle"])
def test_launcher_trains_and_the_ring_carries_the_draw(argv, tmp_path):
    from marl_amd.main import build, make_runner
    from marl_amd.runner import Runner
    from marl_amd.algorithm.maven import MAVENLearner
    from marl_amd.controller.share_params import MAVENMAC
    from marl_amd.utils.logging import Logger
    common = ["--alg", "maven", "--n_steps", "1", "--evaluate_epoch", "0", "--result_dir", str(tmp_path / "res"), "--model_dir", str(tmp_path / "model")]
    args, env = build(argv + common)
    assert (args.noise_dim, args.lambda_mi, args.maven_discrim_dim) == (16, 0.001, 64)
    args.save_cycle = 10 ** 9
    torch.manual_seed(3)
    r = make_runner(args, env, Logger())
    assert type(r.learner) is MAVENLearner and type(r.mac) is MAVENMAC and r.buffer is not None
    before = r.learner._flat.flat.clone()
    E, T1 = 8, args.episode_limit + 1
    expect = []
    for it in range(3):
        r.args.n_steps = r.time_steps + 1
        r.run(0)
        expect.append(mo.noise_draw(args.seed, env.env0, env.episode * T1, 16, E))
        assert np.array_equal(r.mac.noise.cpu().numpy(), expect[-1])
        s = r.learner.last_stats.cpu().numpy()
        assert np.isfinite(s).all() and 0 <= s[3] <= s[1] and s[1] > 0 and s[2] > 0, s
    assert r.train_steps == 3 == len(r.losses) and all(np.isfinite(float(x)) for x in r.losses) and not torch.equal(before, r.learner._flat.flat)
    ring = r.buffer.record
    assert ring.noise.shape == (ring.E,) and np.array_equal(ring.noise[:3 * E].cpu().numpy(), np.concatenate(expect))
    assert len({tuple(x.tolist()) for x in expect}) == 3                   # a fresh draw every rollout
    # an evaluation rollout draws the same way
    r.args.evaluate_epoch = 1
    r.evaluate()
    assert np.array_equal(r.mac.noise.cpu().numpy(), mo.noise_draw(args.seed, env.env0, env.episode * T1, 16, E))
    # the runner's resume file carries the ring's noise
    path = str(tmp_path / "resume.pt")
    r.save_resume(path)
    flat, noise = r.learner._flat.flat.clone(), ring.noise.clone()
    ring.noise.zero_()
    r.learner._flat.flat.add_(1.0)
    r.load_resume(path)
    assert torch.equal(ring.noise, noise) and torch.equal(r.learner._flat.flat, flat)
    # the whole-rollout and overlap refusals
    with pytest.raises(RuntimeError, match="no MAVEN head"):
        r.rolloutWorker.launch_episodes()
    args.overlap_rollout = True
    with pytest.raises(NotImplementedError, match="MAVEN head"):
        Runner(env, Logger(), args)
