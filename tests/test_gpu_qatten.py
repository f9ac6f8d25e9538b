"""The Qatten row kernel (csrc/qatten.hip) on the MI355X against tests/qatten_oracle.py: marl_qatten_mix_fwd, _mix_bwd and _loss_bwd
at every case of qatten_oracle.CASES, at the tile edges marl_qatten_plan reports, through the grid-stride loop, with bases off the
16-byte grid and through a remapped source with an episode map.  Needs a real MI355X: ``pytest -m gpu``.

Bounds: qatten_oracle.bounds (K u (1 + L) mag, constants from the float32 twin); den exact; num within rowwise_oracle.K_TD_NUM u
mag_num plus the propagated q_tot bound 2 sum |m td| bound(q_tot).  The loss-folded entry gives mix_fwd's q_tot and the dq, dp, dw_raw,
dq_tot of mix_fwd -> td_loss -> mix_bwd bit for bit; two calls of an entry give the same bits; padded rows are exact zeros; NaN in the
unread state columns and a saturated softmax leave everything finite; nothing is written past an output."""
import numpy as np
import pytest
import torch

import qatten_oracle as qo
import rowwise_oracle as ro

pytestmark = pytest.mark.gpu

SENT, TAIL = 12345.0, 64
DEV = "cuda"


def _plan(N, U, H, rows=1):
    from marl_amd import ops
    return ops.qatten_plan(rows, N, U, H)


def _sent(n):
    return torch.full((n + TAIL,), SENT, device=DEV)


def _up(x, off=0):
    """x on the device, its base `off` floats past a 256-byte boundary"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    buf = torch.zeros(x.size + off, device=DEV)
    buf[off:] = torch.from_numpy(x).reshape(-1)
    return buf[off:].view(*x.shape)


class Dev:
    """a case's operands on the device; hy rows [p | w_raw | c] at a row stride of `ldh`"""

    def __init__(self, c, off=0, ldh=None):
        HW = c.H * c.U + c.H + 1
        self.c, self.HW = c, HW
        self.ldh = ldh or (HW + 3) // 4 * 4
        hy = np.zeros((c.R, self.ldh), np.float32)
        hy[:, :HW] = np.concatenate([c.p, c.w_raw, c.c[:, None]], 1)
        self.s, self.hy = _up(c.s, off), _up(hy, off)[:, :HW]
        self.q, self.g = _up(c.q), _up(c.g)
        self.q_tgt, self.r, self.term, self.padded = (_up(x) for x in c.loss[:4])
        self.ldd = c.H * c.U + c.H + 3                  # three columns the kernel may not touch

    def src(self):
        from marl_amd import ops
        return ops.src(self.s)

    def outs(self):
        c = self.c
        o = dict(q_tot=_sent(c.R), dq=_sent(c.R * c.N), dhy=_sent(c.R * self.ldd), dq_tot=_sent(c.R), out2=_sent(2))
        return o

    def views(self, o):
        c = self.c
        return dict(q_tot=o["q_tot"][:c.R], dq=o["dq"][:c.R * c.N].view(c.R, c.N), dhy=o["dhy"][:c.R * self.ldd].view(c.R, self.ldd),
                    dq_tot=o["dq_tot"][:c.R], out2=o["out2"][:2])

    def run(self, mode, src=None, dq_tot=None):
        """mode fwd / bwd / loss -> (raw sentinel buffers, views)"""
        from marl_amd import ops
        c = self.c
        o = self.outs()
        v = self.views(o)
        x = src if src is not None else self.src()
        a = (c.R, c.N, c.U, c.H)
        if mode == "fwd":
            ops.qatten_mix_fwd(x, self.hy, self.q, c.scale, v["q_tot"], *a)
        elif mode == "bwd":
            ops.qatten_mix_bwd(x, self.hy, self.q, c.scale, self.g if dq_tot is None else dq_tot, v["dq"], v["dhy"], *a)
        else:
            ops.qatten_loss_bwd(x, self.hy, self.q, c.scale, self.q_tgt, self.r, self.term, self.padded, qo.GAMMA, v["q_tot"], v["dq"],
                                v["dhy"], v["dq_tot"], v["out2"], *a)
        torch.cuda.synchronize()
        return o, v

    def untouched(self, o, written):
        """sentinel tails intact, unwritten outputs untouched, and dhy's columns from H U + H on"""
        c = self.c
        sizes = dict(q_tot=c.R, dq=c.R * c.N, dhy=c.R * self.ldd, dq_tot=c.R, out2=2)
        for k, buf in o.items():
            n = sizes[k] if k in written else 0
            assert (buf[n:] == SENT).all(), k
        if "dhy" in written:
            assert (self.views(o)["dhy"][:, c.H * c.U + c.H:] == SENT).all()


def _frac(name, got, ref, bound, worst):
    err = np.abs(got.astype(np.float64) - ref)
    live = bound > 0
    assert (err[~live] == 0).all(), name
    f = float((err[live] / bound[live]).max()) if live.any() else 0.0
    worst[name] = max(worst.get(name, 0.0), f)
    assert f <= 1.0, (name, f)


def _check_grads(c, v, o, worst, tag):
    HU = c.H * c.U
    b = qo.bounds(o)
    dhy = v["dhy"].cpu().numpy()
    _frac(tag + "dq", v["dq"].cpu().numpy(), o.dq, b.dq, worst)
    _frac(tag + "dw_raw", dhy[:, HU:HU + c.H], o.dw_raw, b.dw_raw, worst)
    _frac(tag + "dp", dhy[:, :HU], o.dp, b.dp, worst)
    _frac(tag + "dp_wide", dhy[:, :HU], o.dp, b.dp_wide, worst)


def check_case(c, off=0, ldh=None, src_of=None):
    """all three entries of one case against the oracle and against each other; returns the worst fractions of the bounds"""
    from marl_amd import ops
    d = Dev(c, off, ldh)
    src = src_of(d) if src_of else None
    worst = {}
    o_f, o_l = qo.oracle_of(c), qo.oracle_of(c, loss=True)
    # forward
    raw_f, f = d.run("fwd", src)
    d.untouched(raw_f, {"q_tot"})
    _frac("q_tot", f["q_tot"].cpu().numpy(), o_f.q_tot, qo.bounds(o_f).q_tot, worst)
    assert torch.isfinite(f["q_tot"]).all()
    # backward from a given gradient
    raw_b, b = d.run("bwd", src)
    d.untouched(raw_b, {"dq", "dhy"})
    _check_grads(c, b, o_f, worst, "")
    # loss-folded
    raw_l, l = d.run("loss", src)
    d.untouched(raw_l, {"q_tot", "dq", "dhy", "dq_tot", "out2"})
    assert torch.equal(l["q_tot"], f["q_tot"])                                        # bit for bit
    num, den = (float(x) for x in l["out2"].cpu())
    assert den == o_l.den
    bq = qo.bounds(o_l).q_tot
    assert abs(num - o_l.num) <= ro.K_TD_NUM * qo.U32 * o_l.mag_num + 2.0 * float(np.sum(np.abs(o_l.mtd) * bq)), (num, o_l.num)
    # the composition the fold replaces: mix_fwd -> td_loss -> mix_bwd, bit for bit
    dq_tot, out2 = _sent(c.R)[:c.R], _sent(2)[:2]
    ops.td_loss(f["q_tot"], d.q_tgt, d.r, d.term, d.padded, qo.GAMMA, dq_tot, out2, c.R)
    _, comp = d.run("bwd", src, dq_tot=dq_tot)
    HU = c.H * c.U
    assert torch.equal(l["dq_tot"], dq_tot) and torch.equal(l["dq"], comp["dq"])
    assert torch.equal(l["dhy"][:, :HU + c.H], comp["dhy"][:, :HU + c.H])
    assert float(out2[1]) == den
    # the folded launch against the oracle: its g = -2 m (m td) within what q_tot's bound and the four roundings of td leave, and
    # its gradients within the bounds of the oracle run on that g; the padded rows and finiteness
    g_l = l["dq_tot"].cpu().numpy().astype(np.float64)
    m = 1.0 - c.padded.astype(np.float64)
    assert (np.abs(g_l - o_l.dq_tot) <= 2.0 * m * (bq + 4 * qo.U32 * o_l.mag_td)).all()
    _check_grads(c, l, qo.rows(c.s, c.p, c.w_raw, c.c, c.q, c.scale, c.N, c.U, c.H, g=g_l), worst, "loss ")
    dead = torch.from_numpy(c.padded == 1).to(DEV)
    for k in ("dq", "dq_tot"):
        assert (l[k][dead] == 0).all(), k
    assert (l["dhy"][dead][:, :HU + c.H] == 0).all()
    for k, cols in (("dq", c.N), ("dhy", HU + c.H), ("dq_tot", None)):
        x = l[k] if cols is None else l[k][:, :cols]
        assert torch.isfinite(x).all(), k
    # two calls, the same bits
    for mode, first in (("fwd", f), ("bwd", b), ("loss", l)):
        _, again = d.run(mode, src)
        for k in first:
            assert torch.equal(first[k], again[k]), (mode, k)
    return worst


def _print(name, worst):
    print("qatten %s: worst fraction of the bound " % (name,) + "  ".join("%s %.3f" % kv for kv in sorted(worst.items())))


@pytest.mark.parametrize("shape", qo.CASES, ids=str)
def test_cases_against_the_oracle(shape):
    c = qo.kernel_case(*shape, seed=shape[0])
    worst = check_case(c)
    _print(shape, worst)


def test_one_of_everything_is_exact():
    c = qo.kernel_case(1, 1, 1, 1, 1)
    d = Dev(c)
    _, b = d.run("bwd")
    assert float(b["dhy"][0, 0]) == 0.0                    # softmax over one agent: lam = 1, dp = 0 exactly
    assert float(b["dq"][0, 0]) == float(np.float32(c.g[0]) * np.abs(c.w_raw[0, 0]))


def test_planted_rows():
    c = qo.kernel_case(65, 5, 24, 4, 120)
    d = Dev(c)
    _, l = d.run("loss")
    P, HU = qo.PLANTED, c.H * c.U
    assert float(l["dhy"][P["w_zero"], HU]) == 0.0         # w_raw = 0: sign(0) = 0, dw_raw exactly 0
    o = qo.oracle_of(c, loss=True)
    sat = l["dhy"][P["saturated"]]
    assert torch.isfinite(sat[:HU + c.H]).all() and abs(o.lam[P["saturated"], 0].max() - 1.0) < 1e-12
    c2 = qo.kernel_case(129, 10, 32, 4, 322)
    assert np.isnan(c2.s[:, 320:]).all()                   # ... and check_case saw every output of that case finite


@pytest.mark.parametrize("name", ["MMM2", "2s3z"])
def test_tile_edges(name):
    N, U, H, S = qo.MAPS[name]
    TR = _plan(N, U, H)[0]
    assert 1 <= TR <= 64 and TR * H <= 256
    worst = {}
    for R in (TR - 1, TR, TR + 1):                          # one row below, at and above a tile; the last is a second workgroup's
        assert _plan(N, U, H, R)[1] == (2 if R > TR else 1)
        for k, v in check_case(qo.kernel_case(R, N, U, H, S, seed=R)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    _print(name + " tile edges (tile %d rows)" % TR, worst)


def test_grid_stride_loop():
    N, U, H, S = 2, 1, 1, 2
    TR = _plan(N, U, H)[0]
    R = 1024 * TR + 1                                       # one row beyond what the capped grid covers in one pass
    tr, grid, lds, rounds = _plan(N, U, H, R)
    assert grid == 1024 and rounds == 2
    _print("grid stride (%d rows)" % R, check_case(qo.kernel_case(R, N, U, H, S, seed=5)))


def test_bases_off_the_16_byte_grid():
    """state base and hy base one float past a 16-byte boundary, odd row strides: the scalar head and tail of every row copy"""
    for shape in ((65, 5, 24, 4, 120), (38, 10, 32, 4, 322)):
        c = qo.kernel_case(*shape, seed=17)
        HW = c.H * c.U + c.H + 1
        d = Dev(c, off=1, ldh=HW)
        assert d.s.data_ptr() % 16 == 4 and d.hy.data_ptr() % 16 == 4
        w = check_case(c, off=1, ldh=HW)
        aligned = Dev(c)
        for mode in ("fwd", "bwd", "loss"):                # the same bits as from aligned operands
            _, a = aligned.run(mode)
            _, b = d.run(mode)
            for k in a:
                assert torch.equal(a[k], b[k]), (mode, k)
        _print(str(shape) + " off the grid", w)


# B sampled episodes of a ring of E, T steps of (T + 1)-slot storage: modelled on REMAP_CASES of tests/qmix_loss_oracle.py
@pytest.mark.parametrize("off", [0, 1])
def test_remapped_source_with_an_episode_map(off):
    from marl_amd import ops
    N, U, H, S = qo.MAPS["MMM2"]
    E, B, T = 7, 5, 9
    g = np.random.default_rng(3)
    ring = g.standard_normal((E, T + 1, S)).astype(np.float32)
    emap = np.array([6, 0, 3, 3, 5], dtype=np.int32)
    c = qo.kernel_case(B * T, N, U, H, S, seed=21)
    c.s = ring[emap][:, off:off + T].reshape(B * T, S).copy()
    c.s[:, N * U:] = np.nan
    ring[:, :, N * U:] = np.nan
    ring_d, emap_d = _up(ring.reshape(-1, S)), torch.from_numpy(emap).to(DEV)
    src_of = lambda d: ops.src(ops.Rows(ring_d, (T, T + 1, off), emap_d))
    assert ops.qatten_supported(ops.Rows(ring_d, (T, T + 1, off), emap_d), N, U, H)
    w = check_case(c, src_of=src_of)
    dense, d = Dev(c), Dev(c)
    for mode in ("fwd", "loss"):
        _, a = dense.run(mode)
        _, b = d.run(mode, src_of(d))
        for k in a:
            assert torch.equal(a[k], b[k]), (mode, k)
    _print("remapped, off %d" % off, w)


def test_unsupported_shapes_and_sources_are_refused_and_write_nothing():
    from marl_amd import ops
    from marl_amd._lib import MarlHipError
    c = qo.kernel_case(8, 5, 24, 4, 120)
    d = Dev(c)
    assert ops.qatten_supported(d.src(), 5, 24, 4)
    bad_shapes = [(17, 4, 4), (4, 65, 4), (4, 4, 9), (0, 4, 4), (4, 0, 4), (4, 4, 0)]
    wide = _up(np.zeros((8, 17 * 65), np.float32))
    for N, U, H in bad_shapes:
        assert not ops.qatten_supported(ops.src(wide), N, U, H)
        assert _lib_plan_refuses(N, U, H)
    other = _up(np.zeros((8, 4), np.float32))
    bad_src = [ops.src(d.s, other), ops.src(d.s, nid=2), ops.src(d.s, gate=d.s),
               ops.src(d.s, idx=torch.zeros(8, 1, dtype=torch.int32, device=DEV), nhot=1, hot_w=3), ops.src(d.s[:, :100])]
    for x in bad_src:
        assert not ops.qatten_supported(x, 5, 24, 4)
        for mode in ("fwd", "bwd", "loss"):
            with pytest.raises(MarlHipError, match="hipError_t 1$"):
                d.run(mode, x)
    # the entries themselves, with operands wide enough for any of these shapes: refused before anything is launched
    R, W = 8, 17 * 65
    z = lambda *shape: torch.zeros(*shape, device=DEV)
    s, hy, q, vec = ops.src(z(R, W)), z(R, W + 80), z(R, 17), z(R)
    for N, U, H in bad_shapes:
        for mode in ("fwd", "bwd", "loss"):
            o = dict(q_tot=_sent(R), dq=_sent(R * 17), dhy=_sent(R * (W + 80)), dq_tot=_sent(R), out2=_sent(2))
            dhy = o["dhy"][:R * (W + 80)].view(R, W + 80)
            with pytest.raises(MarlHipError, match="hipError_t 1$"):
                if mode == "fwd":
                    ops.qatten_mix_fwd(s, hy, q, 1.0, o["q_tot"], R, N, U, H)
                elif mode == "bwd":
                    ops.qatten_mix_bwd(s, hy, q, 1.0, vec, o["dq"], dhy, R, N, U, H)
                else:
                    ops.qatten_loss_bwd(s, hy, q, 1.0, vec, vec, vec, vec, qo.GAMMA, o["q_tot"], o["dq"], dhy, o["dq_tot"], o["out2"],
                                        R, N, U, H)
            torch.cuda.synchronize()
            for buf in o.values():
                assert (buf == SENT).all()


def _lib_plan_refuses(N, U, H):
    from marl_amd import ops
    from marl_amd._lib import MarlHipError
    try:
        ops.qatten_plan(1, N, U, H)
    except MarlHipError:
        return True
    return False
