"""The float64 statement of the FORWARD agent unroll, for the kernel tests of its two entry points (csrc/agent.hip:
agent_fwd_pipe_kernel / agent_fwd_kernel; csrc/agent_x6.hip, csrc/agent_x6p.hip) - tests/test_gpu_unroll.py - and its own CPU tests
(tests/test_unroll_oracle_cpu.py).  TEST INFRASTRUCTURE: the product never imports it.

* `SHAPES`: the (N, O, A) the cases run - the scenario shapes (2s3z, MMM2, and 3s5z for the five-chunk split instantiation, which
  neither of the two reaches) and widths picked for what they reach.
* `make_inputs`: seeded parameters (scale 2.0, as tests/bptt_oracle.py draws them), (T+1)-slot observation storage that holds more
  episodes than the batch, a permuting ep_map, ragged ep_len (1 and T among them), fed actions with -1 entries, a non-zero h0; every
  value is an fp32 number, so the device gets bit for bit what float64 sees.
* `resolve`: the storage addressing of include/marl_hip.h stated in numpy - batch episode b reads storage episode ep_map[b], slot
  t + obs_t0; steps t >= ep_len[b] read zeros; the action fed at step t is ufed[b, t + u_t0], none when that index or the value is
  negative or when no ufed is given.
* `forward`: bptt_oracle.unroll on the resolved inputs (ONE definition of the GRU step: bptt_oracle.gates), in any dtype -> q, hs,
  h_last, the six vectors per row-step the kernels save for BPTT (hprev | x = relu(fc1) | r | z | n | W_hn h + b_hn; plane 0 has one
  more slab: the hidden state after the last step) and the three input-side gate sums (b_ir + b_hr + x W_ir | b_iz + b_hz + x W_iz |
  b_in + x W_in).  The kernels' buffers are decoded with ops.saved_plane.
* The fp32 kernels store PRE-SCALED gate sums when A > 16 (gru_prescale of csrc/common.h: the r and z blocks times -log2(e), the n
  block times 2 log2(e)).  `gate_sum_scale` READS the two factors from csrc/common.h; the test divides the stored sums by them and
  holds the result to float64 like every other tensor.  (The bitwise continuation check covers them a second time.)
* `CASES`: (shape, B, T, cu_budget, launch kind, entry, expected plan) - the smallest row counts that reach each launch plan, found
  with marl_agent_unroll_fwd_plan; `FAMILIES` names the plans the table must reach."""
from __future__ import annotations

import os
import re
import types

import numpy as np
import torch

import bptt_oracle as bo
from oracle import seeded

H = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE, MULTI, X6, R6 = 0, 1, 2, 3                   # plan[0]
ELEMENT, VECTOR, HALF, W2L = 0, 1, 2, 3            # plan[6]

# name -> (seeded.SHAPES entry the other fields come from, N, O, A).  Input width = O + A + N with both flags on.
SHAPES = {
    "2s3z": ("2s3z", 5, 80, 11),        # 96: the anchor, last width on three chunks
    "3s5z": ("3s5z", 8, 128, 14),       # 150: the scenario shape on five chunks
    "MMM2": ("MMM2", 10, 176, 18),      # 204: seven chunks, two action tiles
    "i13": ("2s3z", 3, 8, 2),           # one fc1 chunk, smallest O the split kernel takes
    "i60": ("2s3z", 1, 48, 11),         # two chunks, N = 1
    "i41n20": ("2s3z", 20, 16, 5),      # N > 16: an episode's agents span row tiles, the id block is wider than a tile
    "i97": ("2s3z", 6, 80, 11),         # first width on five chunks (91 without the agent id: back on three)
    "i160": ("2s3z", 8, 136, 16),       # five chunks full, A = 16, last width with one action tile
    "i165a16": ("2s3z", 5, 144, 16),    # seven chunks, two action tiles, the second one empty (160 without the agent id)
    "i161a32": ("2s3z", 1, 128, 32),    # A = 32 at the first width that allows it
    "o192": ("2s3z", 4, 192, 12),       # O at the split kernel's prefetch limit
    "i224": ("2s3z", 16, 176, 32),      # every limit at once
    # the fp32 entry only
    "o30": ("2s3z", 3, 30, 9),          # element-wise: O % 4 != 0
    "o55": ("2s3z", 5, 55, 12),
    "o156a30": ("2s3z", 6, 156, 30),    # two action tiles, wide observations, O % 8 != 0: no half-tile kernel
    "a17": ("2s3z", 5, 80, 17),         # two action tiles on a narrow input
    "i304": ("2s3z", 16, 256, 32),      # wider than 224, LDS-capped tiles per workgroup
}
SCENARIOS = ("2s3z", "3s5z", "MMM2")
F32_ONLY = ("o30", "o55", "o156a30", "a17", "i304")
KINDS = ("plain", "nohs", "save", "cont")


def shape_args(shape, T, la=1, rn=1):
    base, N, O, A = SHAPES[shape]
    return seeded.make_args(base, "qmix", episode_limit=T, n_agents=N, obs_shape=O, n_actions=A, last_action=bool(la), reuse_network=bool(rn))


def width(shape, la=1, rn=1):
    _, N, O, A = SHAPES[shape]
    return O + (A if la else 0) + (N if rn else 0)


# --------------------------------------------------------------------------------------------------------- cases
def _c(shape, B, T, cus, kind, entry, plan, la=1, rn=1, obs_off=0, h_off=0, alias=0, seed=3):
    """kind: "plain" (q, hs, h_last), "nohs" (q, h_last: what the round-6 kernel takes), "save" (+ saved and gi_out), "cont" (slots
    1..T reading the gate sums a saving pass over slots 0..T-1 stored).  entry: "f32" / "x6".  obs_off: obs starts one float past a
    16-byte boundary; h_off: h0 and h_last one float past one; alias: the case also runs with h_last aliasing h0."""
    assert kind in KINDS and entry in ("f32", "x6")
    _, N, O, A = SHAPES[shape]
    return types.SimpleNamespace(shape=shape, B=B, T=T, cus=cus, kind=kind, entry=entry, plan=tuple(plan), la=la, rn=rn, obs_off=obs_off,
                                 h_off=h_off, alias=alias, seed=seed, N=N, O=O, A=A, R=B * N, key=(shape, B, T, la, rn, seed))


def case_id(c):
    s = "%s-B%d-T%d-cu%d-%s-%s" % (c.shape, c.B, c.T, c.cus, c.kind, c.entry)
    for n, f in (("nolast", not c.la), ("noid", not c.rn), ("obsoff", c.obs_off), ("hoff", c.h_off), ("alias", c.alias)):
        if f:
            s += "-" + n
    return s


def plan_id(plan):
    fam = ("pipe", "multi", "x6", "r6")[plan[0]]
    return "%s[RT%d wg%d full%d AC%d K%d %s%s]" % (fam, plan[1], plan[2], plan[3], plan[4], plan[5],
                                                   ("elem", "vec", "half", "w2l")[plan[6]], " reads-gi" if plan[7] else "")


def query(c, kind=None, hs=None):
    """what the library says the case's launch runs (None: it refuses).  kind / hs: another launch on the same inputs"""
    from marl_amd import ops
    kind = kind or c.kind
    hs = (kind != "nohs") if hs is None else hs
    return ops.agent_unroll_fwd_plan(c.entry == "x6", c.B, c.T, c.N, c.O, c.A, last_action=bool(c.la), reuse_network=bool(c.rn),
                                     cu_budget=c.cus, saved=kind == "save", gi_out=kind == "save", gi_in=kind == "cont", hs=hs,
                                     obs_aligned=not c.obs_off, h_aligned=not c.h_off)


def tiles_of(c):
    return (c.R + 15) // 16


def rt_max(c):
    """the most row tiles per workgroup the fp32 entry gives this launch, whatever the row count (LDS and the prefetch registers)"""
    big = types.SimpleNamespace(**dict(vars(c), B=1 << 16, cus=1))
    return query(big)[1]


def _f32(c, p):
    return c.entry == "f32"


# name -> predicate(case, plan): the launch plans the table must reach, each at a scenario shape and at two of the new shapes
# (FAMILIES_ONCE: one case is enough)
FAMILIES = {}
for _ac in (1, 2):
    FAMILIES["f32-pipe-save-ac%d" % _ac] = lambda c, p, a=_ac: p[0] == PIPE and c.kind == "save" and p[4] == a
    FAMILIES["f32-pipe-plain-ac%d" % _ac] = lambda c, p, a=_ac: p[0] == PIPE and c.kind in ("plain", "nohs") and p[4] == a
    FAMILIES["f32-pipe-read-ac%d" % _ac] = lambda c, p, a=_ac: p[0] == PIPE and p[7] == 1 and p[4] == a
FAMILIES.update({
    "f32-multi-rt1": lambda c, p: p[0] == MULTI and p[1] == 1 and p[2] > 1,
    "f32-multi-rt2-short-last": lambda c, p: p[0] == MULTI and p[1] == 2 and p[3] < p[2],
    "f32-multi-rt3-short-last": lambda c, p: p[0] == MULTI and p[1] == 3 and p[3] < p[2],
    # (capped: the CU budget alone would ask for more tiles per workgroup than LDS / the prefetch registers give)
    "f32-multi-rtmax-short-last": lambda c, p: (p[0] == MULTI and p[1] >= 2 and p[3] < p[2] and p[1] == rt_max(c)
                                                 and -(-tiles_of(c) // (c.cus or 256)) > p[1]),
    "f32-half": lambda c, p: p[0] == MULTI and p[6] == HALF,
    "f32-w2l": lambda c, p: p[0] == MULTI and p[6] == W2L,
    "f32-multi-read": lambda c, p: p[0] == MULTI and p[7] == 1,
    "f32-element-T1": lambda c, p: _f32(c, p) and p[6] == ELEMENT and c.T == 1,
    "f32-element-T2": lambda c, p: _f32(c, p) and p[6] == ELEMENT and c.T == 2,
    "f32-element-T5": lambda c, p: _f32(c, p) and p[6] == ELEMENT and c.T == 5,
    "f32-element-save": lambda c, p: _f32(c, p) and p[6] == ELEMENT and c.kind == "save",
    "f32-element-several-tiles": lambda c, p: _f32(c, p) and p[6] == ELEMENT and p[1] > 1 and c.T > 1,
    "f32-T1-alias": lambda c, p: _f32(c, p) and c.T == 1 and c.alias,
    "f32-T2": lambda c, p: _f32(c, p) and c.T == 2 and p[6] != ELEMENT,
    "f32-T3": lambda c, p: _f32(c, p) and c.T == 3,
    "x6-two-tile-all": lambda c, p: p[0] == X6 and p[1] == 2 and p[3] == p[2] and tiles_of(c) % 2 == 0,
    "x6-two-tile-last-without-second": lambda c, p: p[0] == X6 and p[1] == 2 and p[3] == p[2] and tiles_of(c) % 2 == 1,
    "x6-mixed-one": lambda c, p: p[0] == X6 and p[1] == 2 and p[2] - p[3] == 1 and p[3] > 0,
    "x6-mixed-several": lambda c, p: p[0] == X6 and p[1] == 2 and p[2] - p[3] > 1 and p[3] > 0,
    "x6-rounds": lambda c, p: p[0] == X6 and p[2] > 2 * (c.cus or 256),
    "x6-r6-rt3": lambda c, p: p[0] == R6 and p[1] == 3,
    "x6-T4": lambda c, p: p[0] == X6 and c.T == 4,
    "x6-T5": lambda c, p: p[0] == X6 and c.T == 5,
    "x6-h0-misaligned": lambda c, p: p[0] == X6 and c.h_off,
})
for _k in (3, 5, 7):
    FAMILIES["x6-one-tile-K%d-save" % _k] = lambda c, p, k=_k: p[0] == X6 and p[1] == 1 and p[5] == k and c.kind == "save"
    FAMILIES["x6-one-tile-K%d-read" % _k] = lambda c, p, k=_k: p[0] == X6 and p[1] == 1 and p[5] == k and p[7] == 1
    FAMILIES["x6-one-tile-K%d-plain" % _k] = lambda c, p, k=_k: p[0] == X6 and p[1] == 1 and p[5] == k and c.kind in ("plain", "nohs")
FAMILIES_ONCE = {
    "f32-T40": lambda c, p: _f32(c, p) and c.T == 40,
    "x6-seven-chunks-second-action-tile-empty": lambda c, p: p[0] == X6 and p[5] == 7 and p[4] == 2 and c.A <= 16,
    "x6-r6-N-above-16": lambda c, p: p[0] == R6 and c.N > 16,
    "rows-one-past-a-tile": lambda c, p: c.R % 16 == 1,
    "rows-whole-tiles": lambda c, p: c.R % 16 == 0,
}

# the expected plan is what the query returned when the row count was picked; tests/test_unroll_oracle_cpu.py holds the table to the library
CASES = [
    _c("2s3z", 4, 4, 2, "save", "f32", (0, 1, 2, 2, 1, 6, 1, 0)),   # pipe[RT1 wg2 full2 AC1 K6 vec]
    _c("i60", 17, 4, 2, "save", "f32", (0, 1, 2, 2, 1, 4, 1, 0)),   # pipe[RT1 wg2 full2 AC1 K4 vec]
    _c("i13", 6, 4, 2, "save", "f32", (0, 1, 2, 2, 1, 1, 1, 0)),   # pipe[RT1 wg2 full2 AC1 K1 vec]
    _c("2s3z", 4, 4, 2, "plain", "f32", (0, 1, 2, 2, 1, 6, 1, 0)),   # pipe[RT1 wg2 full2 AC1 K6 vec]
    _c("i97", 3, 4, 2, "plain", "f32", (0, 1, 2, 2, 1, 7, 1, 0)),   # pipe[RT1 wg2 full2 AC1 K7 vec]
    _c("i41n20", 1, 4, 2, "plain", "f32", (0, 1, 2, 2, 1, 3, 1, 0)),   # pipe[RT1 wg2 full2 AC1 K3 vec]
    _c("2s3z", 4, 4, 2, "cont", "f32", (0, 1, 2, 2, 1, 6, 1, 1)),   # pipe[RT1 wg2 full2 AC1 K6 vec reads-gi]
    _c("i165a16", 4, 4, 2, "cont", "f32", (0, 1, 2, 2, 1, 11, 1, 1)),   # pipe[RT1 wg2 full2 AC1 K11 vec reads-gi]
    _c("o192", 5, 4, 2, "cont", "f32", (0, 1, 2, 2, 1, 13, 1, 1)),   # pipe[RT1 wg2 full2 AC1 K13 vec reads-gi]
    _c("MMM2", 2, 4, 2, "save", "f32", (0, 1, 2, 2, 2, 13, 1, 0)),   # pipe[RT1 wg2 full2 AC2 K13 vec]
    _c("i161a32", 17, 4, 2, "save", "f32", (0, 1, 2, 2, 2, 11, 1, 0)),   # pipe[RT1 wg2 full2 AC2 K11 vec]
    _c("o156a30", 3, 4, 2, "save", "f32", (0, 1, 2, 2, 2, 12, 1, 0)),   # pipe[RT1 wg2 full2 AC2 K12 vec]
    _c("MMM2", 2, 4, 2, "plain", "f32", (0, 1, 2, 2, 2, 13, 1, 0)),   # pipe[RT1 wg2 full2 AC2 K13 vec]
    _c("a17", 4, 4, 2, "plain", "f32", (0, 1, 2, 2, 2, 7, 1, 0)),   # pipe[RT1 wg2 full2 AC2 K7 vec]
    _c("i224", 2, 4, 2, "plain", "f32", (0, 1, 2, 2, 2, 14, 1, 0)),   # pipe[RT1 wg2 full2 AC2 K14 vec]
    _c("MMM2", 2, 4, 2, "cont", "f32", (0, 1, 2, 2, 2, 13, 1, 1)),   # pipe[RT1 wg2 full2 AC2 K13 vec reads-gi]
    _c("i304", 2, 4, 2, "cont", "f32", (0, 1, 2, 2, 2, 19, 1, 1)),   # pipe[RT1 wg2 full2 AC2 K19 vec reads-gi]
    _c("i161a32", 17, 4, 2, "cont", "f32", (0, 1, 2, 2, 2, 11, 1, 1)),   # pipe[RT1 wg2 full2 AC2 K11 vec reads-gi]
    _c("2s3z", 4, 1, 2, "plain", "f32", (1, 1, 2, 2, 1, 6, 1, 0)),   # multi[RT1 wg2 full2 AC1 K6 vec]
    _c("o30", 6, 1, 2, "plain", "f32", (1, 1, 2, 2, 1, 3, 0, 0)),   # multi[RT1 wg2 full2 AC1 K3 elem]
    _c("o55", 4, 1, 2, "plain", "f32", (1, 1, 2, 2, 1, 5, 0, 0)),   # multi[RT1 wg2 full2 AC1 K5 elem]
    _c("2s3z", 7, 2, 2, "plain", "f32", (1, 2, 2, 1, 1, 6, 1, 0)),   # multi[RT2 wg2 full1 AC1 K6 vec]
    _c("i160", 5, 2, 2, "plain", "f32", (1, 2, 2, 1, 1, 10, 1, 0)),   # multi[RT2 wg2 full1 AC1 K10 vec]
    _c("i13", 11, 2, 2, "plain", "f32", (1, 2, 2, 1, 1, 1, 1, 0)),   # multi[RT2 wg2 full1 AC1 K1 vec]
    _c("2s3z", 13, 2, 2, "plain", "f32", (1, 3, 2, 1, 1, 6, 1, 0)),   # multi[RT3 wg2 full1 AC1 K6 vec]
    _c("i60", 65, 2, 2, "plain", "f32", (1, 3, 2, 1, 1, 4, 1, 0)),   # multi[RT3 wg2 full1 AC1 K4 vec]
    _c("i165a16", 13, 2, 2, "plain", "f32", (1, 3, 2, 1, 1, 11, 1, 0)),   # multi[RT3 wg2 full1 AC1 K11 vec]
    _c("3s5z", 13, 2, 2, "save", "f32", (1, 4, 2, 1, 1, 10, 1, 0)),   # multi[RT4 wg2 full1 AC1 K10 vec]
    _c("o156a30", 17, 2, 2, "cont", "f32", (1, 4, 2, 1, 2, 12, 1, 1)),   # multi[RT4 wg2 full1 AC2 K12 vec reads-gi]
    _c("o192", 26, 2, 2, "plain", "f32", (1, 4, 2, 1, 1, 13, 2, 0)),   # multi[RT4 wg2 full1 AC1 K13 half]
    _c("MMM2", 7, 2, 2, "plain", "f32", (1, 3, 2, 1, 2, 13, 2, 0)),   # multi[RT3 wg2 full1 AC2 K13 half]
    _c("i224", 5, 2, 2, "plain", "f32", (1, 3, 2, 1, 2, 14, 2, 0)),   # multi[RT3 wg2 full1 AC2 K14 half]
    _c("MMM2", 7, 2, 2, "save", "f32", (1, 3, 2, 1, 2, 13, 3, 0)),   # multi[RT3 wg2 full1 AC2 K13 w2l]
    _c("i304", 5, 2, 2, "save", "f32", (1, 2, 3, 2, 2, 19, 3, 0)),   # multi[RT2 wg3 full2 AC2 K19 w2l]
    _c("a17", 40, 2, 2, "save", "f32", (1, 6, 3, 2, 2, 7, 3, 0)),   # multi[RT6 wg3 full2 AC2 K7 w2l]
    _c("2s3z", 4, 2, 2, "cont", "f32", (1, 1, 2, 2, 1, 6, 1, 1)),   # multi[RT1 wg2 full2 AC1 K6 vec reads-gi]
    _c("i97", 3, 2, 2, "cont", "f32", (1, 1, 2, 2, 1, 7, 1, 1)),   # multi[RT1 wg2 full2 AC1 K7 vec reads-gi]
    _c("2s3z", 4, 1, 2, "plain", "f32", (1, 1, 2, 2, 1, 6, 0, 0), obs_off=1),   # multi[RT1 wg2 full2 AC1 K6 elem]
    _c("2s3z", 4, 2, 2, "plain", "f32", (1, 1, 2, 2, 1, 6, 0, 0), obs_off=1),   # multi[RT1 wg2 full2 AC1 K6 elem]
    _c("o30", 6, 2, 2, "plain", "f32", (1, 1, 2, 2, 1, 3, 0, 0)),   # multi[RT1 wg2 full2 AC1 K3 elem]
    _c("o55", 4, 2, 2, "plain", "f32", (1, 1, 2, 2, 1, 5, 0, 0)),   # multi[RT1 wg2 full2 AC1 K5 elem]
    _c("2s3z", 4, 5, 2, "plain", "f32", (1, 1, 2, 2, 1, 6, 0, 0), obs_off=1),   # multi[RT1 wg2 full2 AC1 K6 elem]
    _c("o30", 6, 5, 2, "plain", "f32", (1, 1, 2, 2, 1, 3, 0, 0)),   # multi[RT1 wg2 full2 AC1 K3 elem]
    _c("o55", 4, 5, 2, "plain", "f32", (1, 1, 2, 2, 1, 5, 0, 0)),   # multi[RT1 wg2 full2 AC1 K5 elem]
    _c("2s3z", 4, 1, 2, "save", "f32", (1, 1, 2, 2, 1, 6, 0, 0), obs_off=1),   # multi[RT1 wg2 full2 AC1 K6 elem]
    _c("o30", 6, 1, 2, "save", "f32", (1, 1, 2, 2, 1, 3, 0, 0)),   # multi[RT1 wg2 full2 AC1 K3 elem]
    _c("o55", 4, 1, 2, "save", "f32", (1, 1, 2, 2, 1, 5, 0, 0)),   # multi[RT1 wg2 full2 AC1 K5 elem]
    _c("2s3z", 7, 2, 2, "plain", "f32", (1, 2, 2, 1, 1, 6, 0, 0), obs_off=1),   # multi[RT2 wg2 full1 AC1 K6 elem]
    _c("o30", 11, 2, 2, "plain", "f32", (1, 2, 2, 1, 1, 3, 0, 0)),   # multi[RT2 wg2 full1 AC1 K3 elem]
    _c("o55", 7, 2, 2, "plain", "f32", (1, 2, 2, 1, 1, 5, 0, 0)),   # multi[RT2 wg2 full1 AC1 K5 elem]
    _c("2s3z", 4, 1, 0, "plain", "f32", (1, 1, 2, 2, 1, 6, 1, 0), alias=1),   # multi[RT1 wg2 full2 AC1 K6 vec]
    _c("i160", 3, 1, 0, "plain", "f32", (1, 1, 2, 2, 1, 10, 1, 0), alias=1),   # multi[RT1 wg2 full2 AC1 K10 vec]
    _c("i41n20", 2, 1, 0, "plain", "f32", (1, 1, 3, 3, 1, 3, 1, 0), alias=1),   # multi[RT1 wg3 full3 AC1 K3 vec]
    _c("2s3z", 4, 3, 2, "plain", "f32", (1, 1, 2, 2, 1, 6, 1, 0)),   # multi[RT1 wg2 full2 AC1 K6 vec]
    _c("i60", 17, 3, 2, "plain", "f32", (1, 1, 2, 2, 1, 4, 1, 0)),   # multi[RT1 wg2 full2 AC1 K4 vec]
    _c("i161a32", 17, 3, 2, "plain", "f32", (1, 1, 2, 2, 2, 11, 1, 0)),   # multi[RT1 wg2 full2 AC2 K11 vec]
    _c("2s3z", 10, 4, 2, "plain", "x6", (2, 2, 2, 2, 1, 3, 1, 0), h_off=1),   # x6[RT2 wg2 full2 AC1 K3 vec]
    _c("i13", 17, 4, 2, "plain", "x6", (2, 2, 2, 2, 1, 3, 1, 0)),   # x6[RT2 wg2 full2 AC1 K3 vec]
    _c("i97", 9, 4, 2, "plain", "x6", (2, 2, 2, 2, 1, 3, 1, 0), rn=0, h_off=1),   # x6[RT2 wg2 full2 AC1 K3 vec]
    _c("2s3z", 7, 4, 2, "plain", "x6", (2, 2, 2, 2, 1, 3, 1, 0), h_off=1),   # x6[RT2 wg2 full2 AC1 K3 vec]
    _c("i41n20", 2, 4, 2, "plain", "x6", (2, 2, 2, 2, 1, 3, 1, 0), h_off=1),   # x6[RT2 wg2 full2 AC1 K3 vec]
    _c("i13", 11, 4, 2, "plain", "x6", (2, 2, 2, 2, 1, 3, 1, 0), h_off=1),   # x6[RT2 wg2 full2 AC1 K3 vec]
    _c("2s3z", 13, 4, 2, "plain", "x6", (2, 2, 3, 2, 1, 3, 1, 0)),   # x6[RT2 wg3 full2 AC1 K3 vec]
    _c("i60", 65, 4, 2, "plain", "x6", (2, 2, 3, 2, 1, 3, 1, 0)),   # x6[RT2 wg3 full2 AC1 K3 vec]
    _c("i97", 11, 4, 2, "plain", "x6", (2, 2, 3, 2, 1, 3, 1, 0), rn=0, h_off=1),   # x6[RT2 wg3 full2 AC1 K3 vec]
    _c("2s3z", 17, 4, 2, "plain", "x6", (2, 2, 4, 2, 1, 3, 1, 0)),   # x6[RT2 wg4 full2 AC1 K3 vec]
    _c("i41n20", 7, 4, 3, "plain", "x6", (2, 2, 6, 3, 1, 3, 1, 0)),   # x6[RT2 wg6 full3 AC1 K3 vec]
    _c("i13", 27, 4, 2, "plain", "x6", (2, 2, 4, 2, 1, 3, 1, 0)),   # x6[RT2 wg4 full2 AC1 K3 vec]
    _c("MMM2", 7, 4, 2, "plain", "x6", (2, 1, 5, 5, 2, 7, 1, 0), h_off=1),   # x6[RT1 wg5 full5 AC2 K7 vec]
    _c("i165a16", 13, 4, 2, "plain", "x6", (2, 1, 5, 5, 2, 7, 1, 0)),   # x6[RT1 wg5 full5 AC2 K7 vec]
    _c("o192", 17, 4, 2, "plain", "x6", (2, 1, 5, 5, 2, 7, 1, 0)),   # x6[RT1 wg5 full5 AC2 K7 vec]
    _c("2s3z", 4, 5, 2, "plain", "x6", (2, 1, 2, 2, 1, 3, 1, 0)),   # x6[RT1 wg2 full2 AC1 K3 vec]
    _c("i160", 3, 5, 2, "plain", "x6", (2, 1, 2, 2, 1, 5, 1, 0)),   # x6[RT1 wg2 full2 AC1 K5 vec]
    _c("i224", 2, 5, 2, "plain", "x6", (2, 1, 2, 2, 2, 7, 1, 0)),   # x6[RT1 wg2 full2 AC2 K7 vec]
    _c("2s3z", 4, 4, 2, "save", "x6", (2, 1, 2, 2, 1, 3, 1, 0)),   # x6[RT1 wg2 full2 AC1 K3 vec]
    _c("i60", 17, 4, 2, "save", "x6", (2, 1, 2, 2, 1, 3, 1, 0)),   # x6[RT1 wg2 full2 AC1 K3 vec]
    _c("i97", 3, 4, 2, "save", "x6", (2, 1, 2, 2, 1, 3, 1, 0), rn=0),   # x6[RT1 wg2 full2 AC1 K3 vec]
    _c("2s3z", 4, 4, 2, "cont", "x6", (2, 1, 2, 2, 1, 3, 1, 1)),   # x6[RT1 wg2 full2 AC1 K3 vec reads-gi]
    _c("i41n20", 1, 4, 2, "cont", "x6", (2, 1, 2, 2, 1, 3, 1, 1)),   # x6[RT1 wg2 full2 AC1 K3 vec reads-gi]
    _c("i60", 17, 4, 2, "cont", "x6", (2, 1, 2, 2, 1, 3, 1, 1)),   # x6[RT1 wg2 full2 AC1 K3 vec reads-gi]
    _c("i13", 6, 4, 2, "plain", "x6", (2, 1, 2, 2, 1, 3, 1, 0), h_off=1),   # x6[RT1 wg2 full2 AC1 K3 vec]
    _c("i97", 3, 4, 2, "plain", "x6", (2, 1, 2, 2, 1, 3, 1, 0), rn=0, h_off=1),   # x6[RT1 wg2 full2 AC1 K3 vec]
    _c("3s5z", 3, 4, 2, "save", "x6", (2, 1, 2, 2, 1, 5, 1, 0)),   # x6[RT1 wg2 full2 AC1 K5 vec]
    _c("i165a16", 4, 4, 2, "save", "x6", (2, 1, 2, 2, 1, 5, 1, 0), rn=0),   # x6[RT1 wg2 full2 AC1 K5 vec]
    _c("i160", 3, 4, 2, "save", "x6", (2, 1, 2, 2, 1, 5, 1, 0)),   # x6[RT1 wg2 full2 AC1 K5 vec]
    _c("3s5z", 3, 4, 2, "cont", "x6", (2, 1, 2, 2, 1, 5, 1, 1)),   # x6[RT1 wg2 full2 AC1 K5 vec reads-gi]
    _c("i165a16", 4, 4, 2, "cont", "x6", (2, 1, 2, 2, 1, 5, 1, 1), rn=0),   # x6[RT1 wg2 full2 AC1 K5 vec reads-gi]
    _c("i160", 3, 4, 2, "cont", "x6", (2, 1, 2, 2, 1, 5, 1, 1)),   # x6[RT1 wg2 full2 AC1 K5 vec reads-gi]
    _c("3s5z", 3, 4, 2, "plain", "x6", (2, 1, 2, 2, 1, 5, 1, 0), h_off=1),   # x6[RT1 wg2 full2 AC1 K5 vec]
    _c("i165a16", 4, 4, 2, "plain", "x6", (2, 1, 2, 2, 1, 5, 1, 0), rn=0, h_off=1),   # x6[RT1 wg2 full2 AC1 K5 vec]
    _c("MMM2", 2, 4, 2, "save", "x6", (2, 1, 2, 2, 2, 7, 1, 0)),   # x6[RT1 wg2 full2 AC2 K7 vec]
    _c("i161a32", 17, 4, 2, "save", "x6", (2, 1, 2, 2, 2, 7, 1, 0)),   # x6[RT1 wg2 full2 AC2 K7 vec]
    _c("o192", 5, 4, 2, "save", "x6", (2, 1, 2, 2, 2, 7, 1, 0)),   # x6[RT1 wg2 full2 AC2 K7 vec]
    _c("MMM2", 2, 4, 2, "cont", "x6", (2, 1, 2, 2, 2, 7, 1, 1)),   # x6[RT1 wg2 full2 AC2 K7 vec reads-gi]
    _c("i224", 2, 4, 2, "cont", "x6", (2, 1, 2, 2, 2, 7, 1, 1)),   # x6[RT1 wg2 full2 AC2 K7 vec reads-gi]
    _c("i161a32", 17, 4, 2, "cont", "x6", (2, 1, 2, 2, 2, 7, 1, 1)),   # x6[RT1 wg2 full2 AC2 K7 vec reads-gi]
    _c("2s3z", 1640, 4, 0, "nohs", "x6", (3, 3, 171, 171, 1, 3, 1, 0)),   # r6[RT3 wg171 full171 AC1 K3 vec]
    _c("i13", 2731, 4, 0, "nohs", "x6", (3, 3, 171, 171, 1, 3, 1, 0)),   # r6[RT3 wg171 full171 AC1 K3 vec]
    _c("i60", 8193, 4, 0, "nohs", "x6", (3, 3, 171, 171, 1, 3, 1, 0)),   # r6[RT3 wg171 full171 AC1 K3 vec]
    _c("i41n20", 411, 4, 0, "nohs", "x6", (3, 3, 172, 171, 1, 3, 1, 0)),   # r6[RT3 wg172 full171 AC1 K3 vec]
    _c("2s3z", 13, 40, 0, "save", "f32", (0, 1, 5, 5, 1, 6, 1, 0)),   # pipe[RT1 wg5 full5 AC1 K6 vec]
    _c("2s3z", 13, 40, 0, "save", "x6", (2, 1, 5, 5, 1, 3, 1, 0)),   # x6[RT1 wg5 full5 AC1 K3 vec]
    _c("i165a16", 13, 4, 2, "save", "x6", (2, 1, 5, 5, 2, 7, 1, 0)),   # x6[RT1 wg5 full5 AC2 K7 vec]
    _c("i165a16", 13, 5, 2, "cont", "x6", (2, 1, 5, 5, 2, 7, 1, 1)),   # x6[RT1 wg5 full5 AC2 K7 vec reads-gi]
    _c("i304", 40, 2, 2, "plain", "f32", (1, 2, 20, 20, 2, 19, 2, 0)),   # multi[RT2 wg20 full20 AC2 K19 half]
    _c("i304", 23, 5, 2, "save", "f32", (1, 2, 12, 11, 2, 19, 1, 0)),   # multi[RT2 wg12 full11 AC2 K19 vec]
    _c("o156a30", 23, 5, 2, "plain", "f32", (1, 3, 3, 3, 2, 12, 1, 0)),   # multi[RT3 wg3 full3 AC2 K12 vec]
    _c("o156a30", 23, 5, 2, "save", "f32", (1, 3, 3, 3, 2, 12, 1, 0)),   # multi[RT3 wg3 full3 AC2 K12 vec]
    _c("i224", 11, 4, 2, "plain", "f32", (1, 3, 4, 3, 2, 14, 2, 0)),   # multi[RT3 wg4 full3 AC2 K14 half]
    _c("i224", 11, 4, 2, "save", "f32", (1, 2, 6, 5, 2, 14, 1, 0)),   # multi[RT2 wg6 full5 AC2 K14 vec]
    _c("i41n20", 23, 5, 2, "plain", "x6", (2, 2, 15, 14, 1, 3, 1, 0)),   # x6[RT2 wg15 full14 AC1 K3 vec]
    _c("i41n20", 23, 5, 2, "save", "f32", (1, 8, 4, 3, 1, 3, 1, 0)),   # multi[RT8 wg4 full3 AC1 K3 vec]
    _c("i160", 23, 5, 2, "plain", "f32", (1, 5, 3, 2, 1, 10, 2, 0)),   # multi[RT5 wg3 full2 AC1 K10 half]
    _c("i161a32", 49, 5, 2, "save", "f32", (1, 2, 2, 2, 2, 11, 1, 0)),   # multi[RT2 wg2 full2 AC2 K11 vec]
    _c("i161a32", 33, 5, 2, "cont", "f32", (1, 2, 2, 1, 2, 11, 1, 1)),   # multi[RT2 wg2 full1 AC2 K11 vec reads-gi]
    _c("i224", 16, 5, 3, "cont", "f32", (1, 3, 6, 5, 2, 14, 1, 1)),   # multi[RT3 wg6 full5 AC2 K14 vec reads-gi]
    _c("a17", 23, 5, 2, "cont", "f32", (1, 4, 2, 2, 2, 7, 1, 1)),   # multi[RT4 wg2 full2 AC2 K7 vec reads-gi]
    _c("MMM2", 16, 5, 3, "cont", "f32", (1, 4, 3, 2, 2, 13, 1, 1)),   # multi[RT4 wg3 full2 AC2 K13 vec reads-gi]
    _c("2s3z", 23, 5, 2, "save", "x6", (2, 2, 4, 4, 1, 3, 1, 0)),   # x6[RT2 wg4 full4 AC1 K3 vec]
    _c("2s3z", 23, 5, 2, "cont", "x6", (2, 2, 4, 4, 1, 3, 1, 1)),   # x6[RT2 wg4 full4 AC1 K3 vec reads-gi]
    _c("i13", 27, 5, 2, "save", "x6", (2, 2, 4, 2, 1, 3, 1, 0)),   # x6[RT2 wg4 full2 AC1 K3 vec]
    _c("i41n20", 7, 4, 3, "cont", "x6", (2, 2, 6, 3, 1, 3, 1, 1)),   # x6[RT2 wg6 full3 AC1 K3 vec reads-gi]
    _c("2s3z", 61, 5, 2, "save", "f32", (1, 6, 4, 3, 1, 6, 1, 0)),   # multi[RT6 wg4 full3 AC1 K6 vec]: the most LDS allows, 305 rows
    _c("2s3z", 45, 5, 2, "plain", "f32", (1, 6, 3, 2, 1, 6, 2, 0)),   # multi[RT6 wg3 full2 AC1 K6 half]
    _c("MMM2", 40, 5, 2, "save", "f32", (1, 2, 13, 12, 2, 13, 1, 0)),   # multi[RT2 wg13 full12 AC2 K13 vec]: too many tiles for W2L
    _c("MMM2", 40, 5, 2, "plain", "f32", (1, 4, 7, 6, 2, 13, 2, 0)),   # multi[RT4 wg7 full6 AC2 K13 half]
]


# --------------------------------------------------------------------------------------------------------- inputs
def make_inputs(c):
    """numpy fp32 (integers int64): p, store (E, T+1, N, O), u (B, T, N) with -1 entries, emap (B,), lens (B,), h0 (R, 64)"""
    args = shape_args(c.shape, c.T, c.la, c.rn)
    p = seeded.seeded_state(seeded.agent_param_shapes(args), seed=11 + c.seed, scale=2.0)
    rng = np.random.default_rng(c.seed + 1000 * c.T + c.B)
    B, T, N, O, A = c.B, c.T, c.N, c.O, c.A
    E = B + 3
    store = rng.standard_normal((E, T + 1, N, O)).astype(np.float32)
    u = rng.integers(-1, A, size=(B, T, N))
    emap = rng.permutation(E)[:B]
    lens = rng.integers(1, T + 1, size=B)
    lens[0], lens[-1] = T, 1
    if B > 2:
        lens[1] = max(1, T - 1)            # rows of the first tile differ (N < 16), whatever the draw
    h0 = (rng.standard_normal((B * N, H)) * 0.5).astype(np.float32)
    return types.SimpleNamespace(args=args, p=p, store=store, u=u, emap=emap, lens=lens, h0=h0)


def resolve(inp, T, obs_t0, u_t0, with_u=True):
    """obs (B, T, N, O) fp32 and fed actions (B, T, N) int64 (-1: none) as the kernels address them"""
    B = inp.emap.shape[0]
    obs = inp.store[inp.emap][:, obs_t0:obs_t0 + T].copy()
    obs[np.arange(T)[None, :] >= inp.lens[:, None]] = 0
    fed = np.full((B, T, inp.u.shape[2]), -1, dtype=np.int64)
    if with_u:
        for t in range(T):
            if 0 <= t + u_t0 < inp.u.shape[1]:
                fed[:, t] = inp.u[:, t + u_t0]
    return obs, fed


def forward(inp, T, obs_t0, u_t0, h0, dtype=torch.float64, with_u=True):
    """-> q (B,T,N,A), hs (B,T,N,64), h_last (R,64), planes: six (T,R,64) (plane 0: (T+1,R,64)), gi: three (T,R,64)"""
    obs, fed = resolve(inp, T, obs_t0, u_t0, with_u)
    k = types.SimpleNamespace(args=inp.args, p=inp.p, obs=obs, ufed=fed, h0=np.asarray(h0, dtype=np.float32))
    u = bo.unroll(k, dtype)
    p = {n: v.detach() for n, v in u.p.items()}
    R = u.B * u.N
    hs = u.hs.detach()
    hprev = [u.h0.detach()] + [hs[:, t].reshape(R, H) for t in range(u.T)]
    pl = [[] for _ in range(6)]
    gi3 = [[] for _ in range(3)]
    bhh = p["rnn.bias_hh"]
    for t in range(u.T):
        x, gi, gh, r, z, n = bo.gates(p, u.pre[t].detach(), hprev[t])
        for i, v in enumerate((hprev[t], x, r, z, n, gh[:, 2 * H:])):
            pl[i].append(v)
        gi3[0].append(gi[:, :H] + bhh[:H])
        gi3[1].append(gi[:, H:2 * H] + bhh[H:2 * H])
        gi3[2].append(gi[:, 2 * H:])
    pl[0].append(hprev[u.T])
    return types.SimpleNamespace(q=u.q.detach(), hs=hs, h_last=u.h_last.detach(), planes=[torch.stack(v) for v in pl],
                                 gi=[torch.stack(v) for v in gi3])


def gate_sum_scale(A, entry):
    """what the stored gate sums of (r, z, n) are multiplied by: 1 for the split kernels and for one action tile; the fp32 kernels
    with two action tiles store gru_prescale()'s - the factors are READ from csrc/common.h"""
    if entry == "x6" or A <= 16:
        return (1.0, 1.0, 1.0)
    src = open(os.path.join(ROOT, "marl_amd", "csrc", "common.h")).read()
    val = lambda name: float(re.search(r"#define\s+%s\s+\(\s*(-?[0-9.eE+-]+)f\s*\)" % name, src).group(1))
    assert re.search(r"wih\[0\]\[c\] \*= MARL_NLOG2E;.*\n.*wih\[1\]\[c\] \*= MARL_NLOG2E;.*\n.*wih\[2\]\[c\] \*= MARL_2LOG2E;", src), "gru_prescale changed"
    nl, l2 = val("MARL_NLOG2E"), val("MARL_2LOG2E")
    return (nl, nl, l2)


def scaled_err(got, want):
    return bo.scaled_err(got, want)
