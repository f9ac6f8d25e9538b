#!/usr/bin/env python3
"""HIP-event times of the three entries of the Qatten row kernel (csrc/qatten.hip) at 2s3z (N 5, U 24, S 120) and MMM2 (N 10, U 32,
S 322), 491 520 rows (4096 episodes x 120 steps) and 61 440 rows (512 episodes).  Beside each time: the bytes the entry moves, that
count at 6.0 TB/s (the streaming read rate of the chip - a floor, not a target), and for loss_bwd the time of the composition it
replaces, mix_fwd + marl_td_loss + mix_bwd.

    python tools/time_qatten.py [--iters 50] [--warmup 10] [--shape 2s3z|MMM2]

Per configuration the operands are rotated over enough buffer sets to exceed the 256 MB Infinity Cache, so a repeat does not find its
inputs cached; the median of --iters timed launches is printed.  Run each configuration under a time limit of its own."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"2s3z": (5, 24, 4, 120), "MMM2": (10, 32, 4, 322)}        # N, U, H, S
ROWS = (491520, 61440)
HBM = 6.0e12


def bytes_per_row(N, U, H, entry):
    """floats a row moves: the N U unit features, p | w_raw | c, q, and the outputs"""
    rd = N * U + H * U + H + 1 + N
    if entry == "mix_fwd":
        return 4 * (rd + 1)
    wr = N + H * U + H
    if entry == "mix_bwd":
        return 4 * (rd + 1 + wr)
    return 4 * (rd + 4 + wr + 2)           # loss_bwd: q_tot_tgt, r, term, padded in; q_tot, dq_tot out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--shape", default=None, choices=sorted(SHAPES))
    o = ap.parse_args()
    from marl_amd import ops
    dev = torch.device("cuda")
    for name in ([o.shape] if o.shape else sorted(SHAPES)):
        N, U, H, S = SHAPES[name]
        ld = (S + 3) // 4 * 4
        HW = H * U + H + 1
        ldh = (HW + 3) // 4 * 4
        for R in ROWS:
            per_set = 4 * R * (ld + 2 * ldh + 2 * N + 8)
            sets = max(2, int(np.ceil(512e6 / per_set)))
            g = torch.Generator(device=dev).manual_seed(1)
            rnd = lambda *shape: torch.randn(*shape, device=dev, generator=g)
            B = [dict(s=rnd(R, ld)[:, :S], hy=rnd(R, ldh)[:, :HW], q=rnd(R, N), q_tgt=rnd(R), r=rnd(R), term=(rnd(R) > 1.5).float(),
                      padded=(rnd(R) > 1.0).float(), q_tot=torch.empty(R, device=dev), dq=torch.empty(R, N, device=dev),
                      dhy=torch.empty(R, ldh, device=dev)[:, :H * U + H], dq_tot=torch.empty(R, device=dev)) for _ in range(sets)]
            out2 = torch.zeros(2, device=dev)
            scale = 1.0 / np.sqrt(32.0)
            a = (R, N, U, H)
            fwd = lambda b: ops.qatten_mix_fwd(ops.src(b["s"]), b["hy"], b["q"], scale, b["q_tot"], *a)
            td = lambda b: ops.td_loss(b["q_tot"], b["q_tgt"], b["r"], b["term"], b["padded"], 0.99, b["dq_tot"], out2, R)
            bwd = lambda b: ops.qatten_mix_bwd(ops.src(b["s"]), b["hy"], b["q"], scale, b["dq_tot"], b["dq"], b["dhy"], *a)
            loss = lambda b: ops.qatten_loss_bwd(ops.src(b["s"]), b["hy"], b["q"], scale, b["q_tgt"], b["r"], b["term"], b["padded"], 0.99,
                                                 b["q_tot"], b["dq"], b["dhy"], b["dq_tot"], out2, *a)

            def comp(b):
                fwd(b); td(b); bwd(b)

            def time(fn):
                for i in range(o.warmup):
                    fn(B[i % sets])
                torch.cuda.synchronize()
                ts = []
                for i in range(o.iters):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn(B[i % sets])
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1) * 1e3)
                return float(np.median(ts))

            tr, grid, lds, rounds = ops.qatten_plan(*a)
            print("%s rows %d: tile %d rows, %d workgroups, %d B LDS, %d rounds, %d buffer sets" % (name, R, tr, grid, lds, rounds, sets))
            t_comp = time(comp)
            for entry, fn in (("mix_fwd", fwd), ("mix_bwd", bwd), ("loss_bwd", loss)):
                nb = bytes_per_row(N, U, H, entry) * R
                t = time(fn)
                extra = "   composition mix_fwd + td_loss + mix_bwd %.1f us" % t_comp if entry == "loss_bwd" else ""
                print("  %-8s %8.1f us   %d B/row, %.1f MB, %.1f us at 6.0 TB/s (%.2f of it)%s"
                      % (entry, t, nb // R, nb / 1e6, nb / HBM * 1e6, t / (nb / HBM * 1e6), extra), flush=True)


if __name__ == "__main__":
    main()
