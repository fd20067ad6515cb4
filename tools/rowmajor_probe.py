#!/usr/bin/env python3
"""Row-major lane order of the nonzero-split CSR SpMV against the lane order of record, per row length: matrices of
1M rows with exactly k entries per row near the diagonal (k = 2 .. 12: odd and even strides, even ones have LDS bank
conflicts on the transposed reads), the order forced (variant bit 4) and forbidden (bit 8) taking turns, 5 rounds of
200 launches each, HIP events, median us per launch; cached and nontemporal matrix streams.  Under
`rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -- python tools/rowmajor_probe.py --once` every kernel runs
once per order, for the counters.  Results: profiles/r06_rowmajor_gather.md."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "repo-8852-ginkgo_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

import gkomi
from gpu_util import DevCsr, csr_apply_srow, dev, make_srow

SPLIT, NT, FORCE, FORBID = 4, 2 << 8, 4 << 8, 8 << 8


def fixed_rows(n, k):
    """every row k distinct columns in a strided window around the diagonal (interior rows; the ends wrap)"""
    rows = np.arange(n, dtype=np.int64)[:, None]
    cols = np.sort((rows + (np.arange(k) - k // 2) * 3) % n, axis=1)
    rp = np.arange(n + 1, dtype=np.int32) * k
    return rp, cols.reshape(-1).astype(np.int32), np.random.default_rng(k).standard_normal(n * k)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--once", action="store_true", help="one launch per kernel (counter runs)")
    args = ap.parse_args()
    gk = gkomi.lib()
    n = args.rows
    b = dev(np.sin(0.01 * np.arange(n)).reshape(n, 1))
    for k, tile in ((2, 1536), (3, 1536), (4, 1536), (5, 1536), (6, 1536), (7, 3072), (8, 3072), (12, 3072)):
        rp, ci, v = fixed_rows(n, k)
        A = DevCsr(n, n, rp, ci, v)
        srow, _ = make_srow(gk, A, tile)
        y = torch.empty((n, 1), dtype=torch.float64, device="cuda:0")
        for nt in (0, NT):
            times = {FORCE: [], FORBID: []}
            for _ in range(1 if args.once else 5):
                for order in (FORBID, FORCE):
                    run = lambda: csr_apply_srow(gk, A, b, srow, tile, y, strategy=SPLIT | nt | order, hint=k)
                    reps = 1 if args.once else 200
                    if not args.once:
                        for _ in range(20):
                            run()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        run()
                    e1.record()
                    torch.cuda.synchronize()
                    times[order].append(e0.elapsed_time(e1) * 1e3 / reps)
            base, new = statistics.median(times[FORBID]), statistics.median(times[FORCE])
            print(f"k {k:2d} tile {tile} {'nt    ' if nt else 'cached'} lane order {base:7.2f} us "
                  f"[{min(times[FORBID]):.2f}, {max(times[FORBID]):.2f}]  row-major {new:7.2f} us "
                  f"[{min(times[FORCE]):.2f}, {max(times[FORCE]):.2f}]  {100 * (new / base - 1):+.1f} %", flush=True)


if __name__ == "__main__":
    main()
