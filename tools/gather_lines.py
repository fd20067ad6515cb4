#!/usr/bin/env python3
"""CPU count (numpy, no GPU) of what one 64-lane gather instruction of the nonzero-split CSR SpMV touches in b: distinct
64-B lines and pairs of neighbouring lanes whose addresses are neighbours (|column difference| == 1), averaged over the
gather instructions of randomly chosen tiles -- for the lane order of record (lane l of an instruction takes nonzero
base + l) and for the row-major order with stride s (wave w owns segment [w 64 S, (w + 1) 64 S) of the tile, lane l of
instruction j takes segment slot l s + j for j < s and 64 j + l beyond).  Results: profiles/r06_rowmajor_gather.md."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import matgen


def count(ci, tile, s, tiles, rng):
    """s == 0: the lane order of record"""
    S = tile // 256
    lane = np.arange(64)
    lines, adjacent, n = 0.0, 0.0, 0
    for t in rng.choice(len(ci) // tile - 1, size=tiles, replace=False):
        for w in range(4):
            for j in range(S):
                if s == 0:
                    slot = j * 256 + w * 64 + lane
                else:
                    slot = w * 64 * S + (lane * s + j if j < s else 64 * j + lane)
                cols = ci[t * tile + slot].astype(np.int64)
                lines += len(np.unique(cols // 8))
                adjacent += np.count_nonzero(np.abs(np.diff(cols)) == 1) / 63.0
                n += 1
    return lines / n, adjacent / n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tiles", type=int, default=200)
    args = ap.parse_args()
    cases = [("5-pt 1000^2", matgen.poisson_2d_5pt(1000), 1536, (0, 5, 4, 6)),
             ("7-pt 108^3", matgen.poisson_3d_7pt(108), 3072, (0, 7, 6, 8))]
    for name, (n, rp, ci, v), tile, strides in cases:
        for s in strides:
            lines, adjacent = count(np.asarray(ci), tile, s, args.tiles, np.random.default_rng(1))
            order = "lane order of record" if s == 0 else f"row-major, s = {s}"
            print(f"{name} tile {tile} {order:22s} {lines:6.2f} lines  {adjacent:5.2f} adjacent lane pairs")


if __name__ == "__main__":
    main()
