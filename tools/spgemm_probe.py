#!/usr/bin/env python3
"""Times the two calls of gkomi_csr_spgemm_f64_i32 (count, fill) separately with HIP events and prints the achieved
bytes/s by the model of DESIGN.md 4.18: A once (12 B per nonzero + 4 per row), every B row once per reference to it
(12 B per product), C once (12 B per entry + 4 per row).  Shapes: A A on the 1000^2 5-point and the 100^3 7-point
matrix, and A P, R (A P) for piecewise-constant prolongation over 2 x 2 and 2 x 2 x 2 aggregates.

    python tools/spgemm_probe.py [--reps 5] [--small]     (--small: 200^2 / 40^3, a quick look)

The count call blocks (it reads nnz(C) back), so its time includes that round trip."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "repo-8852-ginkgo_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import gkomi  # noqa: E402
import matgen  # noqa: E402
from gkomi import formats  # noqa: E402


def aggregation(shape, agg):
    """piecewise-constant prolongation: one 1.0 per row, aggregates of agg points per dimension"""
    idx = np.indices(shape).reshape(len(shape), -1)
    coarse = [s // agg for s in shape]
    col = np.zeros(idx.shape[1], np.int64)
    for d, c in enumerate(coarse):
        col = col * c + np.minimum(idx[d] // agg, c - 1)
    n = idx.shape[1]
    return n, int(np.prod(coarse)), np.arange(n + 1, dtype=np.int32), col.astype(np.int32), np.ones(n)


def transpose_host(nrows, ncols, rp, ci, v):
    rows = np.repeat(np.arange(nrows), np.diff(rp))
    order = np.argsort(ci, kind="stable")
    trp = np.zeros(ncols + 1, np.int64)
    np.add.at(trp, ci.astype(np.int64) + 1, 1)
    return np.cumsum(trp).astype(np.int32), rows[order].astype(np.int32), v[order]


def timed_product(gk, A, B, reps):
    s = torch.cuda.current_stream().cuda_stream
    nb = gk.csr_spgemm_workspace_bytes(A.nrows, B.ncols)
    ws = torch.empty(max(nb, 8), dtype=torch.uint8, device="cuda:0")
    ptrs = torch.empty(A.nrows + 1, dtype=torch.int32, device="cuda:0")
    nnz = ctypes.c_int64(0)

    def call(cols, vals):
        gk.csr_spgemm_f64_i32(s, A.nrows, A.ncols, A.nnz, A.row_ptrs, A.col_idxs, A.vals, B.nrows, B.ncols, B.nnz, B.row_ptrs,
                              B.col_idxs, B.vals, None, None, 0, 0, 0, None, None, None, ptrs, cols, vals, ctypes.addressof(nnz), ws, nb)

    call(None, None)
    cols = torch.empty(nnz.value, dtype=torch.int32, device="cuda:0")
    vals = torch.empty(nnz.value, dtype=torch.float64, device="cuda:0")
    t_count, t_fill = [], []
    for _ in range(reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        call(None, None)
        e[1].record()
        call(cols, vals)
        e[2].record()
        torch.cuda.synchronize()
        t_count.append(e[0].elapsed_time(e[1]))
        t_fill.append(e[1].elapsed_time(e[2]))
    lens = torch.diff(B.row_ptrs.long())
    products = int(lens[A.col_idxs.long()].sum().item())
    C = formats.Csr(gk, A.nrows, B.ncols, ptrs, cols, vals)
    model = 12 * A.nnz + 4 * A.nrows + 12 * products + 12 * C.nnz + 4 * C.nrows
    return C, products, model, float(np.median(t_count[1:])), float(np.median(t_fill[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    gk = gkomi.lib()
    g2, g3 = (200, 40) if args.small else (1000, 100)
    print("| product | rows | nnz(A) | products | nnz(C) | count ms | fill ms | model MB | count GB/s | fill GB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|")

    def row(name, A, B):
        C, products, model, tc, tf = timed_product(gk, A, B, args.reps)
        print(f"| {name} | {A.nrows} | {A.nnz} | {products} | {C.nnz} | {tc:.3f} | {tf:.3f} | {model / 1e6:.1f} | "
              f"{model / tc / 1e6:.1f} | {model / tf / 1e6:.1f} |", flush=True)
        return C

    for name, gen, shape in ((f"5-pt {g2}^2", matgen.poisson_2d_5pt, (g2, g2)), (f"7-pt {g3}^3", matgen.poisson_3d_7pt, (g3,) * 3)):
        n, rp, ci, v = gen(shape[0])
        A = formats.Csr.from_host(gk, n, n, rp, ci, v)
        row(f"A A, {name}", A, A)
        _, nc, prp, pci, pv = aggregation(shape, 2)
        P = formats.Csr.from_host(gk, n, nc, prp, pci, pv)
        R = formats.Csr.from_host(gk, nc, n, *transpose_host(n, nc, prp, pci, pv))
        AP = row(f"A P, {name}", A, P)
        row(f"R (A P), {name}", R, AP)


if __name__ == "__main__":
    main()
