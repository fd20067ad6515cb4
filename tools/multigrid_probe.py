"""Times the fused Jacobi sweep of solver::Multigrid (gkomi_multigrid_jacobi_sweeps_f64_i32) against the same sweep
through the three existing entry points (dense copy, advanced CSR SpMV with the nonzero-split strategy,
jacobi::scalar_apply) on 2-D 5-point Poisson matrices of 256, 4 096, 65 536 and 1 048 576 rows and on the Galerkin
coarse matrix FixedCoarsening makes of each (every second row); then a whole V-cycle of a three-level hierarchy with
the fused path on and off; then Cg on the example's system with and without that V-cycle as preconditioner.

    python tools/multigrid_probe.py [--repeat 7] [--out profiles/multigrid_probe.md]

Clock: device events around a batch of `inner` back-to-back calls (so that the window is milliseconds, not one launch)
after a warm-up batch of the same shape, the two versions alternating; the figure is the median over `--repeat`
batches divided by `inner`, with the smallest and largest batch next to it.  Every timed pair is first compared bit
for bit.  Both versions are driven from Python through ctypes: the time per sweep includes the host's cost of issuing
one launch (fused) or three (sequence) wherever the device outruns the host, which is the situation of the coarse
levels of a cycle.  Cg is timed on the host around the blocking solve."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "repo-8852-ginkgo_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np
import torch

import gkomi
import matgen
from gkomi import formats, solvers

SPLIT = 4


def batches(fns, inner, repeat):
    """per function the (median, min, max) microseconds per call over `repeat` batches of `inner` calls; the functions
    alternate batch by batch"""
    for fn in fns:
        for _ in range(inner):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(repeat):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / inner)
    return [(statistics.median(t), min(t), max(t)) for t in times]


def same_bits(a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


def sweep_pair(gk, A, zero):
    """(fused, sequence) one-sweep smoothers of A as closures over their own x, and a check that they agree"""
    n = A.nrows
    dv = A.vals.device
    b = torch.from_numpy(np.cos(0.3 * np.arange(n))).to(dv).reshape(n, 1)
    x0 = torch.from_numpy(np.sin(0.17 * np.arange(n))).to(dv).reshape(n, 1)
    fused = solvers.JacobiSmoother(gk, A, 1, 0.9, fused=True)
    plain = solvers.JacobiSmoother(gk, A, 1, 0.9, fused=False)
    xf, xp = x0.clone(), x0.clone()
    fused.apply(b, xf, zero=zero)
    plain.apply(b, xp, zero=zero)
    torch.cuda.synchronize()
    assert same_bits(xf, xp), "the fused sweep and the three-call sequence differ"
    return (lambda: fused.apply(b, xf, zero=zero)), (lambda: plain.apply(b, xp, zero=zero))


def poisson(gk, g, dv):
    n, rp, ci, v = matgen.poisson_2d_5pt(g)
    return formats.Csr.from_host(gk, n, n, rp, ci, v, device=dv, strategy=SPLIT)


def hierarchy(gk, A, fused):
    halve = solvers.fixed_coarsening_factory(gk, lambda m: torch.arange(0, m.nrows, 2, dtype=torch.int32, device=m.vals.device))
    jac = lambda m: solvers.jacobi_generate(gk, m.nrows, m.row_ptrs, m.col_idxs, m.vals, max_block_size=1)
    return solvers.Multigrid(gk, A, [halve], pre_smoother=[jac], max_levels=2, min_coarse_rows=8, smoother_iters=2,
                             default_initial_guess="zero", max_iters=1, fused=fused)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a GPU"
    gk = gkomi.lib()
    dv = torch.device("cuda:0")
    lines = ["# Multigrid probe", "",
             f"Machine: {torch.cuda.get_device_name(0)}; library {gk.version().decode()}.  Clock: device events around batches of "
             f"back-to-back calls issued from Python, warm-up batch first, versions alternating; median of {args.repeat} batches "
             "per call, (min .. max) of the batches behind it.  Every pair agrees bit for bit.", "",
             "## One Jacobi sweep: fused kernel against copy + advanced SpMV (split) + scalar_apply", "",
             "| matrix | rows | nonzeros | guess | fused us | sequence us | sequence / fused |", "|---|---|---|---|---|---|---|"]
    crossover = []
    for g in (16, 64, 256, 1024):
        A = poisson(gk, g, dv)
        coarse = solvers.fixed_coarsening(gk, A.nrows, A.row_ptrs, A.col_idxs, A.vals,
                                          torch.arange(0, A.nrows, 2, dtype=torch.int32, device=dv), strategy=SPLIT).get_coarse_op()
        for label, m in ((f"poisson {g}x{g}", A), (f"its Galerkin coarse matrix", coarse)):
            inner = 200 if m.nrows <= 100000 else 50
            for zero in (False, True):
                f, p = sweep_pair(gk, m, zero)
                (fm, f0, f1), (pm, p0, p1) = batches([f, p], inner, args.repeat)
                lines.append(f"| {label} | {m.nrows} | {m.nnz} | {'zero' if zero else 'provided'} | {fm:.1f} ({f0:.1f} .. {f1:.1f}) | "
                             f"{pm:.1f} ({p0:.1f} .. {p1:.1f}) | {pm / fm:.2f} |")
                crossover.append((m.nrows, zero, pm / fm))
    slower = [(n, z, r) for n, z, r in crossover if r < 1.0]
    lines += ["", "Fused at least as fast as the sequence at every size: " + ("yes." if not slower else
              "NO -- slower at " + ", ".join(f"{n} rows ({'zero' if z else 'provided'} guess, ratio {r:.2f})" for n, z, r in slower) + "."),
              "", "## One V-cycle, three levels (every second row, twice), 2 sweeps, Identity on the coarsest level", "",
              "| fine rows | fused us | sequence us | sequence / fused |", "|---|---|---|---|"]
    for g in (64, 256, 1024):
        A = poisson(gk, g, dv)
        n = A.nrows
        b = torch.from_numpy(np.cos(0.3 * np.arange(n))).to(dv).reshape(n, 1)
        on, off = hierarchy(gk, A, True), hierarchy(gk, A, False)
        xa, xb = torch.zeros_like(b), torch.zeros_like(b)
        on.apply(b, xa)
        off.apply(b, xb)
        torch.cuda.synchronize()
        assert same_bits(xa, xb)
        (fm, f0, f1), (pm, p0, p1) = batches([lambda: on.apply(b, xa), lambda: off.apply(b, xb)], 20, args.repeat)
        lines.append(f"| {n} | {fm:.0f} ({f0:.0f} .. {f1:.0f}) | {pm:.0f} ({p0:.0f} .. {p1:.0f}) | {pm / fm:.2f} |")
    lines += ["", "## Cg on the example's system (2-D Poisson 64 x 64, reduction 1e-8), host clock around the blocking solve", "",
              "| preconditioner | iterations | ms (median of 3) |", "|---|---|---|"]
    A = poisson(gk, 64, dv)
    n = A.nrows
    b = torch.from_numpy(np.cos(0.3 * np.arange(n))).to(dv)
    mg = hierarchy(gk, A, True)
    for label, pre in (("none", None), ("one V-cycle (injection coarsening: a weak hierarchy; for the record, no claim)", mg)):
        res, times = None, []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = solvers.cg_solve(gk, n, A.row_ptrs, A.col_idxs, A.vals, b, max_iters=5000, reduction=1e-8, precond=pre)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        lines.append(f"| {label} | {res['iterations']} | {statistics.median(times[1:]):.2f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
