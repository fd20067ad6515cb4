#!/usr/bin/env python3
"""Times ParICT (csrc/par_ict.hip) and writes profiles/par_ict_probe.md: the whole of
gkomi.solvers.par_ict_generate, each kernel of one iteration on its own (wall clock around a synchronized call; the
count calls and the thresholds block by themselves), the number of dependency levels of L' at every sweep, and in the
same run CG to a 1e-10 reduction (iterations and time) with no preconditioner, ParIC, the exact IC(0) and ParICT.
Matrices: 1138_bus and a 2-D 5-point grid.  No threshold: the table is the result.

    python tools/par_ict_probe.py [--reps 3] [--grid 300] [--iterations 5] [--fill-in-limit 2.0]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "repo-8852-ginkgo_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import gkomi  # noqa: E402
import matgen  # noqa: E402
from gkomi import solvers  # noqa: E402


def wall(fn, reps):
    best = float("inf")
    out = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best * 1e3, out


def sorted_csr(n, rp, ci, v):
    for r in range(n):
        b, e = rp[r], rp[r + 1]
        o = np.argsort(ci[b:e], kind="stable")
        ci[b:e], v[b:e] = ci[b:e][o], v[b:e][o]
    return n, rp, ci, v


def bus_1138():
    kind, nr, nc, rows, cols, vals = matgen.read_mtx(os.path.join(ROOT, "tests", "golden", "1138_bus.mtx"))
    return (nr,) + tuple(matgen.coo_to_csr(nr, rows, cols, vals))


def one_iteration(gk, n, a, l, lt, limit, reps):
    """the kernels of ParIctState::iterate, one after the other, each timed alone -> ({kernel: ms}, (l, lt), levels)"""
    ms = {}
    ms["spgemm(L, L^T)"], llh = wall(lambda: solvers.par_ilut_spgemm(gk, n, l, lt), reps)
    ms["add_candidates"], l_new = wall(lambda: solvers.par_ict_add_candidates(gk, n, llh, a, l), reps)
    ms["analyse (sweep 1)"], sweep = wall(lambda: solvers.ParIctSweep(gk, n, l_new), reps)
    # a sweep of its own output is another sweep: time it on a fresh copy of the values
    keep = l_new[2].clone()

    def sweep_once():
        l_new[2].copy_(keep)
        sweep.compute(a)
    ms["sweep 1 (with a value copy)"], _ = wall(sweep_once, reps)
    levels = [sweep.nlevels]
    rank = max(0, int(l_new[2].numel()) - limit - 1)
    ms["approximate threshold"], thr = wall(lambda: solvers.par_ilut_threshold_approx(gk, l_new[2], rank), reps)
    ms["threshold_select (not on the default path)"], _ = wall(lambda: solvers.par_ilut_threshold_select(gk, l_new[2], rank), reps)
    ms["threshold_filter"], l2 = wall(lambda: solvers.par_ilut_threshold_filter(gk, n, l_new, thr), reps)
    ms["analyse (sweep 2)"], sweep2 = wall(lambda: solvers.ParIctSweep(gk, n, l2), reps)
    keep2 = l2[2].clone()

    def sweep_twice():
        l2[2].copy_(keep2)
        sweep2.compute(a)
    ms["sweep 2 (with a value copy)"], _ = wall(sweep_twice, reps)
    levels.append(sweep2.nlevels)
    ms["transpose"], lt2 = wall(lambda: solvers._transpose(gk, n, *l2), reps)
    return ms, (l2, lt2), levels


def probe(gk, name, n, rp, ci, v, args, lines):
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    a = (d(rp), d(ci), d(v))
    b = d(np.cos(0.3 * np.arange(n)))
    kw = dict(iterations=args.iterations, fill_in_limit=args.fill_in_limit)
    lines.append(f"## {name}: n = {n}, nnz = {len(v)}\n")
    lines.append("| what | ms (best of %d) | note |" % args.reps)
    lines.append("|---|---|---|")
    pre = {}
    for approximate in (True, False):
        t, p = wall(lambda: solvers.par_ict_generate(gk, n, *a, approximate_select=approximate, **kw), args.reps)
        tag = "approximate" if approximate else "exact"
        pre["ParICT " + tag] = p
        finite = bool(torch.isfinite(p.L[2]).all().item())
        lines.append(f"| par_ict_generate, {tag} selection | {t:.2f} | nnz(L) {int(p.L[2].numel())}, all finite {finite}, "
                     f"levels per sweep {p.levels} |")
    t, p = wall(lambda: solvers.ic_generate(gk, n, *a), args.reps)
    pre["exact IC(0)"] = p
    lines.append(f"| ic_generate (exact IC(0)) | {t:.2f} | nnz(L) {int(p.L[2].numel())}, levels {p.analysis.nlevels} |")
    t, p = wall(lambda: solvers.par_ic_generate(gk, n, *a), args.reps)
    pre["ParIC"] = p
    lines.append(f"| par_ic_generate | {t:.2f} | nnz(L) {int(p.L[2].numel())} |")
    # the first iterations, kernel by kernel
    p0 = solvers.par_ict_generate(gk, n, *a, iterations=0)
    limit = int(int(p0.L[2].numel()) * args.fill_in_limit)
    l, lt = p0.L, p0.Lt
    for it in range(min(args.iterations, 2)):
        ms, (l, lt), levels = one_iteration(gk, n, a, l, lt, limit, args.reps)
        for k, t in ms.items():
            lines.append(f"| iteration {it + 1}: {k} | {t:.3f} | |")
        lines.append(f"| iteration {it + 1}: levels of L' at its two sweeps | | {levels} |")
    t, plain = wall(lambda: solvers.cg_solve(gk, n, *a, b, max_iters=20000, reduction=1e-10), args.reps)
    lines.append(f"| CG, no preconditioner | {t:.2f} | {plain['iterations']} iterations, converged {plain['converged']} |")
    for tag, p in pre.items():
        t, res = wall(lambda: solvers.cg_solve(gk, n, *a, b, max_iters=20000, reduction=1e-10, precond=p), args.reps)
        lines.append(f"| CG + {tag} | {t:.2f} | {res['iterations']} iterations, converged {res['converged']} |")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--grid", type=int, default=300)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--fill-in-limit", type=float, default=2.0)
    args = ap.parse_args()
    gk = gkomi.lib()
    lines = ["# ParICT probe (tools/par_ict_probe.py)\n",
             f"{torch.cuda.get_device_name(0)}; {gk.version().decode()}; iterations {args.iterations}, fill_in_limit {args.fill_in_limit}.",
             "Wall clock around synchronized calls, best of the repetitions; the sweeps are timed with the copy that restores",
             "their input.  Every sweep pays one level analysis: the pattern changes with every call.  b = cos(0.3 i).\n"]
    probe(gk, "1138_bus", *sorted_csr(*bus_1138()), args, lines)
    probe(gk, f"2-D 5-point grid {args.grid} x {args.grid}", *sorted_csr(*matgen.poisson_2d_5pt(args.grid)), args, lines)
    out = os.path.join(ROOT, "profiles", "par_ict_probe.md")
    with open(out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))
    print("written", out)


if __name__ == "__main__":
    main()
