#!/usr/bin/env python3
"""Times ParILUT (csrc/par_ilut.hip) and writes profiles/par_ilut_probe.md: the whole of
gkomi.solvers.par_ilut_generate, each kernel of one iteration on its own (wall clock around a synchronized call; the
count calls and the thresholds block by themselves), the number of dependency levels of L' at every sweep, and next to
them ParILU on the same matrix in the same run, with the iterations and time of GMRES(30) to a 1e-10 reduction under
each preconditioner.  Matrices: the reference's ani4 and a 2-D 5-point grid.  No threshold: the table is the result.

    python tools/par_ilut_probe.py [--reps 5] [--grid 300] [--iterations 5] [--fill-in-limit 2.0]"""
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


def ani4():
    kind, nr, nc, rows, cols, vals = matgen.read_mtx(os.path.join(ROOT, "tests", "golden", "ani4.mtx"))
    return (nr,) + tuple(matgen.coo_to_csr(nr, rows, cols, vals))


def one_iteration(gk, n, a, l, u, limits, approximate, reps):
    """the kernels of ParIlutState::iterate, one after the other, each timed alone -> ({kernel: ms}, (l, u), levels)"""
    ms = {}
    ms["spgemm"], lu = wall(lambda: solvers.par_ilut_spgemm(gk, n, l, u), reps)
    ms["add_candidates"], (l_new, u_new) = wall(lambda: solvers.par_ilut_add_candidates(gk, n, lu, a, l, u), reps)
    ms["transpose"], u_csc = wall(lambda: solvers._transpose(gk, n, *u_new), reps)
    ms["analyse (sweep 1)"], sweep = wall(lambda: solvers.ParIlutSweep(gk, n, l_new, u_new), reps)
    # the sweep is idempotent on its own output only to rounding: time it on fresh copies
    keep = (l_new[2].clone(), u_new[2].clone())

    def sweep_once():
        l_new[2].copy_(keep[0])
        u_new[2].copy_(keep[1])
        sweep.compute(a, u_csc)
    ms["sweep 1 (with two value copies)"], _ = wall(sweep_once, reps)
    levels = [sweep.nlevels]
    l_rank = max(0, int(l_new[2].numel()) - limits[0] - 1)
    u_rank = max(0, int(u_new[2].numel()) - limits[1] - 1)
    if approximate:
        ms["approximate threshold (L' and U'^T)"], thr = wall(
            lambda: (solvers.par_ilut_threshold_approx(gk, l_new[2], l_rank), solvers.par_ilut_threshold_approx(gk, u_csc[2], u_rank)), reps)
    else:
        ms["threshold_select (L' and U')"], thr = wall(
            lambda: (solvers.par_ilut_threshold_select(gk, l_new[2], l_rank), solvers.par_ilut_threshold_select(gk, u_new[2], u_rank)), reps)
    ms["threshold_filter (L' and U')"], (l2, u2) = wall(
        lambda: (solvers.par_ilut_threshold_filter(gk, n, l_new, thr[0]), solvers.par_ilut_threshold_filter(gk, n, u_new, thr[1])), reps)
    ms["analyse (sweep 2)"], sweep2 = wall(lambda: solvers.ParIlutSweep(gk, n, l2, u2), reps)
    keep2 = (l2[2].clone(), u2[2].clone())

    def sweep_twice():
        l2[2].copy_(keep2[0])
        u2[2].copy_(keep2[1])
        sweep2.compute(a)
    ms["sweep 2 (with two value copies)"], _ = wall(sweep_twice, reps)
    levels.append(sweep2.nlevels)
    return ms, (l2, u2), levels


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
        t, p = wall(lambda: solvers.par_ilut_generate(gk, n, *a, approximate_select=approximate, **kw), args.reps)
        tag = "approximate" if approximate else "exact"
        pre["ParILUT " + tag] = p
        lines.append(f"| par_ilut_generate, {tag} selection | {t:.2f} | nnz(L) {int(p.L[2].numel())}, nnz(U) {int(p.U[2].numel())}, "
                     f"levels per sweep {p.levels} |")
    t, p = wall(lambda: solvers.par_ilu_generate(gk, n, *a), args.reps)
    pre["ParILU"] = p
    lines.append(f"| par_ilu_generate | {t:.2f} | nnz(L) {int(p.L[2].numel())}, nnz(U) {int(p.U[2].numel())} |")
    # the first iteration, kernel by kernel
    p0 = solvers.par_ilut_generate(gk, n, *a, iterations=0)
    limits = (int(int(p0.L[2].numel()) * args.fill_in_limit), int(int(p0.U[2].numel()) * args.fill_in_limit))
    l, u = p0.L, p0.U
    for it in range(min(args.iterations, 2)):
        ms, (l, u), levels = one_iteration(gk, n, a, l, u, limits, True, args.reps)
        for k, t in ms.items():
            lines.append(f"| iteration {it + 1}: {k} | {t:.3f} | |")
        lines.append(f"| iteration {it + 1}: levels of L' at its two sweeps | | {levels} |")
    plain = solvers.gmres_solve(gk, n, *a, b, krylov_dim=30, max_iters=3000, reduction=1e-10)
    lines.append(f"| GMRES(30), no preconditioner | | {plain['iterations']} iterations, converged {plain['converged']} |")
    for tag, p in pre.items():
        t, res = wall(lambda: solvers.gmres_solve(gk, n, *a, b, krylov_dim=30, max_iters=3000, reduction=1e-10, precond=p), args.reps)
        lines.append(f"| GMRES(30) + {tag} | {t:.2f} | {res['iterations']} iterations, converged {res['converged']} |")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--grid", type=int, default=300)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--fill-in-limit", type=float, default=2.0)
    args = ap.parse_args()
    gk = gkomi.lib()
    lines = ["# ParILUT probe (tools/par_ilut_probe.py)\n",
             f"{torch.cuda.get_device_name(0)}; {gk.version().decode()}; iterations {args.iterations}, fill_in_limit {args.fill_in_limit}.",
             "Wall clock around synchronized calls, best of the repetitions; the sweeps are timed with the two copies that",
             "restore their input.  Every sweep pays one level analysis: the pattern changes with every call.\n"]
    probe(gk, "ani4", *sorted_csr(*ani4()), args, lines)
    probe(gk, f"2-D 5-point grid {args.grid} x {args.grid}", *sorted_csr(*matgen.poisson_2d_5pt(args.grid)), args, lines)
    out = os.path.join(ROOT, "profiles", "par_ilut_probe.md")
    with open(out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))
    print("written", out)


if __name__ == "__main__":
    main()
