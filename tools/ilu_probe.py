#!/usr/bin/env python3
"""Times the exact ILU(0) / IC(0) (csrc/ilu.hip) next to ParILU / ParIC on the same matrix in the same
run and writes profiles/ilu_probe.md: the analysis (gkomi_ilu_analyse_i32, blocking), the numeric phase of compute_lu and
ic compute (wall clock around a synchronized call: the call reads its launch list back first), par_ilu_generate /
par_ic_generate, and iterations and time to a 1e-10 reduction of CG (with each IC) and GMRES (with each ILU).
Matrices: P2 (1000^2 5-point), a 3-D 7-point grid, the reference's ani4.  No threshold: the table is the result.

    python tools/ilu_probe.py [--reps 5] [--small]     (--small: 200^2 / 30^3, a quick look)"""
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


def probe(gk, name, n, rp, ci, v, reps, lines):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    rpd, cid, vd = d(rp), d(ci), d(v)
    b = d(np.ones(n))
    t_an, an = wall(lambda: solvers.FactorizationAnalysis(gk, n, rpd, cid), reps)
    work = vd.clone()

    def numeric(ic):
        work.copy_(vd)
        (an.ic_compute if ic else an.compute_lu)(rpd, cid, work)

    t_ilu, _ = wall(lambda: numeric(False), reps)
    t_ic, _ = wall(lambda: numeric(True), reps)
    row = [name, str(n), str(an.nlevels), str(an.widest_level), str(an.launches), f"{t_an:.3f}", f"{t_ilu:.3f}", f"{t_ic:.3f}"]
    for gen, solve in ((solvers.ilu_generate, "gmres"), (solvers.par_ilu_generate, "gmres"), (solvers.ic_generate, "cg"),
                       (solvers.par_ic_generate, "cg")):
        t_gen, pre = wall(lambda: gen(gk, n, rpd, cid, vd), 1)
        if solve == "cg":
            t_s, r = wall(lambda: solvers.cg_solve(gk, n, rpd, cid, vd, b, max_iters=5000, reduction=1e-10, precond=pre), reps)
        else:
            t_s, r = wall(lambda: solvers.gmres_solve(gk, n, rpd, cid, vd, b, krylov_dim=50, max_iters=5000, reduction=1e-10,
                                                      precond=pre), reps)
        row += [f"{t_gen:.2f}", f"{r['iterations']}{'' if r['converged'] else '*'}", f"{t_s:.2f}"]
    lines.append("| " + " | ".join(row) + " |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    gk = gkomi.lib()
    g2, g3 = (200, 30) if args.small else (1000, 100)
    head = ["matrix", "rows", "levels", "widest level", "launches", "analysis ms", "ILU(0) ms", "IC(0) ms"]
    for what in ("ILU(0)+GMRES", "ParILU+GMRES", "IC(0)+CG", "ParIC+CG"):
        head += [f"{what}: generate ms", "iterations", "solve ms"]
    lines = ["# Exact ILU(0) / IC(0) next to ParILU / ParIC (`tools/ilu_probe.py`)", "",
             f"Best of {args.reps} wall-clock times around synchronized calls; generate is one call, analysis of the triangular",
             "solves included.  `*`: not converged within 5000 iterations.  No threshold: the numbers are the result.", "",
             "| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    probe(gk, f"P2 {g2}^2 5-pt", *sorted_csr(*matgen.poisson_2d_5pt(g2)), args.reps, lines)
    probe(gk, f"{g3}^3 7-pt", *sorted_csr(*matgen.poisson_3d_7pt(g3)), args.reps, lines)
    probe(gk, "ani4", *sorted_csr(*ani4()), args.reps, lines)
    text = "\n".join(lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "ilu_probe.md"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
