#!/usr/bin/env python3
"""A probe, not a benchmark: times the steps of the sparse direct solver (csrc/lu.hip, solvers.lu_generate / Direct) on
5-point grids of a few sizes with HIP events and prints a table -- the elimination forest (host work behind a blocking
call), the symbolic phase (count, prefix sum, factorize, sort, transpose, spgeam), lu_factorization::initialize, the level
analysis, the numeric phase, one direct solve -- with nnz(L), the number of levels and the longest row of the combined
factor.  Banded factors have about one level per row, so the numeric phase is mostly single-workgroup runs; that is
accepted, and no test asserts a time.

Every step runs as a child process under its own time limit (it redoes the steps before it untimed); the first child
that fails or runs out of time ends the probe, nothing is started after it.  Whoever has the GPU writes the output to
profiles/lu_probe.md:

    python tools/lu_probe.py [--grids 32 64 128] [--reps 3] [--limit 120] > profiles/lu_probe.md"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ["forest", "symbolic", "initialize", "analysis", "numeric", "solve"]


def child(grid, step, reps):
    for p in (os.path.join(ROOT, "repo-8852-ginkgo_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import numpy as np
    import torch

    import gkomi
    import matgen
    from gkomi import solvers

    gk = gkomi.lib()
    n, rp, ci, v = matgen.poisson_2d_5pt(grid)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    rp, ci, v = d(rp), d(ci), d(v)
    s = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        best, out = float("inf"), None
        for _ in range(reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            out = fn()
            stop.record()
            stop.synchronize()
            best = min(best, start.elapsed_time(stop))
        return best, out

    info = {"rows": n}
    if step == "forest":
        ms, _ = timed(lambda: solvers.elimination_forest(gk, n, rp, ci))
        return dict(info, ms=ms)
    forest = solvers.elimination_forest(gk, n, rp, ci)
    if step == "symbolic":
        ms, (L, combined) = timed(lambda: solvers.symbolic_cholesky(gk, n, rp, ci, forest=forest))
        return dict(info, ms=ms, nnz_L=int(L[1].numel()), longest_row=int(torch.diff(combined[0]).max().item()))
    _, combined = solvers.symbolic_cholesky(gk, n, rp, ci, forest=forest)
    if step == "analysis":
        ms, an = timed(lambda: solvers.FactorizationAnalysis(gk, n, combined[0], combined[1]))
        return dict(info, ms=ms, levels=an.nlevels, launches=an.launches)
    f = solvers.LuFactorization(gk, n, rp, ci, combined[:2])
    frp, fc, fv = f.combined
    init = lambda: gk.lu_initialize_f64_i32(s, n, rp, ci, v, int(fc.numel()), frp, fc, fv, f.diag_idxs, f._flag, 8)
    if step == "initialize":
        ms, _ = timed(init)
        return dict(info, ms=ms)
    if step == "numeric":
        best = float("inf")
        for _ in range(reps):
            init()
            ms, _ = timed(lambda: gk.lu_factorize_f64_i32(s, n, frp, fc, fv, f.analysis.ws, f.analysis.nbytes))
            best = min(best, ms)
        return dict(info, ms=best)
    f.refactorize(v)
    direct = solvers.Direct(gk, f)
    b = torch.ones((n, 1), dtype=torch.float64, device="cuda:0")
    x = torch.zeros_like(b)
    ms, _ = timed(lambda: direct.apply(b, x))
    r = torch.zeros_like(b)
    gk.csr_spmv_f64_i32(s, n, n, 1, int(v.numel()), rp, ci, v, x, 1, r, 1, None, None, 0, 5)
    return dict(info, ms=ms, residual=float(torch.linalg.norm(r - b).item()), overrun=direct.overrun())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds per step")
    ap.add_argument("--child", nargs=2, metavar=("GRID", "STEP"))
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(child(int(args.child[0]), args.child[1], args.reps)))
        return 0
    print("# Steps of the sparse direct solver on 5-point grids (`tools/lu_probe.py`)\n")
    print(f"Best of {args.reps} HIP-event times per step, every step a child process with a limit of {args.limit} s.  A probe:")
    print("no threshold, the numbers are the result.\n")
    head = ["grid", "rows", "nnz(L)", "longest row", "levels", "launches"] + [f"{st} ms" for st in STEPS] + ["residual"]
    print("| " + " | ".join(head) + " |\n|" + "---|" * len(head))
    for grid in args.grids:
        got = {}
        for step in STEPS:
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--reps", str(args.reps),
                   "--child", str(grid), step]
            r = subprocess.run(cmd, capture_output=True, text=True)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print(f"\n{grid}^2 {step}: exit status {r.returncode}; the probe ends here.\n{r.stderr[-2000:]}")
                return 1
            got[step] = json.loads(line[0][7:])
        row = [f"{grid}^2", got["forest"]["rows"], got["symbolic"]["nnz_L"], got["symbolic"]["longest_row"], got["analysis"]["levels"],
               got["analysis"]["launches"]] + [f"{got[st]['ms']:.3f}" for st in STEPS] + [f"{got['solve']['residual']:.2e}"]
        print("| " + " | ".join(str(c) for c in row) + " |", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
