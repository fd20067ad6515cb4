#!/usr/bin/env python3
"""Times ISAI (csrc/isai.hip) against the triangular-solve apply it replaces, in one process, and writes
profiles/isai_probe.md.
  config 4   the AT-like 108^3 convection-diffusion system of bench.py, GMRES(30) to a 1e-10 reduction, ParILU with the
             factory default of 10 sweeps: no preconditioner, the triangular-solve apply (gkomi_ilu_apply_cb, the
             behaviour before ISAI), and Ilu over LowerIsai / UpperIsai at sparsity powers 1, 2, 3;
  config 3   the heterogeneous 1104^2 diffusion system of bench.py, CG: no preconditioner, the exact IC(0) with its
             triangular solves, Ic over LowerIsai.
Per variant: iterations, us per iteration, us per apply, total ms, generate ms, nnz of the inverses.  A solve is a host
clock around a synchronized call, best of --reps after one warm-up solve; an apply is device events around --applies
applies after 5 warm-up applies.  No threshold: the table is the result.

    python tools/isai_probe.py [--reps 3] [--applies 100] [--grid3d 108] [--grid2d 1104] [--powers 1 2 3]"""
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
from gkomi import formats, solvers  # noqa: E402

BREAK_EVEN_US = 158    # profiles/r04_trs_bound.md: both solves together, for ParILU to pay on config 4


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def apply_us(pre, n, count):
    b = torch.ones((n, 1), dtype=torch.float64, device="cuda:0")
    z = torch.empty_like(b)
    for _ in range(5):
        pre.apply(b, z)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(count):
        pre.apply(b, z)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / count * 1e3


def solve_row(gk, name, solve, pre, n, args, gen_ms=None, nnz=None):
    solve(pre)                                           # warm-up
    best, res = min((timed(lambda: solve(pre)) for _ in range(args.reps)), key=lambda t: t[0])
    it = max(res["iterations"], 1)
    ap = apply_us(pre, n, args.applies) if pre is not None else None
    return (f"| {name} | {res['iterations']} | {best / it * 1e3:.1f} | {'%.1f' % ap if ap is not None else ''} | {best:.2f} | "
            f"{'%.1f' % gen_ms if gen_ms is not None else ''} | {nnz if nnz is not None else ''} | {res['converged']} |")


HEAD = ["| variant | iterations | us per iteration | us per apply | total ms | generate ms | nnz of the inverses | converged |",
        "|---|---|---|---|---|---|---|---|"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--applies", type=int, default=100)
    ap.add_argument("--grid3d", type=int, default=108)
    ap.add_argument("--grid2d", type=int, default=1104)
    ap.add_argument("--powers", type=int, nargs="*", default=[1, 2, 3])
    ap.add_argument("--commit", default="", help="what the note says the numbers were taken on")
    args = ap.parse_args()
    gk = gkomi.lib()
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    lines = ["# ISAI probe (tools/isai_probe.py)\n",
             f"{torch.cuda.get_device_name(0)}; {gk.version().decode()}; {args.commit or 'working tree'}.  Every row of both tables comes",
             "from this one run: the triangular-solve rows are the behaviour before ISAI, measured beside it.",
             f"A solve: host clock around a synchronized call, best of {args.reps} after one warm-up.  An apply: device events around",
             f"{args.applies} applies after 5 warm-up applies.  Generate: one synchronized call after the library's one-time set-up.\n"]

    # ---- config 4 -----------------------------------------------------------------------------------------------
    n, rp, ci, v = matgen.at_like(args.grid3d)
    a = (d(rp), d(ci), d(v))
    A = formats.Csr(gk, n, n, *a)
    b = d(np.cos(0.3 * np.arange(n)).reshape(n, 1))
    gmres = lambda pre: solvers.solve_op(gk, "gmres", A, b, krylov_dim=30, max_iters=3000, reduction=1e-10, precond=pre)
    solvers.par_ilu_generate(gk, n, a[0].clone(), a[1], a[2], iterations=0)         # the library's one-time set-up
    gen, ilu = timed(lambda: solvers.par_ilu_generate(gk, n, a[0].clone(), a[1], a[2], iterations=0))
    lines += [f"## config 4: AT-like {args.grid3d}^3 convection-diffusion, n = {n}, nnz = {len(v)}, GMRES(30), ParILU (10 sweeps), reduction 1e-10\n",
              f"Break-even of profiles/r04_trs_bound.md: an apply (both solves together) under {BREAK_EVEN_US} us.\n"] + HEAD
    lines.append(solve_row(gk, "no preconditioner", gmres, None, n, args))
    lines.append(solve_row(gk, "ParILU, triangular solves (ParILU generate incl. the solve analysis)", gmres, ilu, n, args, gen))
    solvers.ilu_isai_from_factors(gk, n, ilu.L, ilu.U)                               # one-time set-up of the new kernels
    for power in args.powers:
        gen_isai, pre = timed(lambda: solvers.ilu_isai_from_factors(gk, n, ilu.L, ilu.U, sparsity_power=power))
        nnz = f"{int(pre.l_inverse[2].numel())} + {int(pre.u_inverse[2].numel())}"
        lines.append(solve_row(gk, f"ParILU, LowerIsai / UpperIsai, power {power} (generate: the two inverses only)", gmres, pre, n, args,
                               gen_isai, nnz))
        del pre
    lines.append("")
    del ilu, A, a, b

    # ---- config 3 -----------------------------------------------------------------------------------------------
    n, rp, ci, v = matgen.diffusion_2d_patch_ordered(args.grid2d)
    a = (d(rp), d(ci), d(v))
    A = formats.Csr(gk, n, n, *a)
    b = torch.ones((n, 1), dtype=torch.float64, device="cuda:0")
    cg = lambda pre: solvers.solve_op(gk, "cg", A, b, max_iters=20000, reduction=1e-10, precond=pre)
    solvers.ic_generate(gk, n, *a)
    gen, ic = timed(lambda: solvers.ic_generate(gk, n, *a))
    lines += [f"## config 3: heterogeneous {args.grid2d}^2 diffusion (patch ordered), n = {n}, nnz = {len(v)}, CG, exact IC(0), reduction 1e-10\n"] + HEAD
    lines.append(solve_row(gk, "no preconditioner", cg, None, n, args))
    lines.append(solve_row(gk, "IC(0), triangular solves (IC generate incl. the solve analysis)", cg, ic, n, args, gen))
    for power in args.powers[:2]:
        gen_isai, pre = timed(lambda: solvers.ic_isai_from_factor(gk, n, ic.L, sparsity_power=power))
        nnz = f"{int(pre.l_inverse[2].numel())} + {int(pre.u_inverse[2].numel())}"
        lines.append(solve_row(gk, f"IC(0), LowerIsai and its transpose, power {power} (generate: the two inverses only)", cg, pre, n,
                               args, gen_isai, nnz))
        del pre
    lines.append("")
    out = os.path.join(ROOT, "profiles", "isai_probe.md")
    with open(out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))
    print("written", out)


if __name__ == "__main__":
    main()
