#!/usr/bin/env python3
"""Every fused single-rhs driver that is paced by pace_fused_solve (csrc/internal.hpp) on poisson_2d_5pt(40): fused CG
plain and with block-Jacobi, fused BiCGSTAB / FCG / CGS, the fused float CG and the mixed-precision Ir.  Writes x and
host_info of every solve to an .npz.  GKOMI_HOST_WATCH is read once per host thread, so the two ways the host follows
a solve (the host_watch line, GKOMI_HOST_WATCH=0: blocking looks) are compared by running this script twice
(tests/test_host_watch_fallback_gpu.py).
usage: python tools/host_watch_solves.py OUT.npz [fixed|large]
  (default) check_every 1 and 4 to convergence, then max_iters = 3 so that the last-launch branch runs
  fixed     one pass, max_iters = 40 with reduction 0: the same launches whatever the host sees (for kernel traces)
  large     poisson_2d_5pt(1025), n = 1 050 625: n / 2 pairs are more than the 512 x 1024 lanes of the vector kernels, so
            1024 lanes run the grid-stride loop once, and n is odd, so the tail runs (at 40 x 40 neither does).  Fused CG,
            BiCGSTAB, FCG, CGS, each plain and with block-Jacobi, max_iters = 6 with reduction 0 (for bit comparisons of
            two builds of the library, GKOMI_LIB)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "repo-8852-ginkgo_amd"), os.path.join(ROOT, "tests")]
import numpy as np, torch
import gkomi, matgen
import gkomi.solvers as solvers
from gpu_util import dev, host, stream_ptr

mode = sys.argv[2] if len(sys.argv) > 2 else ""
gk = gkomi.lib()
n, rp, ci, v = matgen.poisson_2d_5pt(1025 if mode == "large" else 40)
b = np.random.default_rng(5).standard_normal(n)
rpd, cid, vd, bd = dev(rp.astype(np.int32)), dev(ci.astype(np.int32)), dev(v), dev(b)
vf, bf = dev(v.astype(np.float32)), dev(b.astype(np.float32))
jacobi = solvers.jacobi_generate(gk, n, rpd, cid, vd, max_block_size=8)
out = {}


def keep(tag, r):
    out[tag + "_x"] = host(r["x"]).copy()
    out[tag + "_info"] = np.array([r["iterations"], float(r["converged"]), float(np.ravel(r["residual_norm"])[0]),
                                   float(np.ravel(r["baseline_norm"])[0])])


def fused_f32(max_iters, reduction):
    x = torch.zeros(n, dtype=torch.float32, device="cuda:0")
    nb = gk.cg_fused_workspace_bytes_f32(n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda:0")
    info = np.zeros(4)
    gk.cg_solve_fused_f32_i32(stream_ptr(), n, len(v), rpd, cid, vf, bf, x, max_iters, reduction, 0, ws, nb, info)
    return {"x": x, "iterations": int(info[0]), "converged": bool(info[1]), "residual_norm": info[2], "baseline_norm": info[3]}


def all_solves(tag, check_every, max_iters, reduction):
    keep(tag + "cg", solvers.cg_solve(gk, n, rpd, cid, vd, bd, max_iters=max_iters, reduction=reduction, check_every=check_every))
    keep(tag + "cg_jacobi", solvers.cg_solve(gk, n, rpd, cid, vd, bd, max_iters=max_iters, reduction=reduction,
                                             check_every=check_every, precond=jacobi))
    for s in ("bicgstab", "fcg", "cgs"):
        keep(tag + s, solvers.krylov_solve(gk, s, n, rpd, cid, vd, bd, max_iters=max_iters, reduction=reduction,
                                           check_every=check_every, fused=True))
    keep(tag + "cg_f32", fused_f32(max_iters, max(reduction, 1e-5) if reduction > 0 else 0.0))
    # (the inner solves are capped too when max_iters is small: Ir must not depend on how they were followed)
    keep(tag + "ir_mixed", solvers.ir_mixed(gk, n, rpd, cid, vd, bd, max_iters=min(max_iters, 100), reduction=reduction,
                                            inner_max_iters=min(max_iters, 100)))


def large_solves(tag, check_every, max_iters, reduction):
    for name, precond in (("", None), ("_jacobi", jacobi)):
        keep(tag + "cg" + name, solvers.cg_solve(gk, n, rpd, cid, vd, bd, max_iters=max_iters, reduction=reduction,
                                                 check_every=check_every, precond=precond))
        for s in ("bicgstab", "fcg", "cgs"):
            keep(tag + s + name, solvers.krylov_solve(gk, s, n, rpd, cid, vd, bd, max_iters=max_iters, reduction=reduction,
                                                      check_every=check_every, fused=True, precond=precond))


if mode == "fixed":
    all_solves("fixed_", 4, 40, 0.0)
elif mode == "large":
    large_solves("large_", 4, 6, 0.0)
else:
    for ce in (1, 4):
        all_solves(f"ce{ce}_", ce, 1000, 1e-10)
    all_solves("cap3_", 4, 3, 1e-10)
torch.cuda.synchronize()
np.savez(sys.argv[1], **out)
print(f"solves {len(out) // 2}")
