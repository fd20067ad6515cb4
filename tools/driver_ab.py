#!/usr/bin/env python3
"""A/B of the Krylov drivers against another build of the library, in one process: every driver of cg_solver.hip,
krylov.hip and idr.hip solves the same small systems with both builds, and x (bit for bit), host_info and the error
codes must be equal.

    python tools/driver_ab.py path/to/other/libgkomi.so

Systems: 5-point Poisson 24 x 24 (n = 576) and the 12^3 convection matrix of tests/test_krylov_gpu.py; Identity and
block-Jacobi; nrhs 1 and 3 for the reference-sequence drivers; max_iters 0 / 5 / 1000 (immediate stop, iteration
limit, convergence); check_every 1 / 32; x aligned and 8 bytes off (the fused drivers' fallback to the reference
sequence); one Poisson system just above the single-launch CG's lower bound of 64 rows per CU."""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "repo-8852-ginkgo_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

import gkomi
import matgen
from gkomi import formats, solvers
from gkomi._lib import _Lib

dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


def convection(n3=12):
    n, rp, ci, v = matgen.poisson_3d_7pt(n3)
    v = v.copy()
    rows = np.repeat(np.arange(n), np.diff(rp))
    v[ci == rows - 1] -= 0.5
    v[ci == rows] += 0.5
    return n, rp, ci, v


class System:
    def __init__(self, name, n, rp, ci, v, symmetric):
        self.name, self.n, self.symmetric = name, n, symmetric
        self.host = (rp, ci, v)
        self.rp, self.ci, self.v = dev(rp), dev(ci), dev(v)
        self.b = {1: dev(np.sin(0.1 * np.arange(n))),
                  3: dev(np.cos(0.05 * np.arange(3 * n)).reshape(n, 3))}
        self.pre = {}   # (library, nrhs) -> block-Jacobi of that library

    def precond(self, gk, nrhs):
        key = (id(gk), nrhs)
        if key not in self.pre:
            self.pre[key] = solvers.jacobi_generate(gk, self.n, self.rp, self.ci, self.v, max_block_size=4, nrhs=nrhs)
        return self.pre[key]

    def x0(self, nrhs, misaligned):
        if not misaligned:
            return torch.zeros((self.n, nrhs), dtype=torch.float64, device="cuda")
        assert nrhs == 1
        x = torch.zeros(self.n + 1, dtype=torch.float64, device="cuda")[1:]
        assert x.data_ptr() % 16 == 8
        return x


def run(gk, S, driver, nrhs, jacobi, misaligned, kw):
    """One solve; returns (error code or None, x, host_info as a tuple of bytes)."""
    b = S.b[nrhs]
    x = S.x0(nrhs, misaligned)
    pre = S.precond(gk, nrhs) if jacobi else None
    csr = (S.n, S.rp, S.ci, S.v)
    try:
        if driver in ("cg_mode0", "cg_fused"):
            r = solvers.cg_solve(gk, *csr, b, x=x, mode=int(driver == "cg_fused"), precond=pre, **kw)
        elif driver in ("cg_op", "cg_fused_op"):
            A = formats.Csr.from_host(gk, S.n, S.n, *S.host)
            kw = {k: v for k, v in kw.items() if driver == "cg_fused_op" or k != "check_every"}
            r = solvers.solve_op(gk, "cg", A, b, x=x, fused=driver == "cg_fused_op", precond=pre, **kw)
        elif driver == "bicg":
            r = solvers.bicg_solve(gk, *csr, b, x=x, precond=pre, precond_t=pre, **kw)
        elif driver == "ir":
            kw = {k: v for k, v in kw.items() if k != "check_every"}
            r = solvers.ir_solve(gk, *csr, b, x=x, inner=pre, relaxation_factor=0.2, **kw)
        elif driver.startswith("idr"):
            r = solvers.idr_solve(gk, *csr, b, x=x, subspace_dim=2, precond=pre, fused=driver.endswith("fused"), **kw)
        else:
            name, _, how = driver.partition("_")
            r = solvers.krylov_solve(gk, name, *csr, b, x=x, precond=pre, fused=how == "fused", **kw)
    except gkomi.GkomiError as e:
        return e.code, None, None
    torch.cuda.synchronize()
    info = (r["iterations"], r["converged"], r["residual_norm"].tobytes(), r["baseline_norm"].tobytes())
    return None, x, info


def same(a, b):
    (ea, xa, ia), (eb, xb, ib) = a, b
    if ea is not None or eb is not None:
        return ea == eb
    return torch.equal(xa.contiguous().view(torch.int64), xb.contiguous().view(torch.int64)) and ia == ib


def error_codes(gk, S):
    """Return codes of bad requests (nothing is launched): workspace one byte short, bad baseline, bad max_iters."""
    out = []
    info = np.zeros(4)
    b = S.b[1].reshape(S.n, 1)
    x = torch.zeros_like(b)
    nnz = int(S.v.numel())
    for name, nbytes in (("cg", gk.cg_workspace_bytes(S.n, 1)), ("bicgstab", gk.krylov_workspace_bytes(S.n, 1))):
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        tail = (1,) if name == "cg" else ()
        for short, max_iters, baseline in ((1, 10, 0), (0, -1, 0), (0, 10, 3), (1, -1, 0)):
            try:
                getattr(gk, name + "_solve_f64_i32")(None, S.n, 1, nnz, S.rp, S.ci, S.v, 0, -1, None, None, b, x, max_iters,
                                                     1e-6, baseline, *tail, 1, ws, nbytes - short, info)
                out.append(0)
            except gkomi.GkomiError as e:
                out.append(e.code)
    return out


def main():
    other, mine = _Lib(sys.argv[1]), gkomi.lib()
    print(f"A = {other.path}\nB = {mine.path}")
    poisson = System("poisson24", *matgen.poisson_2d_5pt(24, 24), True)
    conv = System("convection12", *convection(), False)
    reference = ["cg_mode0", "cg_op", "bicgstab_solve", "fcg_solve", "cgs_solve", "bicg", "ir", "idr_solve"]
    fused = ["cg_fused", "cg_fused_op", "bicgstab_fused", "fcg_fused", "cgs_fused", "idr_fused"]
    cases = bad = 0
    for S in (poisson, conv):
        for driver in reference + fused:
            if not S.symmetric and (driver.startswith("cg") or driver.startswith("fcg")):
                continue
            for nrhs in ((1, 3) if driver in reference else (1,)):
                for misaligned in ((False, True) if driver in fused else (False,)):
                    for jacobi in (False, True):
                        for max_iters in (0, 5, 1000):
                            for check_every in (1, 32):
                                kw = dict(max_iters=max_iters, reduction=1e-9, check_every=check_every)
                                a = run(other, S, driver, nrhs, jacobi, misaligned, kw)
                                b = run(mine, S, driver, nrhs, jacobi, misaligned, kw)
                                cases += 1
                                if not same(a, b):
                                    bad += 1
                                    print(f"DIFFERS {S.name} {driver} nrhs={nrhs} jacobi={jacobi} misaligned={misaligned} "
                                          f"{kw}: A {a[0]} {a[2] and a[2][:2]}  B {b[0]} {b[2] and b[2][:2]}")
    ea, eb = error_codes(other, poisson), error_codes(mine, poisson)
    print(f"error codes A {ea}\nerror codes B {eb}")
    bad += ea != eb
    # the single-launch CG, just above its lower bound of 64 rows per CU
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = math.isqrt(64 * cus - 1) + 2
    big = System(f"poisson{g}", *matgen.poisson_2d_5pt(g, g), True)
    assert big.n >= 64 * cus
    for max_iters in (0, 5, 1000):
        res = []
        for gk in (other, mine):
            before = gk.cg_persistent_solves()
            x = big.x0(1, False)
            r = solvers.cg_solve(gk, big.n, big.rp, big.ci, big.v, big.b[1], x=x, mode=1, max_row_nnz=5,
                                 max_iters=max_iters, reduction=1e-9)
            res.append((gk.cg_persistent_solves() - before, x, r["iterations"], r["converged"],
                        r["residual_norm"].tobytes(), r["baseline_norm"].tobytes()))
        a, b = res
        ok = a[0] == b[0] == 1 and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64)) and a[2:] == b[2:]
        cases += 1
        bad += not ok
        print(f"single-launch cg n={big.n} max_iters={max_iters}: persistent solves A +{a[0]} B +{b[0]}, "
              f"{a[2]} / {b[2]} iterations, {'same bits' if ok else 'DIFFERS'}")
    print(f"{cases} cases, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
