#!/usr/bin/env python3
"""A/B of gkomi/solvers.py against another version of the same file, in one process and on one library: every public
solve function is called through both modules with the same arguments, and x (torch.equal) and every other entry of
the returned dict must be equal.  Then the working tree's module must refuse a strided b in every solve function
before anything reaches the C ABI.  Then the generate functions of the factorizations go through both modules
(generate_ab below).

    python tools/solvers_ab.py [other]

other: a file holding the other version, or a git revision whose solvers.py is taken (default HEAD~1).

Systems: 5-point Poisson 24 x 24 (n = 576) for all solvers and the 12^3 convection matrix of tests/test_krylov_gpu.py
for the nonsymmetric ones; Identity and block-Jacobi; nrhs 1 and 3; fused on and off where the function has it;
solve_op with every solver name on a Csr and an Ell."""
import ctypes
import importlib.util
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "repo-8852-ginkgo_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

import gkomi
import matgen
from gkomi import formats, solvers

REL = "repo-8852-ginkgo_amd/gkomi/solvers.py"
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


def load_other(arg):
    """the other solvers.py as a module of the gkomi package (its relative imports resolve there)"""
    with tempfile.TemporaryDirectory() as tmp:
        path = arg
        if not os.path.isfile(path):
            path = os.path.join(tmp, "solvers_other.py")
            with open(path, "wb") as f:
                f.write(subprocess.run(["git", "show", f"{arg}:{REL}"], cwd=ROOT, check=True, capture_output=True).stdout)
        spec = importlib.util.spec_from_file_location("gkomi._solvers_other", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    return mod


def convection(n3=12):
    n, rp, ci, v = matgen.poisson_3d_7pt(n3)
    v = v.copy()
    rows = np.repeat(np.arange(n), np.diff(rp))
    v[ci == rows - 1] -= 0.5
    v[ci == rows] += 0.5
    return n, rp, ci, v


class System:
    def __init__(self, gk, name, n, rp, ci, v, symmetric):
        self.name, self.n, self.symmetric = name, n, symmetric
        self.csr = (n, dev(rp), dev(ci), dev(v))
        self.b = {1: dev(np.sin(0.1 * np.arange(n))), 3: dev(np.cos(0.05 * np.arange(3 * n)).reshape(n, 3))}
        self.jacobi = {k: solvers.jacobi_generate(gk, *self.csr, max_block_size=4, nrhs=k) for k in (1, 3)}
        A = formats.Csr.from_host(gk, n, n, rp, ci, v)
        self.formats = {"csr": A, "ell": formats.Ell.from_csr(A)}


def calls(S):
    """(label, nrhs, function name, arguments after gk, keywords without b / x / the preconditioner, keyword that
    takes the preconditioner)"""
    kw = dict(max_iters=300, reduction=1e-9)
    for nrhs in (1, 3):
        for fused in ((False, True) if nrhs == 1 else (False,)):
            if S.symmetric:
                yield f"cg_solve mode={int(fused)}", nrhs, "cg_solve", S.csr, dict(kw, mode=int(fused)), "precond"
            for name in ("bicgstab", "fcg", "cgs"):
                if S.symmetric or name != "fcg":
                    yield f"krylov_solve {name} fused={fused}", nrhs, "krylov_solve", (name, *S.csr), dict(kw, fused=fused), "precond"
            yield f"idr_solve fused={fused}", nrhs, "idr_solve", S.csr, dict(kw, fused=fused, subspace_dim=2), "precond"
            for fmt, A in S.formats.items():
                for name in ("cg", "gmres", "bicgstab", "fcg", "cgs", "idr"):
                    if (S.symmetric or name not in ("cg", "fcg")) and not (fused and name == "gmres"):
                        yield (f"solve_op {name} {fmt} fused={fused}", nrhs, "solve_op", (name, A),
                               dict(kw, fused=fused, krylov_dim=20), "precond")
        yield "bicg_solve", nrhs, "bicg_solve", S.csr, kw, "precond"
        yield "ir_solve", nrhs, "ir_solve", S.csr, dict(kw, relaxation_factor=0.2, max_iters=50), "inner"
        yield "gmres_solve", nrhs, "gmres_solve", S.csr, dict(kw, krylov_dim=20), "precond"
    if S.symmetric:
        yield "ir_mixed", 1, "ir_mixed", S.csr, dict(max_iters=20, reduction=1e-12), None


def same(ra, rb):
    if set(ra) != set(rb) or not torch.equal(ra["x"], rb["x"]) or ra["x"].shape != rb["x"].shape:
        return False
    for k in ra:
        a, b = ra[k], rb[k]
        if k == "x":
            continue
        if type(a) is not type(b):
            return False
        if isinstance(a, np.ndarray):
            if a.dtype != b.dtype or not np.array_equal(a, b):
                return False
        elif a != b:
            return False
    return True


def unsorted(m):
    """every row's entries in another order (a fixed permutation per row)"""
    rp, ci, v = (np.array(x) for x in m)
    rng = np.random.default_rng(5)
    for r in range(len(rp) - 1):
        o = rng.permutation(rp[r + 1] - rp[r]) + rp[r]
        ci[rp[r]:rp[r + 1]], v[rp[r]:rp[r + 1]] = ci[o], v[o]
    return rp, ci, v


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def same_csr(a, b, values=True):
    return all(x.shape == y.shape and torch.equal(bits(x), bits(y)) for x, y in list(zip(a, b))[:3 if values else 2])


def generate_ab(gk, other):
    """par_ilu_generate, par_ic_generate, ilu_generate, ic_generate, par_ilut_generate, par_ict_generate, symbolic_cholesky
    and lu_generate through both modules.  Matrices: ani1, the 24 x 20 grid, ilu_exact_util.arrow(1100), and ani1 with
    the entries of every row permuted (for the four functions that sort; the others have no sort path and are not
    handed unsorted rows).  The IC family, symbolic_cholesky and lu_generate get spd_version of the matrix (a symmetric
    pattern).  Defaults, and approximate_select=False, fill_in_limit=1.2, iterations=2 for the threshold pair.  Every
    factor array of the exact and threshold functions and of the direct solver's must be equal by its bits (row
    pointers, column indices, values; .levels too); of the two asynchronous par_i*_generate the patterns."""
    import ilu_exact_util as xu
    import par_ilut_util as pu
    mats = {"ani1": pu.RECORDED_CASES["ani1"](), "grid_24x20": pu.RECORDED_CASES["grid_24x20"](), "arrow(1100)": xu.arrow(1100)}
    mats["ani1 unsorted"] = unsorted(mats["ani1"])
    exact = dict(approximate_select=False, fill_in_limit=1.2, iterations=2)
    runs = [("par_ilu_generate", False, {}, ("L", "U"), False), ("par_ic_generate", True, {}, ("L", "Lt"), False),
            ("ilu_generate", False, {}, ("L", "U"), True), ("ic_generate", True, {}, ("L", "Lt"), True),
            ("par_ilut_generate", False, {}, ("L", "U"), True), ("par_ilut_generate", False, exact, ("L", "U"), True),
            ("par_ict_generate", True, {}, ("L", "Lt"), True), ("par_ict_generate", True, exact, ("L", "Lt"), True)]
    cases = bad = 0

    def check(label, ok):
        nonlocal cases, bad
        cases += 1
        if not ok:
            bad += 1
            print(f"DIFFERS {label}")
    for name, m in mats.items():
        sorts = name.endswith("unsorted")
        spd = xu.spd_version(m) if not sorts else unsorted(xu.spd_version(mats["ani1"]))
        n = len(m[0]) - 1
        for fn, symmetric, kw, factors, values in runs:
            if sorts and not values:
                continue
            a = tuple(dev(x) for x in (spd if symmetric else m))
            pa, pb = (getattr(mod, fn)(gk, n, *a, **kw) for mod in (other, solvers))
            torch.cuda.synchronize()
            ok = all(same_csr(getattr(pa, f), getattr(pb, f), values) for f in factors)
            check(f"{name} {fn} {kw}", ok and getattr(pa, "levels", None) == getattr(pb, "levels", None))
        if sorts:
            continue
        a = tuple(dev(x) for x in spd)
        ra, rb = (mod.symbolic_cholesky(gk, n, a[0], a[1]) for mod in (other, solvers))
        check(f"{name} symbolic_cholesky", same_csr(ra[0], rb[0]) and same_csr(ra[1], rb[1]))
        fa, fb = (mod.lu_generate(gk, n, *a, symmetric_sparsity=True) for mod in (other, solvers))
        torch.cuda.synchronize()
        check(f"{name} lu_generate", same_csr(fa.combined, fb.combined) and torch.equal(fa.diag_idxs, fb.diag_idxs))
    print(f"generate: {cases} cases, {bad} differ")
    return bad


def main():
    other = load_other(sys.argv[1] if len(sys.argv) > 1 else "HEAD~1")
    gk = gkomi.lib()
    print(f"A = {other.__file__}\nB = {solvers.__file__}\nlibrary = {gk.path}")
    poisson = System(gk, "poisson24", *matgen.poisson_2d_5pt(24, 24), True)
    conv = System(gk, "convection12", *convection(), False)
    cases = bad = 0
    for S in (poisson, conv):
        for label, nrhs, fn, args, kw, pkey in calls(S):
            pre = S.jacobi[nrhs]
            variants = [("identity", {})]
            if pkey is not None:
                variants.append(("jacobi", {pkey: pre}))
            if fn == "bicg_solve":
                variants[1][1]["precond_t"] = pre   # block-Jacobi of a symmetric pattern; any M^-T serves the A/B
            if fn == "cg_solve":   # the callback as an integer address and as a ctypes function pointer
                variants.append(("jacobi by address", dict(precond=pre.fn, precond_ctx=pre.ctx_ptr)))
                variants.append(("jacobi by ctypes pointer", dict(precond=solvers.APPLY_FN(pre.fn), precond_ctx=pre.ctx_ptr)))
            for vname, extra in variants:
                for x0 in (False, True):   # x drawn by the function, or given as the initial guess
                    res = []
                    for mod in (other, solvers):
                        x = torch.full_like(S.b[nrhs], 0.25) if x0 else None
                        res.append(getattr(mod, fn)(gk, *args, S.b[nrhs], x=x, **kw, **extra))
                        torch.cuda.synchronize()
                    cases += 1
                    if not same(*res):
                        bad += 1
                        print(f"DIFFERS {S.name} {label} nrhs={nrhs} {vname} x0={x0}: "
                              f"A {res[0]['iterations']} {res[0]['converged']}  B {res[1]['iterations']} {res[1]['converged']}")
    # a strided b must be refused before the C ABI sees its pointer: the library that would be called raises on use
    class NoAbi:
        def __getattr__(self, name):
            raise RuntimeError(f"gk.{name} reached with a strided operand")
    n = poisson.n
    strided = torch.ones((n, 2), dtype=torch.float64, device="cuda")[:, 0]
    assert not strided.reshape(n, 1).is_contiguous()
    refused = 0
    attempts = [("bicg_solve", lambda: solvers.bicg_solve(NoAbi(), *poisson.csr, strided)),
                ("ir_solve", lambda: solvers.ir_solve(NoAbi(), *poisson.csr, strided)),
                ("gmres_solve", lambda: solvers.gmres_solve(NoAbi(), *poisson.csr, strided)),
                ("solve_op", lambda: solvers.solve_op(NoAbi(), "cg", poisson.formats["csr"], strided))]
    for name, attempt in attempts:
        try:
            attempt()
            print(f"NOT REFUSED: {name} took a strided b")
        except AssertionError:
            refused += 1
    bad += len(attempts) - refused
    print(f"{cases} cases, {bad} differ; strided b refused by {refused} of {len(attempts)}")
    bad += generate_ab(gk, other)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
