"""Every solve driver against the oracle, bit for bit, on the exact systems of tests/exact_systems.py: the same
iteration count, the same `converged`, x as bits (NaN matching NaN), and the reported norms -- the oracle's where it
reports one, the exact known value (the root of an exactly summed integer) otherwise.  No tolerance anywhere: the
certificate of test_exact_systems.py shows that on these inputs no summation order changes a bit, so the device's
regrouped reductions may not either.  The cases drive whole solves through what the generic systems never reach: a
zero right-hand side under the rhs_norm baseline (0 < 0 is false: the guards alone keep x finite until the limit),
an exact guess, convergence in one step, stagnation through p.q = 0, Gmres's lucky breakdown and its 0 / 0.

Every driver loop ends by the iteration limit (and every device-side meeting by its poll limit) whatever the values
are; a NaN never decides whether a loop goes on (krylov_driver.hpp check(), internal.hpp pace_fused_solve,
cg_persistent.hpp pcg_meet, the host loops of gmres.hip, cb_gmres.hip, idr.hip, mixed.hip)."""
import numpy as np
import pytest
import torch

import exact_systems as xs
from gkomi import formats, solvers
from gpu_util import dev, host, stream_ptr

pytestmark = pytest.mark.gpu
F = np.float32
_WANT = {}


def want(oracle, solver, case, n):
    """the oracle's (iterations, x, residual norm or None), computed once"""
    key = (solver, case, n)
    if key not in _WANT:
        _WANT[key] = xs.run(oracle, solver, case, n)
    return _WANT[key]


def sizes(solver_names, cases=None):
    """(case, n) for every case on which all of solver_names are kept"""
    out = []
    for case, kept in xs.KEPT.items():
        if all(s in kept for s in solver_names) and (cases is None or case in cases):
            out += [(case, n) for n in xs.CASES[case].sizes()]
    return out


class System:
    def __init__(self, case, n):
        self.case, self.n, self.c = case, n, xs.CASES[case]
        self.A, self.b, self.x0 = self.c.build(n)
        _, self.rp, self.ci, self.v = self.A
        self.rpd, self.cid, self.vd = dev(self.rp), dev(self.ci), dev(self.v)
        self.max_row_nnz = int(np.diff(self.rp).max())
        self.kw = dict(max_iters=self.c.max_iters, reduction=xs.REDUCTION, baseline=self.c.baseline)

    def csr(self):
        return (self.n, self.rpd, self.cid, self.vd)

    def bd(self, cols=1):
        return dev(self.b) if cols == 1 else dev(np.stack([self.b] * cols, 1))

    def xd(self, cols=1):
        return dev(self.x0) if cols == 1 else dev(np.stack([self.x0] * cols, 1))

    def baseline_norm(self, dtype=np.float64):
        if self.c.baseline == "absolute":
            return dtype(1.0)
        return np.sqrt(dtype(np.sum(self.b * self.b)))        # an integer below 2^24: exact in either type


def mismatches(what, res, expect, system, solver, dtype=np.float64, norms=None):
    """what differs between a driver's report and the oracle's (iterations, x, residual norm): a list of lines.
    dtype: of x; norms: the type the driver takes its norms in, where that is not dtype"""
    it, x, resnorm = expect
    norms = norms or dtype
    bad = []
    if res["iterations"] != it:
        bad.append(f"{what}: {res['iterations']} iterations, the oracle {it}")
    if bool(res["converged"]) != (it < system.c.max_iters):
        bad.append(f"{what}: converged = {res['converged']} after {it} of {system.c.max_iters} iterations")
    got = host(res["x"]).reshape(system.n, -1)
    cols = got.shape[1]
    for j in range(cols):
        gx = got[:, j].copy()
        if not xs.same_bits(gx, np.asarray(x, dtype)):
            diff = np.flatnonzero(~((gx == x) | (np.isnan(gx) & np.isnan(x))))
            at = int(diff[0]) if len(diff) else -1
            bad.append(f"{what}: x[:, {j}] differs in {len(diff)} entries, first at {at}: {gx[at]!r}, the oracle {x[at]!r}")
    # the reported norms: the oracle's, or the exact known |b - A x| that xs.run puts in its place; None: not exact
    want_res = None
    if resnorm is not None:
        want_res = dtype(resnorm) if norms is dtype else xs.residual_norm(system.A, system.b, x, norms)
    want_base = system.baseline_norm(norms)
    got_res = np.atleast_1d(np.asarray(res["residual_norm"], np.float64))
    got_base = np.atleast_1d(np.asarray(res["baseline_norm"], np.float64))
    for j in range(cols):
        if want_res is not None and not xs.same_bits(np.float64(got_res[j]), np.float64(want_res)):
            bad.append(f"{what}: residual_norm[{j}] = {got_res[j]!r}, expected {float(want_res)!r}")
        if not xs.same_bits(np.float64(got_base[j]), np.float64(want_base)):
            bad.append(f"{what}: baseline_norm[{j}] = {got_base[j]!r}, expected {float(want_base)!r}")
    return bad


def report(bad):
    assert not bad, "\n" + "\n".join(bad)


# ---- Cg

@pytest.mark.parametrize("case,n", sizes(["cg"]))
def test_cg(gk, oracle, case, n):
    s = System(case, n)
    e = want(oracle, "cg", case, n)
    bad = []
    run = lambda **k: solvers.cg_solve(gk, *s.csr(), s.bd(), x=s.xd(), **s.kw, **k)
    bad += mismatches("mode 0", run(mode=0), e, s, "cg")
    bad += mismatches("mode 1, check_every 5", run(mode=1, check_every=5), e, s, "cg")
    before = gk.cg_persistent_solves()
    bad += mismatches("mode 1 with the row-length hint", run(mode=1, check_every=4, max_row_nnz=s.max_row_nnz), e, s, "cg")
    if n >= xs.LARGE - 1:
        assert gk.cg_persistent_solves() == before + 1, "the single-launch kernel did not run (or gave up)"
    A = formats.Csr.from_host(gk, n, n, s.rp, s.ci, s.v)
    for name, M in (("Csr", A), ("Ell", A.to("ell"))):
        for fused in (False, True):
            res = solvers.solve_op(gk, "cg", M, s.bd(), x=s.xd(), fused=fused, check_every=5, **s.kw)
            bad += mismatches(f"solve_op on {name}, fused={fused}", res, e, s, "cg")
    report(bad)


@pytest.mark.parametrize("case,n", sizes(["cg_jacobi"]))
def test_cg_with_scalar_jacobi(gk, oracle, case, n):
    """block size 1 on 2 I: the inverse 0.5 is exact"""
    s = System(case, n)
    e = want(oracle, "cg_jacobi", case, n)
    pre = solvers.jacobi_generate(gk, *s.csr(), max_block_size=1)
    bad = []
    for mode in (0, 1):
        res = solvers.cg_solve(gk, *s.csr(), s.bd(), x=s.xd(), mode=mode, check_every=5, precond=pre, **s.kw)
        bad += mismatches(f"mode {mode}", res, e, s, "cg_jacobi")
    report(bad)


# ---- Fcg, Bicgstab, Cgs, Bicg, Ir

@pytest.mark.parametrize("solver", ["fcg", "bicgstab", "cgs"])
def test_krylov(gk, oracle, solver):
    bad = []
    for case, n in sizes([solver]):
        s = System(case, n)
        e = want(oracle, solver, case, n)
        tag = f"{case}[{n}] "
        run = lambda b, x, **k: solvers.krylov_solve(gk, solver, *s.csr(), b, x=x, check_every=5, **s.kw, **k)
        bad += mismatches(tag + "sequence", run(s.bd(), s.xd()), e, s, solver)
        bad += mismatches(tag + "sequence, 3 columns", run(s.bd(3), s.xd(3)), e, s, solver)
        bad += mismatches(tag + "fused", run(s.bd(), s.xd(), fused=True), e, s, solver)
        A = formats.Csr.from_host(gk, n, n, s.rp, s.ci, s.v)
        res = solvers.solve_op(gk, solver, A, s.bd(), x=s.xd(), fused=True, check_every=4, **s.kw)
        bad += mismatches(tag + "solve_op fused", res, e, s, solver)
    report(bad)


def test_bicg(gk, oracle):
    bad = []
    for case, n in sizes(["bicg"]):
        s = System(case, n)
        e = want(oracle, "bicg", case, n)
        for cols in (1, 3):
            res = solvers.bicg_solve(gk, *s.csr(), s.bd(cols), x=s.xd(cols), check_every=5, **s.kw)
            bad += mismatches(f"{case}[{n}] {cols} column(s)", res, e, s, "bicg")
    report(bad)


def test_ir(gk, oracle):
    bad = []
    for case, n in sizes(["ir"]):
        s = System(case, n)
        e = want(oracle, "ir", case, n)
        for cols in (1, 3):
            res = solvers.ir_solve(gk, *s.csr(), s.bd(cols), x=s.xd(cols), relaxation_factor=xs.IR_RELAXATION, **s.kw)
            bad += mismatches(f"{case}[{n}] {cols} column(s)", res, e, s, "ir")
    report(bad)


@pytest.mark.parametrize("solver", ["cg", "fcg", "bicgstab", "cgs", "bicg", "ir", "gmres"])
def test_three_different_columns(gk, oracle, solver):
    """A column that converges at once, one that never does and one that stagnates (or has converged before the first
    step) in one solve: xs.solve_columns, which the reference executor agrees with
    (test_ref_oracle_parity_solvers.py, exact-*-columns-*).  For Gmres that includes the reference's repeated
    correction of the column that stopped first, and the NaN column next to it."""
    bad = []
    for names in xs.column_sets(solver):
        for n in (xs.SMALL, xs.LARGE):
            systems = [System(c, n) for c in names]
            s = systems[0]
            b = dev(np.stack([t.b for t in systems], 1))
            x = dev(np.stack([t.x0 for t in systems], 1))
            kw = dict(max_iters=xs.MAX_ITERS, reduction=xs.REDUCTION)
            if solver == "cg":
                res = solvers.cg_solve(gk, *s.csr(), b, x=x, mode=0, **kw)
            elif solver == "bicg":
                res = solvers.bicg_solve(gk, *s.csr(), b, x=x, check_every=5, **kw)
            elif solver == "ir":
                res = solvers.ir_solve(gk, *s.csr(), b, x=x, relaxation_factor=xs.IR_RELAXATION, **kw)
            elif solver == "gmres":
                res = solvers.gmres_solve(gk, *s.csr(), b, x=x, krylov_dim=5, **kw)
            else:
                res = solvers.krylov_solve(gk, solver, *s.csr(), b, x=x, check_every=5, **kw)
            it, xe, resnorms = xs.solve_columns(oracle, solver, names, n)
            tag = f"{'-'.join(names)}[{n}]"
            if res["iterations"] != it:
                bad.append(f"{tag}: {res['iterations']} iterations, expected {it}")
            if res["converged"]:
                bad.append(f"{tag}: converged, with a column that cannot")
            got = host(res["x"])
            for j, c in enumerate(names):
                if not xs.same_bits(got[:, j].copy(), xe[:, j].copy()):
                    at = int(np.flatnonzero(~((got[:, j] == xe[:, j]) | (np.isnan(got[:, j]) & np.isnan(xe[:, j]))))[0])
                    bad.append(f"{tag}: column {j} ({c}) differs, first at {at}: {got[at, j]!r}, expected {xe[at, j]!r}")
                if resnorms is not None and not xs.same_bits(np.float64(res["residual_norm"][j]), np.float64(resnorms[j])):
                    bad.append(f"{tag}: residual_norm[{j}] = {res['residual_norm'][j]!r}, expected {resnorms[j]!r}")
    report(bad)


# ---- Gmres, CbGmres, Idr

@pytest.mark.parametrize("case,n", sizes(["gmres"]))
def test_gmres(gk, oracle, case, n):
    """krylov_dim 5 at both sizes (the multi-launch and the single-launch Arnoldi step); the cyclic shift at n = 8 with
    krylov_dim 8 and 10, where every Givens step takes the this_h == 0 branch"""
    s = System(case, n)
    e = want(oracle, "gmres", case, n)
    bad = []
    for cols in (1, 3):
        res = solvers.gmres_solve(gk, *s.csr(), s.bd(cols), x=s.xd(cols), krylov_dim=s.c.krylov_dim, **s.kw)
        bad += mismatches(f"{cols} column(s)", res, e, s, "gmres")
    report(bad)


@pytest.mark.parametrize("storage", ["keep", "reduce1"])
def test_cb_gmres(gk, oracle, storage):
    solver = "cb_gmres:" + storage
    bad = []
    for case, n in sizes([solver]):
        s = System(case, n)
        e = want(oracle, solver, case, n)
        res = solvers.cb_gmres_solve(gk, *s.csr(), s.bd(), x=s.xd(), krylov_dim=s.c.krylov_dim, storage=storage, **s.kw)
        bad += mismatches(f"{case}[{n}]", res, e, s, solver)
    report(bad)


@pytest.mark.parametrize("fused", [False, True], ids=["sequence", "fused"])
def test_idr(gk, oracle, fused):
    """every vector stays zero (or, on b = 0, becomes 0 / 0 = NaN as in the reference): any subspace gives the same"""
    bad = []
    for case, n in sizes(["idr"]):
        s = System(case, n)
        e = want(oracle, "idr", case, n)
        res = solvers.idr_solve(gk, *s.csr(), s.bd(), x=s.xd(), subspace_dim=xs.IDR_SUBSPACE_DIM, kappa=xs.IDR_KAPPA,
                                subspace=dev(xs.idr_subspace(n)), check_every=5, fused=fused, **s.kw)
        bad += mismatches(f"{case}[{n}]", res, e, s, "idr")
    report(bad)


# ---- float, mixed precision

def cg_f32(gk, s, fused):
    x = dev(s.x0.astype(F))
    args = (stream_ptr(), s.n, len(s.v), s.rpd, s.cid, dev(s.v.astype(F)), dev(s.b.astype(F)), x, s.c.max_iters,
            xs.REDUCTION, xs.BASELINES[s.c.baseline])
    nb = (gk.cg_fused_workspace_bytes_f32 if fused else gk.cg_workspace_bytes_f32)(s.n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda:0")
    info = np.zeros(4)
    (gk.cg_solve_fused_f32_i32 if fused else gk.cg_solve_f32)(*args, ws, nb, info)
    return {"x": x, "iterations": int(info[0]), "converged": bool(info[1]), "residual_norm": info[2],
            "baseline_norm": info[3]}


@pytest.mark.parametrize("fused", [False, True], ids=["sequence", "fused"])
def test_cg_f32(gk, oracle, fused):
    """gkomi_cg_solve_f32 is Cg<float> kernel by kernel and reports float norms.  The fused driver deliberately takes
    its norms in double ("Partial sums are doubles"): the double root of the same exact sum."""
    bad = []
    for case, n in sizes(["cg_f32"], cases=("Z0", "Z1", "E", "O", "K", "N", "N2")):
        s = System(case, n)
        bad += mismatches(f"{case}[{n}]", cg_f32(gk, s, fused), want(oracle, "cg_f32", case, n), s, "cg_f32", dtype=F,
                          norms=np.float64 if fused else None)
    report(bad)


def test_ir_mixed(gk, oracle):
    bad = []
    for case, n in sizes(["ir_mixed"]):
        s = System(case, n)
        res = solvers.ir_mixed(gk, *s.csr(), s.bd(), x=s.xd(), **s.kw)
        bad += mismatches(f"{case}[{n}]", res, want(oracle, "ir_mixed", case, n), s, "ir_mixed")
    report(bad)


# ---- distributed Cg over the loopback communicator (ranks = threads, as in test_distributed_native_gpu.py)

@pytest.mark.parametrize("world", [1, 2])
def test_distributed_cg(gk, oracle, world):
    import gkomi.distributed as gd
    from test_distributed_native_gpu import LoopbackComm, build_parts, loopback_lib, run_ranks
    lib = loopback_lib()
    bad = []
    for case, n in sizes(["cg"], cases=("Z0", "O", "K")):
        s = System(case, n)
        e = want(oracle, "cg", case, n)
        part, parts = build_parts(gk, world, n, s.rp, s.ci, s.v)
        bounds = [int(x) for x in part.range_bounds]
        wh = lib.loopback_world_create(world)
        out = [None] * world

        def rank_body(r):
            comm = LoopbackComm(lib, wh, r, world)
            A = gd.NativeMatrix.from_parts(*parts[r])
            lo, hi = bounds[r], bounds[r + 1]
            x = dev(s.x0[lo:hi].reshape(-1, 1))
            res = A.cg(comm, dev(s.b[lo:hi].reshape(-1, 1)), x, check_every=5, **s.kw)
            out[r] = (host(x)[:, 0].copy(), res)
            A.close()
            comm.close()

        try:
            run_ranks(world, rank_body)
        finally:
            lib.loopback_world_destroy(wh)
        res = dict(out[0][1], x=torch.from_numpy(np.concatenate([o[0] for o in out])))
        bad += mismatches(f"{case}[{n}] over {world} rank(s)", res, e, s, "cg")
        bad += [f"{case}[{n}]: rank {r} reports {out[r][1]}, rank 0 {out[0][1]}" for r in range(1, world)
                if out[r][1] != out[0][1]]
    report(bad)
