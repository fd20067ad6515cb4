"""Systems on which a whole solve is exact -- TEST INFRASTRUCTURE.

Matrices of 0, +-1 and 2 with right-hand sides of small integers: every product and every partial sum of the whole
trajectory is an integer (or an integer over a power of two) far below 2^53 -- below 2^24 for the float twins -- so
every summation order gives the same bits and a driver that regroups its reductions must still equal the reference
bit for bit, iteration count included.  They are also the degenerate inputs: a zero right-hand side, an exact guess,
convergence in one step, stagnation through a zero denominator, lucky breakdown.

Nothing here is assumed exact: `order_independent` re-solves a (solver, case) pair under a reversed and a random
symmetric permutation, which re-orders every reduction, and only a pair whose three results are identical is in
KEPT (tests/test_exact_systems.py checks every one).  A pair that fails is not given a tolerance, it is left out."""
import numpy as np

import cb_gmres_util
import idr_util

SMALL, LARGE = 301, 20001            # LARGE: odd, beyond both single-launch thresholds (16 k rows; 64 rows x 256 CUs)
MAX_ITERS, REDUCTION = 17, 1e-10
BASELINES = {"rhs_norm": 0, "initial_resnorm": 1, "absolute": 2}
F = np.float32


# ---- matrices: (n, row_ptrs, col_idxs, values)

def from_coo(n, rows, cols, vals):
    rows, cols, vals = np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(vals, np.float64)
    order = np.lexsort((cols, rows))
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return n, rp, cols[order].astype(np.int32), vals[order].copy()


def to_coo(n, rp, ci, v):
    return np.repeat(np.arange(n), np.diff(rp)), ci.astype(np.int64), v


def two_i(n):
    return from_coo(n, np.arange(n), np.arange(n), np.full(n, 2.0))


def skew(n, at=0, size=None):
    """tridiagonal, +1 above and -1 below, no diagonal; as COO triplets when placed at an offset"""
    i = np.arange(n - 1)
    rows, cols = np.concatenate([i, i + 1]) + at, np.concatenate([i + 1, i]) + at
    vals = np.concatenate([np.ones(n - 1), -np.ones(n - 1)])
    return from_coo(n, rows, cols, vals) if size is None else (rows, cols, vals)


def indef(n):
    return from_coo(n, np.arange(n), np.arange(n), np.where(np.arange(n) % 2 == 0, 1.0, -1.0))


def shift(n):
    return from_coo(n, np.arange(n), (np.arange(n) + 1) % n, np.ones(n))


def mixed(n):
    """2 I on the first half of the rows, skew on the rest (block diagonal)"""
    h = n // 2
    r, c, v = skew(n - h, at=h, size=n)
    d = np.arange(h)
    return from_coo(n, np.concatenate([d, r]), np.concatenate([d, c]), np.concatenate([np.full(h, 2.0), v]))


SYSTEMS = {"2I": two_i, "skew": skew, "indef": indef, "shift": shift, "mixed": mixed}


# ---- vectors

def b_i(n):
    return (7 * np.arange(n) % 11 - 5).astype(np.float64)


def x_i(n):
    return (3 * np.arange(n) % 5 - 2).astype(np.float64)


def signs(n, count):
    """`count` entries of +-1, then zeros: the norm is sqrt(count)"""
    out = np.zeros(n)
    k = np.arange(min(count, n))
    out[k] = np.where((k * k + k // 3) % 3 == 0, -1.0, 1.0)
    return out


def first_half(vec):
    out = vec.copy()
    out[len(vec) // 2:] = 0.0
    return out


def second_half(vec):
    out = vec.copy()
    out[:len(vec) // 2] = 0.0
    return out


def apply(mat, x):
    n, rp, ci, v = mat
    out = np.zeros(n)
    np.add.at(out, np.repeat(np.arange(n), np.diff(rp)), v * x[ci])
    return out


def _low_bit(values):
    """exponent of the lowest set bit of every nonzero double"""
    m, e = np.frexp(values[values != 0])
    m = np.abs(m * 2.0 ** 53).astype(np.int64)
    return e - 53 + np.log2((m & -m).astype(np.float64)).astype(np.int64)


def exact_norm2(r, bits=53):
    """Is |r|^2 the same in EVERY summation order and grouping in a format of `bits` significant bits?  Sufficient: all
    the squares are exact, hence multiples of 2^q for the lowest bit q among them, and their total is below
    2^(bits + q): then every partial sum of every subset is representable.  (A permutation cannot show this when the
    entries are all alike.)"""
    r = np.asarray(r, np.float64)
    if not np.isfinite(r).all():
        return False
    if not r.any():
        return True
    q = int(_low_bit(r).min())
    scaled = [int(v) for v in np.abs(r) / 2.0 ** q]      # r in units of its lowest bit: integers, exactly
    return all(v * v < 2 ** bits for v in scaled) and sum(v * v for v in scaled) < 2 ** bits


def residual(A, b, x):
    return b - apply(A, np.asarray(x, np.float64))


def residual_norm(A, b, x, dtype=np.float64):
    """|b - A x|, the root taken in `dtype`; meaningful as an exact known value where exact_norm2 says so"""
    r = residual(A, b, x)
    return dtype(np.sqrt(dtype(np.sum(r * r))))


zeros = np.zeros
e0 = lambda n: np.eye(1, n)[0].copy()


# ---- the cases: system, b(n, A), x0(n), baseline, the parity of n or sizes of its own, max_iters, krylov_dim

class Case:
    def __init__(self, name, system, b, x0, baseline="rhs_norm", even=False, max_iters=MAX_ITERS, krylov_dim=5,
                 large=True, own_sizes=None):
        self.name, self.system, self.b, self.x0, self.baseline = name, system, b, x0, baseline
        self.even, self.max_iters, self.krylov_dim, self.large, self.own_sizes = even, max_iters, krylov_dim, large, own_sizes

    def sizes(self):
        """the small and the large n of this case"""
        if self.own_sizes:
            return self.own_sizes
        small, large = (SMALL - 1, LARGE - 1) if self.even else (SMALL, LARGE)
        return (small, large) if self.large else (small,)

    def build(self, n):
        """(A, b, x0) at n rows"""
        A = SYSTEMS[self.system](n)
        return A, self.b(n, A), self.x0(n)


_CASES = [
    Case("Z0", "2I", lambda n, A: zeros(n), zeros),
    Case("Z1", "2I", lambda n, A: zeros(n), x_i),
    Case("Zabs", "2I", lambda n, A: zeros(n), zeros, baseline="absolute"),
    Case("E", "2I", lambda n, A: apply(A, x_i(n)), x_i),
    Case("O", "2I", lambda n, A: b_i(n), zeros),
    Case("O16", "2I", lambda n, A: signs(n, 256), zeros),
    Case("K", "skew", lambda n, A: b_i(n), x_i),
    Case("N", "indef", lambda n, A: np.ones(n), zeros, even=True),
    # alpha = n / 1, then beta = rho' / rho is rounded: at 20001 rows the squares that follow are no longer exact and
    # Cg, Fcg and Bicg fail the certificate, so this case exists at the small size only
    Case("Nodd", "indef", lambda n, A: np.ones(n), zeros, large=False),
    # N at sizes whose root is a power of two (and 16384 = 64 rows x 256 CUs is still a single-launch size): |b| is
    # 16 and 128, so Gmres normalises exactly and breaks down luckily at its second step
    Case("N2", "indef", lambda n, A: np.ones(n), zeros, own_sizes=(256, 16384)),
    Case("H", "shift", lambda n, A: e0(n), zeros),
    Case("Mc", "mixed", lambda n, A: first_half(b_i(n)), zeros),
    Case("Mc8", "mixed", lambda n, A: first_half(signs(n, 64)), zeros),
    Case("Ms", "mixed", lambda n, A: second_half(b_i(n)), lambda n: second_half(x_i(n))),
    Case("Zm", "mixed", lambda n, A: zeros(n), zeros),
    # Gmres on the cyclic shift: every Givens step takes the this_h == 0 branch; converges at iteration n
    Case("H8k8", "shift", lambda n, A: e0(n), zeros, own_sizes=(8,), krylov_dim=8),
    Case("H8k10", "shift", lambda n, A: e0(n), zeros, own_sizes=(8,), krylov_dim=10),
    Case("H301k400", "shift", lambda n, A: e0(n), zeros, own_sizes=(301,), max_iters=400, krylov_dim=400),
]
CASES = {c.name: c for c in _CASES}

SHORT = ("cg", "fcg", "bicgstab", "cgs", "bicg")
ALL7 = SHORT + ("gmres", "ir")
# the (solver, case) pairs that pass the certificate; every one is checked by tests/test_exact_systems.py
KEPT = {
    "Z0": ALL7 + ("cg_f32", "ir_mixed", "idr", "cg_jacobi"),
    "Z1": SHORT + ("ir", "cg_f32", "cg_jacobi"),
    "Zabs": ALL7 + ("idr", "cb_gmres:keep", "cb_gmres:reduce1", "cg_jacobi"),
    "E": ALL7 + ("cg_f32", "ir_mixed", "idr", "cb_gmres:keep", "cb_gmres:reduce1", "cg_jacobi"),
    # Gmres is not kept on O: |b| is irrational, the normalised basis vector is rounded, and both x and the residual
    # norm change in their last bits under a permutation.  O16 (|b| = 16) is its one-step case.
    "O": SHORT + ("ir", "cg_f32", "ir_mixed", "cg_jacobi"),
    "O16": ALL7 + ("cb_gmres:keep", "cb_gmres:reduce1", "cg_jacobi"),
    "K": ("cg", "bicgstab", "bicg", "ir", "cg_f32"),
    # Gmres is not kept on N and Nodd: it passes the permutations only because every entry of r0 / |r0| is the same
    # rounded number, which no permutation re-orders -- a regrouped sum of their squares differs (the device's did).
    # Gmres is kept where |r0| is zero or a power of two, so that the basis is exact: N2 is N at such sizes.
    "N": ("cg", "fcg", "bicgstab", "bicg", "ir", "cg_f32"),
    "Nodd": ("cg", "fcg", "cgs", "bicg", "ir"),
    "N2": ("cg", "fcg", "bicgstab", "bicg", "gmres", "ir", "cg_f32"),
    "H": ALL7 + ("cb_gmres:keep", "cb_gmres:reduce1"),
    "Mc": SHORT + ("ir",),
    "Mc8": ALL7,
    "Ms": ("cg", "bicgstab", "bicg", "ir"),
    "Zm": ALL7,
    "H8k8": ("gmres",),
    "H8k10": ("gmres",),
    "H301k400": ("gmres",),
}
# pairs whose iterations and x pass the certificate but whose final residual norm is not exact (exact_norm2 below):
# Ir halves its step 17 times (r has 17 binary places), Cgs on the shift grows r to 1e13.  Their norm is compared
# nowhere; tests/test_exact_systems.py checks that this set is exactly the pairs that need it.
X_ONLY = {("ir", "K"), ("ir", "N"), ("ir", "N2"), ("ir", "Nodd"), ("ir", "Ms"), ("cgs", "H")}
IR_RELAXATION = 0.5
IDR_SUBSPACE_DIM, IDR_KAPPA = 2, 0.7


def pairs(solvers=None):
    return [(s, c) for c, ss in KEPT.items() for s in ss if solvers is None or s in solvers]


# Three different columns in one solve: one that converges at once, one that never does, one that stagnates or has
# converged before the first step.  Per solver only columns whose single-column solve is kept.
def column_sets(solver):
    if solver == "gmres":       # the zero column turns to NaN and must leave its neighbours alone
        return [("Mc8", "Zm", "Mc8"), ("O16", "E", "Z0")]
    on_mixed = ("Mc", "Ms", "Zm") if solver in KEPT["Ms"] else ("Mc", "Zm", "Mc8")
    return [on_mixed, ("O", "E", "Z0")]


# ---- the oracle (and the restatements that stand in for it), one call for every solver

def idr_subspace(n):
    """the s x n subspace the tests hand to the device and to the restatement: small integers"""
    i = np.arange(n)
    return np.stack([((5 * i + k) % 7 - 3).astype(np.float64) for k in range(IDR_SUBSPACE_DIM)])


def ir_mixed_restated(oracle, n, rp, ci, v, b, x, max_iters, reduction, inner_max_iters=100, inner_reduction=1e-2,
                      relaxation=1.0):
    """core/solver/ir.cpp:188-277 with Cg<float> as the inner solver, baselines rhs_norm: the loop of
    tests/test_mixed_precision_gpu.py.  -> (x, iterations, converged, inner iterations, residual norm)"""
    vf = v.astype(F)

    def residual(x):
        ax = np.zeros((n, 1))
        oracle.ref_csr_spmv(n, 1, rp, ci, v, x.reshape(n, 1), 1, ax, 1)
        return b - ax[:, 0]

    x = x.copy()
    r = residual(x)
    goal = reduction * np.linalg.norm(b)
    it, inner_total = -1, 0
    while True:
        it += 1
        if it >= max_iters or np.linalg.norm(r) < goal:
            return x, it, it < max_iters, inner_total, float(np.linalg.norm(r))
        rf = r.astype(F)
        d = rf.copy()
        inner_total += oracle.ref_cg_solve_f32(n, rp, ci, vf, rf, d, inner_max_iters, F(inner_reduction), 0)
        x = x + relaxation * d.astype(np.float64)
        r = residual(x)


def cg_scalar_jacobi(oracle, n, rp, ci, v, b, x, max_iters, reduction, base):
    """ref_cg_solve (oracle/cg.c, core/solver/cg.cpp:107-193) with z = D^-1 r in place of the Identity's copy: the
    oracle's own kernels, scalar Jacobi (max_block_size 1) between them.  x is updated in place -> iterations"""
    diag, inv = np.zeros(n), np.zeros(n)
    oracle.ref_csr_extract_diagonal(n, rp, ci, v, diag)
    oracle.ref_jacobi_invert_diagonal(n, diag, inv)
    r, z, p, q = b.copy(), np.zeros(n), np.zeros(n), np.zeros(n)
    rho, prev_rho, beta, tau, orig = np.zeros(1), np.ones(1), np.zeros(1), np.zeros(1), np.ones(1)
    status = np.zeros(1, np.uint8)
    oracle.ref_csr_advanced_spmv(n, 1, -1.0, rp, ci, v, x, 1, 1.0, r, 1)
    if base != 2:
        oracle.ref_dense_compute_norm2(n, 1, b if base == 0 else r, 1, orig)
    it = -1
    while True:
        oracle.ref_jacobi_simple_scalar_apply(n, 1, inv, r, 1, z, 1)
        oracle.ref_dense_compute_dot(n, 1, r, 1, z, 1, rho)
        it += 1
        oracle.ref_dense_compute_norm2(n, 1, r, 1, tau)
        if it >= max_iters or tau[0] < reduction * orig[0]:
            return it
        oracle.ref_cg_step_1(n, 1, p, 1, z, 1, rho, prev_rho, status)
        oracle.ref_csr_spmv(n, 1, rp, ci, v, p, 1, q, 1)
        oracle.ref_dense_compute_dot(n, 1, p, 1, q, 1, beta)
        oracle.ref_cg_step_2(n, 1, x, 1, r, 1, p, 1, q, 1, beta, rho, status)
        prev_rho, rho = rho, prev_rho


def gmres_columns(oracle, A, b, x, krylov_dim, max_iters=MAX_ITERS, reduction=REDUCTION, base=0):
    """ref_gmres_solve (oracle/gmres.c, Gmres::apply_dense_impl, core/solver/gmres.cpp:139-372) for n x nrhs b and x:
    the same calls of the oracle's kernels, which all take a column count.  x is updated in place -> (iterations,
    residual_norm per column).  What a single column cannot show: a column that has stopped is finalized by the first
    update after it; later updates skip it in solve_krylov and multi_axpy, its `before_preconditioner` column keeps
    the old correction, and x += ... adds that correction again at every restart."""
    n, rp, ci, v = A
    nrhs, kd = b.shape[1], krylov_dim
    residual, before = np.zeros((n, nrhs)), np.zeros((n, nrhs))
    kb = np.zeros(((kd + 1) * n, nrhs))
    hess_flat = np.zeros((kd + 1) * kd * nrhs)
    hess = hess_flat.reshape(kd + 1, kd * nrhs)         # column block `it` starts at hess_flat[it * nrhs]
    gsin, gcos, rnc, y = np.zeros((kd, nrhs)), np.zeros((kd, nrhs)), np.zeros((kd + 1, nrhs)), np.zeros((kd, nrhs))
    residual_norm, orig, one, h = np.zeros(nrhs), np.ones(nrhs), np.ones(nrhs), np.zeros(nrhs)
    final = np.zeros(nrhs, np.uint64)
    status, flags = np.zeros(nrhs, np.uint8), np.zeros(2, np.uint8)

    def restart():
        residual[...] = b
        oracle.ref_csr_advanced_spmv(n, nrhs, -1.0, rp, ci, v, x, nrhs, 1.0, residual, nrhs)
        oracle.ref_dense_compute_norm2(n, nrhs, residual, nrhs, residual_norm)
        oracle.ref_gmres_restart(n, nrhs, residual, nrhs, residual_norm, rnc, kb, nrhs, final)

    def update():
        oracle.ref_gmres_solve_krylov(nrhs, rnc, hess, kd * nrhs, y, final, status)
        oracle.ref_gmres_multi_axpy(n, nrhs, kb, nrhs, y, before, nrhs, final, status)
        oracle.ref_dense_add_scaled(n, nrhs, one, nrhs, before, nrhs, x, nrhs)      # Identity preconditioner

    oracle.ref_gmres_initialize(n, nrhs, kd, b, nrhs, residual, nrhs, gsin, gcos, status)
    restart()
    if base != 2:
        oracle.ref_dense_compute_norm2(n, nrhs, b if base == 0 else residual, nrhs, orig)
    total, it = -1, 0
    while True:
        total += 1
        if total >= max_iters:
            oracle.ref_set_all_statuses(nrhs, 1, 0, status)
            break
        oracle.ref_residual_norm(nrhs, residual_norm, orig, reduction, 2, 0, status, flags)
        if flags[0]:
            break
        if it == kd:
            update()
            restart()
            it = 0
        nxt = kb[(it + 1) * n:(it + 2) * n]
        oracle.ref_csr_spmv(n, nrhs, rp, ci, v, kb[it * n:(it + 1) * n], nrhs, nxt, nrhs)
        for i in range(it + 1):
            oracle.ref_dense_compute_dot(n, nrhs, nxt, nrhs, kb[i * n:(i + 1) * n], nrhs, h)
            hess[i, it * nrhs:(it + 1) * nrhs] = h
            oracle.ref_dense_sub_scaled(n, nrhs, h, nrhs, kb[i * n:(i + 1) * n], nrhs, nxt, nrhs)
        oracle.ref_dense_compute_norm2(n, nrhs, nxt, nrhs, h)
        hess[it + 1, it * nrhs:(it + 1) * nrhs] = h
        oracle.ref_dense_inv_scale(n, nrhs, h, nrhs, nxt, nrhs)
        oracle.ref_gmres_hessenberg_qr(nrhs, gsin, gcos, residual_norm, rnc, hess_flat[it * nrhs:], kd * nrhs, it, final,
                                       status)
        it += 1
    update()
    return total, residual_norm


def solve(oracle, solver, A, b, x0, baseline="rhs_norm", max_iters=MAX_ITERS, krylov_dim=5, reduction=REDUCTION):
    """One solve of one column by the oracle -> (iterations, x, final residual norm or None where the oracle
    reports none).  cg_f32: float arrays.  idr, cb_gmres:<storage>, ir_mixed: the Python restatements."""
    n, rp, ci, v = A
    base = BASELINES[baseline]
    x = np.array(x0, np.float64)
    b = np.array(b, np.float64)
    if solver == "cg":
        return int(oracle.ref_cg_solve(n, rp, ci, v, b, x, max_iters, reduction, base, None, 0)), x, None
    if solver == "cg_jacobi":
        return cg_scalar_jacobi(oracle, n, rp, ci, v, b, x, max_iters, reduction, base), x, None
    if solver in ("fcg", "bicgstab", "cgs", "bicg"):
        return int(getattr(oracle, f"ref_{solver}_solve")(n, rp, ci, v, b, x, max_iters, reduction, base)), x, None
    if solver == "ir":
        return int(oracle.ref_ir_solve(n, rp, ci, v, IR_RELAXATION, b, x, max_iters, reduction, base)), x, None
    if solver == "gmres":
        fr = np.zeros(1)
        it = oracle.ref_gmres_solve(n, rp, ci, v, None, None, b, x, krylov_dim, max_iters, reduction, base, fr)
        return int(it), x, float(fr[0])
    if solver == "cg_f32":
        xf = x.astype(F)
        it = oracle.ref_cg_solve_f32(n, rp, ci, v.astype(F), b.astype(F), xf, max_iters, F(reduction), base)
        return int(it), xf, None
    if solver == "ir_mixed":
        assert baseline == "rhs_norm"
        xo, it, _, _, res = ir_mixed_restated(oracle, n, rp, ci, v, b, x, max_iters, reduction)
        return it, xo, res
    if solver == "idr":
        bb = b.reshape(n, 1)
        if baseline == "absolute":
            # the restatement knows rhs_norm only.  Here r0 = 0, and 0 < reduction * 1 ends the solve at its first
            # check, before any arithmetic: 0 iterations, x untouched
            assert not residual(A, b, x).any() and reduction > 0
            return 0, x, 0.0
        assert baseline == "rhs_norm"
        with np.errstate(invalid="ignore"):     # b = 0: m_kk = p_k . g_k = 0 and beta = 0 / 0, as in the reference
            res = idr_util.solve(idr_util.csr_apply(oracle, n, rp, ci, v), bb, idr_subspace(n),
                                 subspace_dim=IDR_SUBSPACE_DIM, kappa=IDR_KAPPA, max_iters=max_iters,
                                 reduction=reduction, x=x.reshape(n, 1))
        return int(res["iterations"]), res["x"][:, 0].copy(), float(np.sqrt(np.sum(res["residual"] ** 2)))
    if solver.startswith("cb_gmres:"):
        xx = x.reshape(n, 1)
        with np.errstate(all="ignore"):
            res = cb_gmres_util.solve(cb_gmres_util.CsrOperator(n, rp, ci, v), b.reshape(n, 1), xx, krylov_dim,
                                      solver.split(":")[1], max_iters, reduction, baseline)
        return int(res["iterations"]), xx[:, 0].copy(), float(res["residual_norm"][0])
    raise ValueError(solver)


def run(oracle, solver, case, n, perm=None):
    """The (solver, case) pair at n rows, optionally on P A P^T, P b, P x0 (perm[i]: where row i goes); x comes back
    un-permuted."""
    c = CASES[case]
    A, b, x0 = c.build(n)
    if perm is not None:
        rows, cols, vals = to_coo(*A)
        A = from_coo(n, perm[rows], perm[cols], vals)
        pb, px = np.zeros(n), np.zeros(n)
        pb[perm], px[perm] = b, x0
        b, x0 = pb, px
    it, x, res = solve(oracle, solver, A, b, x0, c.baseline, c.max_iters, c.krylov_dim)
    if res is None:
        # the oracle reports none: the exact known value, |b - A x| (in float for the float twin)
        f32 = x.dtype == F
        exact = exact_norm2(residual(A, b, x), 24 if f32 else 53)
        assert exact or (solver, case) in X_ONLY, f"{solver} on {case}: the residual norm is not exact"
        res = float(residual_norm(A, b, x, F if f32 else np.float64)) if exact and (solver, case) not in X_ONLY else None
    return it, (x[perm] if perm is not None else x), res


def solve_columns(oracle, solver, names, n, perm=None):
    """The cases `names` (on one matrix) as the columns of one solve -> (iterations, x as n x len(names), residual
    norms or None).  Gmres: gmres_columns.  Every other solver: each column is its single-column solve with the same
    iteration limit -- a stopped column is skipped by every step kernel -- and the count is the largest; the
    reference executor agrees (test_ref_oracle_parity_solvers.py)."""
    built = [CASES[c].build(n) for c in names]
    A = built[0][0]
    assert all(CASES[c].system == CASES[names[0]].system and CASES[c].baseline == "rhs_norm" for c in names)
    if solver != "gmres":
        single = [run(oracle, solver, c, n, perm) for c in names]
        return max(r[0] for r in single), np.stack([r[1] for r in single], 1), None
    b, x = np.stack([t[1] for t in built], 1), np.stack([t[2] for t in built], 1)
    if perm is not None:
        rows, cols, vals = to_coo(*A)
        A = from_coo(n, perm[rows], perm[cols], vals)
        pb, px = np.zeros_like(b), np.zeros_like(x)
        pb[perm], px[perm] = b, x
        b, x = pb, px
    it, res = gmres_columns(oracle, A, b, x, 5)
    return it, (x[perm] if perm is not None else x), res


def same_bits(a, b):
    """bit equality, except that any NaN matches any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and a[~na].tobytes() == b[~nb].tobytes()


def order_independent(oracle, solver, case, n):
    """The certificate: the same iterations, x (as bits, NaN matching NaN) and residual norm in the given order,
    reversed, and under a random permutation.  -> (True, result) or (False, what differed)"""
    first = run(oracle, solver, case, n)
    for what, perm in (("reversed", np.arange(n)[::-1].copy()), ("random", np.random.default_rng(n).permutation(n))):
        it, x, res = run(oracle, solver, case, n, perm)
        if it != first[0]:
            return False, f"{what}: {it} iterations, {first[0]} in the given order"
        if not same_bits(x, first[1]):
            return False, f"{what}: x differs"
        if (solver, case) in X_ONLY:
            continue
        if (res is None) != (first[2] is None) or (res is not None and not same_bits(np.float64(res), np.float64(first[2]))):
            return False, f"{what}: residual norm {res!r}, {first[2]!r} in the given order"
    return True, first
