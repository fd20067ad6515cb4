"""solver::Multigrid and multigrid::FixedCoarsening in numpy, statement for statement as the reference executor computes
them: the three kcycle kernels (reference/solver/multigrid_kernels.cpp:53-119), FixedCoarsening::generate
(core/multigrid/fixed_coarsening.cpp:69-118) over csr::sort_by_column_index, csr::transpose and csr::spgemm, Ir over a
scalar Jacobi (core/solver/ir.cpp:186-276, reference/preconditioner/jacobi_kernels.cpp:565-625) and Multigrid's
generate, cycle and outer loop (core/solver/multigrid.cpp:377-705) with a trace of the calls it makes.  Every numpy
operation below is elementwise -- one rounding per product and per sum, no fused multiply-add -- and rows are walked in
stored order, so the results are the reference executor's bit for bit; tests/golden/multigrid_ref.json (recorded from
the reference by the verb multigrid of oracle/ref_driver.cpp) pins that.  The yardstick of tests/test_multigrid_gpu.py,
with the cases both test files and the driver share."""
import os

import numpy as np

import matgen
import ref_exec

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- kcycle kernels ------------------------------------------------------------------------------------

def kcycle_step_1(alpha, rho, v, g, d, e):
    """in place on g, d, e (nrows x nrhs); alpha, rho: nrhs values"""
    with np.errstate(all="ignore"):
        for i in range(g.shape[1]):
            temp = np.float64(alpha[i]) / np.float64(rho[i])
            if np.isfinite(temp):
                g[:, i] -= temp * v[:, i]
                e[:, i] *= temp
            d[:, i] = e[:, i]


def kcycle_step_2(alpha, rho, gamma, beta, zeta, d, e):
    with np.errstate(all="ignore"):
        for i in range(e.shape[1]):
            a, r, g, b, z = (np.float64(t[i]) for t in (alpha, rho, gamma, beta, zeta))
            scalar_d = z / (b - g * g / r)
            scalar_e = np.float64(1.0) - g / a * scalar_d
            if np.isfinite(scalar_d) and np.isfinite(scalar_e):
                e[:, i] = scalar_e * e[:, i] + scalar_d * d[:, i]


def kcycle_check_stop(old_norm, new_norm, rel_tol):
    with np.errstate(all="ignore"):
        return not any(np.float64(n) > np.float64(rel_tol) * np.float64(o) for o, n in zip(old_norm, new_norm))


# ---- Csr: (nrows, ncols, row_ptrs, col_idxs, vals) -------------------------------------------------------

def csr(nrows, ncols, rp, ci, v):
    return int(nrows), int(ncols), np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.asarray(v, np.float64)


def _by_position(m):
    """for k = 0, 1, ...: (rows that have a k-th stored entry, the index of that entry) -- walks every row left to
    right with whole-array operations"""
    rp = m[2].astype(np.int64)
    lens = np.diff(rp)
    for k in range(int(lens.max()) if lens.size else 0):
        rows = np.nonzero(lens > k)[0]
        yield rows, rp[rows] + k


def advanced_spmv(alpha, m, x, beta, y):
    """csr::advanced_spmv (reference/matrix/csr_kernels.cpp:102-128): y = beta y, then y += (alpha val) x[col]"""
    _, _, _, ci, v = m
    with np.errstate(all="ignore"):
        y = y * np.float64(beta)
        for rows, idx in _by_position(m):
            y[rows] += (np.float64(alpha) * v[idx])[:, None] * x[ci[idx]]
    return y


def spmv(m, x):
    """csr::spmv (:75-96): y = 0, y += val x[col]"""
    y = np.zeros((m[0], x.shape[1]))
    with np.errstate(all="ignore"):
        for rows, idx in _by_position(m):
            y[rows] += m[4][idx][:, None] * x[m[3][idx]]
    return y


def sort_by_column_index(m):
    nr, nc, rp, ci, v = m
    ci, v = ci.copy(), v.copy()
    for r in range(nr):
        order = np.argsort(ci[rp[r]:rp[r + 1]], kind="stable")
        ci[rp[r]:rp[r + 1]] = ci[rp[r]:rp[r + 1]][order]
        v[rp[r]:rp[r + 1]] = v[rp[r]:rp[r + 1]][order]
    return nr, nc, rp, ci, v


def transpose(m):
    """csr::transpose (:551-586): the entries of a column in the order of their rows"""
    nr, nc, rp, ci, v = m
    rows = np.repeat(np.arange(nr), np.diff(rp))
    order = np.argsort(ci, kind="stable")
    trp = np.zeros(nc + 1, np.int64)
    np.add.at(trp, ci.astype(np.int64) + 1, 1)
    return csr(nc, nr, np.cumsum(trp), rows[order], v[order])


def spgemm(a, b):
    """csr::spgemm (:209-252): per row of A one entry per distinct column reached, columns ascending, the value
    0.0 + sum of a b in the storage order of A's row and of B's rows"""
    rp, cols, vals = [0], [], []
    for r in range(a[0]):
        acc = {}
        for k in range(a[2][r], a[2][r + 1]):
            av, ar = a[4][k], a[3][k]
            for z in range(b[2][ar], b[2][ar + 1]):
                c = int(b[3][z])
                acc[c] = acc.get(c, np.float64(0.0)) + av * b[4][z]
        for c in sorted(acc):
            cols.append(c)
            vals.append(acc[c])
        rp.append(len(cols))
    return csr(a[0], b[1], rp, cols, vals)


class Level:
    """multigrid::MultigridLevel: fine, restrict, coarse and prolong operators as Csr tuples"""

    def __init__(self, fine, restrict, coarse, prolong):
        self.fine, self.restrict, self.coarse, self.prolong = fine, restrict, coarse, prolong


def fixed_coarsening(m, coarse_rows, skip_sorting=False):
    """FixedCoarsening::generate: sort unless skipped, R = selection (values 1, col_idxs = coarse_rows, row_ptrs 0..m),
    P = R^T, A_c = R (A P)"""
    fine = m if skip_sorting else sort_by_column_index(m)
    coarse_rows = np.asarray(coarse_rows, np.int32)
    nc = len(coarse_rows)
    restrict = csr(nc, fine[0], np.arange(nc + 1), coarse_rows, np.ones(nc))
    prolong = transpose(restrict)
    return Level(fine, restrict, spgemm(restrict, spgemm(fine, prolong)), prolong)


# ---- smoothers and solvers: apply(b, x, zero=False) -> x, b and x n x nrhs ---------------------------------

def inverted_diagonal(m):
    """csr::extract_diagonal (the first stored entry on the diagonal, 0 without one) and jacobi::invert_diagonal
    (reference/preconditioner/jacobi_kernels.cpp:596-608: a zero counts as one)"""
    nr, _, rp, ci, v = m
    d = np.zeros(nr)
    for r in range(nr):
        hit = np.nonzero(ci[rp[r]:rp[r + 1]] == r)[0]
        if hit.size:
            d[r] = v[rp[r] + hit[0]]
    with np.errstate(all="ignore"):
        return 1.0 / np.where(d == 0.0, 1.0, d)


def jacobi_sweeps(m, inv_diag, relax, b, x, sweeps, zero_guess):
    """`sweeps` iterations of Ir over a scalar Jacobi: x = 1 x + (relax (b - A x)) inv_diag; -> the new x"""
    x = np.zeros_like(b) if zero_guess else x.copy()
    with np.errstate(all="ignore"):
        for it in range(sweeps):
            r = b if (it == 0 and zero_guess) else advanced_spmv(-1.0, m, x, 1.0, b.copy())
            x = np.float64(1.0) * x + (np.float64(relax) * r) * inv_diag[:, None]
    return x


class JacobiSmoother:
    """what build_smoother(Jacobi(max_block_size 1), iterations, relaxation) generates on a matrix"""
    uses_initial_guess = True

    def __init__(self, m, iterations=1, relax=0.9):
        self.m, self.inv, self.iterations, self.relax = m, inverted_diagonal(m), iterations, relax

    def apply(self, b, x, zero=False):
        x[:] = jacobi_sweeps(self.m, self.inv, self.relax, b, x, self.iterations, zero)
        return x


class Identity:
    uses_initial_guess = False

    def __init__(self, m=None):
        pass

    def apply(self, b, x, zero=False):
        x[:] = b
        return x

    def apply_advanced(self, alpha, b, beta, x):
        x[:] = np.float64(beta) * x
        x[:] = x + np.float64(alpha) * b
        return x


class Direct:
    """experimental::solver::Direct over Lu with symmetric_sparsity (tests/lu_util.py)"""
    uses_initial_guess = False

    def __init__(self, m):
        import lu_util
        self.combined = lu_util.lu_generate((m[2], m[3], m[4]))[0]

    def apply(self, b, x, zero=False):
        import lu_util
        x[:] = lu_util.direct_apply(self.combined, b)
        return x

    def apply_advanced(self, alpha, b, beta, x):
        """the upper solver's advanced apply: solve, scale x, add_scaled"""
        import lu_util
        plain = lu_util.direct_apply(self.combined, b)
        x[:] = np.float64(beta) * x
        x[:] = x + np.float64(alpha) * plain
        return x


class Cg:
    """solver::Cg with an Iteration criterion (core/solver/cg.cpp, reference/solver/cg_kernels.cpp) and no
    preconditioner: it takes x as its initial guess"""
    uses_initial_guess = True
    ITERATIONS = 10

    def __init__(self, m):
        self.m = m

    def apply(self, b, x, zero=False):
        r = advanced_spmv(-1.0, self.m, x, 1.0, b.copy())
        p = np.zeros_like(b)
        prev_rho = np.ones(b.shape[1])
        with np.errstate(all="ignore"):
            for it in range(self.ITERATIONS + 1):
                z = r
                rho = dot(r, z)
                if it >= self.ITERATIONS:
                    break
                for j in range(b.shape[1]):
                    p[:, j] = z[:, j] if prev_rho[j] == 0.0 else z[:, j] + (rho[j] / prev_rho[j]) * p[:, j]
                q = spmv(self.m, p)
                beta = dot(p, q)
                x_new, r_new = x.copy(), r.copy()
                for j in range(b.shape[1]):
                    if beta[j] != 0.0:
                        tmp = rho[j] / beta[j]
                        x_new[:, j] = x[:, j] + tmp * p[:, j]
                        r_new[:, j] = r[:, j] - tmp * q[:, j]
                x[:], r = x_new, r_new
                prev_rho = rho
        return x


def norm2(v):
    """dense::compute_norm2 of the reference: the squares added in row order, then the root"""
    acc = np.zeros(v.shape[1])
    for row in v:
        acc = acc + row * row
    return np.sqrt(acc)


CYCLES = ("v", "f", "w")
MID_CASES = ("both", "post_smoother", "pre_smoother", "standalone")


class Multigrid:
    """solver::Multigrid.  mg_level: a list of callables matrix -> Level; the smoother lists and coarsest_solver hold
    callables matrix -> object with apply(b, x, zero) (and uses_initial_guess) or None.  criteria: max_iters and,
    optionally, (reduction, baseline) of a ResidualNorm.  trace: a list that receives (what, level) per call."""

    def __init__(self, matrix, mg_level, pre_smoother=(), mid_smoother=(), post_smoother=(), post_uses_pre=True,
                 mid_case="standalone", max_levels=10, min_coarse_rows=64, coarsest_solver=(), cycle="v",
                 smoother_relax=0.9, smoother_iters=1, default_initial_guess="provided", max_iters=1,
                 reduction=None, baseline="rhs_norm", level_selector=None, solver_selector=None, trace=None):
        assert cycle in CYCLES and mid_case in MID_CASES
        self.matrix, self.cycle, self.mid_case = matrix, cycle, mid_case
        self.max_iters, self.reduction, self.baseline = max_iters, reduction, baseline
        self.default_initial_guess = default_initial_guess
        self.trace = trace
        self.smoother_relax, self.smoother_iters = smoother_relax, smoother_iters
        # validate (:711-748)
        if len(mg_level) == 0 or any(f is None for f in mg_level):
            raise ValueError("mg_level")
        for checked, lst in ((True, pre_smoother), (not post_uses_pre, post_smoother),
                             (mid_case == "standalone", mid_smoother)):
            if checked and len(lst) > 1 and len(lst) != len(mg_level):
                raise ValueError("smoother list length")
        if level_selector is None:
            level_selector = (lambda level, m: 0) if len(mg_level) == 1 else (lambda level, m: level)
        if solver_selector is None:
            solver_selector = lambda level, m: 0
        # generate (:491-574)
        self.mg_level_list, self.pre, self.mid, self.post = [], [], [], []
        self.stopped_by = "max_levels"
        m, level = matrix, 0
        while True:
            if level >= max_levels:
                break
            if not m[0] > min_coarse_rows:
                self.stopped_by = "min_coarse_rows"
                break
            index = level_selector(level, m)
            lvl = mg_level[index](m)
            if lvl.coarse[0] == m[0]:
                self.stopped_by = "no_reduction"
                break
            self._handle_list(index, lvl.fine, pre_smoother, self.pre)
            if mid_case == "standalone":
                self._handle_list(index, lvl.fine, mid_smoother, self.mid)
            if not post_uses_pre:
                self._handle_list(index, lvl.fine, post_smoother, self.post)
            self.mg_level_list.append(lvl)
            m = lvl.coarse
            level += 1
        if post_uses_pre:
            self.post = self.pre
        assert level > 0
        if len(coarsest_solver) == 0:
            self.coarsest, self.coarsest_is_identity = Identity(), True
        else:
            f = coarsest_solver[solver_selector(level, m)]
            self.coarsest, self.coarsest_is_identity = (Identity(), True) if f is None else (f(m), False)

    def _handle_list(self, index, m, factories, out):
        if len(factories) == 0:
            out.append(None)
            return
        f = factories[0 if len(factories) == 1 else index]
        if f is None:
            out.append(None)
            return
        s = f(m)
        out.append(s if s.uses_initial_guess else _Wrapped(m, s, self.smoother_iters, self.smoother_relax))

    def _note(self, what, level):
        if self.trace is not None:
            self.trace.append((what, level))

    def _run(self, cycle, level, m, b, x, x_is_zero, first, end):
        total = len(self.mg_level_list)
        if level == total:
            if not self.coarsest_is_identity:
                self._note("coarsest", level)
            self.coarsest.apply(b, x)
            return
        lvl = self.mg_level_list[level]
        pre, post = self.pre[level], self.post[level]
        mid = self.mid[level] if self.mid_case == "standalone" else None
        if (first or self.mid_case in ("both", "pre_smoother")) and pre is not None:
            self._note("pre", level)
            pre.apply(b, x, zero=x_is_zero)
        r = advanced_spmv(-1.0, m, x, 1.0, b.copy())
        self._note("restrict", level)
        g = spmv(lvl.restrict, r)
        e = self.e[level]
        if level + 1 == total:
            e[:] = 0.0
        nxt = self.mg_level_list[level + 1].fine if level + 1 < total else lvl.coarse
        self._run(cycle, level + 1, nxt, g, e, True, True, cycle == "v")
        if level < total - 1:
            if cycle == "f":
                self._run("v", level + 1, nxt, g, e, False, False, True)
            elif cycle == "w":
                self._run(cycle, level + 1, nxt, g, e, False, False, True)
        self._note("prolong", level)
        x[:] = advanced_spmv(1.0, lvl.prolong, e, 1.0, x)
        if (end or self.mid_case in ("both", "post_smoother")) and post is not None:
            self._note("post", level)
            post.apply(b, x)
        if cycle in ("w", "f") and not end and self.mid_case == "standalone" and mid is not None:
            self._note("mid", level)
            mid.apply(b, x)

    def apply(self, b, x, initial_guess=None):
        """-> (x, iterations, residual norms seen by the criterion); x is updated in place"""
        guess = initial_guess or self.default_initial_guess
        if guess == "zero":
            x[:] = 0.0
        elif guess == "rhs":
            x[:] = b
        self.e = [np.zeros((lvl.coarse[0], b.shape[1])) for lvl in self.mg_level_list]
        seen = []
        base = None
        it = 0
        while True:
            if it >= self.max_iters:
                break
            if self.reduction is not None:
                res = norm2(advanced_spmv(-1.0, self.matrix, x, 1.0, b.copy()))
                if base is None:
                    base = norm2(b) if self.baseline == "rhs_norm" else res
                seen.append((res, base))
                if np.all(res <= self.reduction * base):
                    break
            self._run(self.cycle, 0, self.matrix, b, x, it == 0 and guess == "zero", True, True)
            it += 1
        return x, it, seen


class _Wrapped:
    """build_smoother around a solver that takes no initial guess: Ir with an Iteration criterion, relaxation factor
    and that solver inside (ir.cpp:261-274)"""
    uses_initial_guess = True

    def __init__(self, m, inner, iterations, relax):
        self.m, self.inner, self.iterations, self.relax = m, inner, iterations, relax

    def apply(self, b, x, zero=False):
        if zero:
            x[:] = 0.0
        for it in range(self.iterations):
            r = b if (it == 0 and zero) else advanced_spmv(-1.0, self.m, x, 1.0, b.copy())
            self.inner.apply_advanced(self.relax, r, 1.0, x)
        return x


# ---- the dummy hierarchy of reference/test/solver/multigrid_kernels.cpp --------------------------------------
# operators that only count: a level's coarse matrix has one row less, every smoother, restriction, prolongation and
# (non-Identity) coarsest solve takes the next step number

def cycle_steps(make, rec):
    """the step numbers of a transcribed cycle test, from any Multigrid-like constructor `make(**parameters)` whose
    object has .trace-style notes of ("pre" | "mid" | "post" | "restrict" | "prolong" | "coarsest", level)"""
    trace = []
    individual = rec["factory"] == "individual"
    dummy = lambda m: _Recording()
    level = lambda m: Level(m, csr(m[0] - 1, m[0], np.zeros(m[0]), [], []),
                            csr(m[0] - 1, m[0] - 1, np.zeros(m[0]), [], []), csr(m[0], m[0] - 1, np.zeros(m[0] + 1), [], []))
    n = rec["rows"]
    params = dict(mg_level=[level] * 3, pre_smoother=[None, dummy, dummy], post_uses_pre=not individual,
                  mid_case=rec["mid_case"], max_levels=rec["max_levels"], min_coarse_rows=1, cycle=rec["cycle"],
                  max_iters=1, trace=trace)
    if individual:
        params.update(mid_smoother=[None, None, dummy], post_smoother=[dummy, None, dummy])
    else:
        params.update(coarsest_solver=[dummy])
    mg = make(csr(n, n, np.zeros(n + 1), [], []), **params)
    mg.apply(np.zeros((n, 1)), np.zeros((n, 1)))
    got = steps_of(trace)
    if not individual:
        # post_uses_pre: the post smoother IS the pre smoother, whose list of steps the reference's test reads
        for lvl, steps in got["post"].items():
            got["pre"][lvl] = sorted(got["pre"].get(lvl, []) + steps)
        got["post"] = {}
    return got


def steps_of(trace):
    out = {"levels": {}, "pre": {}, "mid": {}, "post": {}, "coarsest": None}
    for step, (what, level) in enumerate(trace):
        if what in ("restrict", "prolong"):
            out["levels"].setdefault(str(level), {"restrict": [], "prolong": []})[what].append(step)
        elif what == "coarsest":
            out["coarsest"] = (out["coarsest"] or []) + [step]
        else:
            out[what].setdefault(str(level), []).append(step)
    return out


def expected_steps(rec):
    """the lists a transcribed test asserts; it does not assert every list, so compare only those"""
    return {k: rec[k] for k in ("levels", "pre", "mid", "post", "coarsest")}


def steps_match(got, rec):
    want = expected_steps(rec)
    for part in ("pre", "mid", "post"):
        for lvl, steps in want[part].items():
            if got[part].get(lvl, []) != steps:
                return False
    for lvl, both in want["levels"].items():
        if got["levels"].get(lvl) != both:
            return False
    return want["coarsest"] is None or got["coarsest"] == want["coarsest"]


class _Recording:
    uses_initial_guess = True

    def apply(self, b, x, zero=False):
        return x


# ---- cases shared by the driver, the CPU tests and the GPU tests -------------------------------------------

def read_mtx(name):
    kind, nr, nc, rows, cols, vals = matgen.read_mtx(os.path.join(HERE, "golden", name))
    assert kind == "coo" and nr == nc
    rp, ci, v = matgen.coo_to_csr(nr, rows, cols, vals)
    return sort_by_column_index(csr(nr, nc, rp, ci, v))


def unsorted_5x5():
    """GenerateMgLevelOnUnsortedCsrMatrix's matrix (tests/golden/multigrid.json carries it too)"""
    return csr(5, 5, [0, 3, 7, 10, 12, 15], [1, 2, 0, 0, 3, 4, 1, 0, 4, 2, 1, 3, 1, 2, 4],
               [-3, -3, 5, -3, -2, -1, 5, -3, -1, 5, -3, 5, -2, -2, 5])


def shuffled_rows(m, seed=11):
    """the same matrix with the entries of every row in a random order"""
    rng = np.random.default_rng(seed)
    nr, nc, rp, ci, v = m
    ci, v = ci.copy(), v.copy()
    for r in range(nr):
        p = rng.permutation(rp[r + 1] - rp[r])
        ci[rp[r]:rp[r + 1]], v[rp[r]:rp[r + 1]] = ci[rp[r]:rp[r + 1]][p], v[rp[r]:rp[r + 1]][p]
    return nr, nc, rp, ci, v


COARSENING_CASES = {
    "sorted_5x5": lambda: (sort_by_column_index(unsorted_5x5()), [0, 2, 3], False),
    "unsorted_5x5": lambda: (unsorted_5x5(), [0, 2, 3], False),
    "ani1_every_2nd": lambda: (read_mtx("ani1.mtx"), list(range(0, 36, 2)), False),
    "ani4_every_3rd": lambda: (read_mtx("ani4.mtx"), list(range(0, 3081, 3)), False),
    "ani1_shuffled": lambda: (shuffled_rows(read_mtx("ani1.mtx")), list(range(0, 36, 2)), False),
}


def right_hand_side(n, nrhs=1):
    j = np.arange(n, dtype=np.float64)
    return np.stack([np.cos(0.3 * j + 0.7 * c) + 0.25 * np.sin(0.011 * j * (c + 1)) for c in range(nrhs)], axis=1)


def initial_guess(n, nrhs=1):
    j = np.arange(n, dtype=np.float64)
    return np.stack([np.sin(0.17 * j + c) for c in range(nrhs)], axis=1)


# smoother runs: Ir over scalar Jacobi on a matrix
SMOOTHER_CASES = {f"{mat}/s{s}/{'zero' if z else 'guess'}/r{relax}": (mat, s, z, relax)
                  for mat in ("ani1", "ani4") for s in (1, 2, 3) for z in (False, True) for relax in (0.9, 1.0)}


def every_second(m):
    return fixed_coarsening(m, list(range(0, m[0], 2)))


def no_reduction(m):
    return fixed_coarsening(m, list(range(m[0])))


# whole applies.  levels: "halve" = FixedCoarsening on every second row, one factory reused on all levels;
# smoothers: per list entry "jacobi" (a Jacobi factory, wrapped by build_smoother), "eye" (an Identity factory, wrapped
# likewise), None (null entry)
_BASE = dict(matrix="ani4", mg_level=["halve"], pre=["jacobi"], mid=[], post=[], post_uses_pre=True,
             mid_case="standalone", max_levels=2, min_coarse_rows=64, coarsest="direct", cycle="v", relax=0.9, iters=2,
             guess="zero", max_iters=3, reduction=None)


def _case(**kw):
    c = dict(_BASE)
    c.update(kw)
    return c


SOLVE_CASES = {}
for _mat in ("ani4", "1138_bus"):
    for _cy in CYCLES:
        SOLVE_CASES[f"{_mat}/{_cy}/direct"] = _case(matrix=_mat, cycle=_cy)
        # a solver that takes an initial guess in the coarsest slot: Cg, ten iterations
        SOLVE_CASES[f"{_mat}/{_cy}/cg"] = _case(matrix=_mat, cycle=_cy, coarsest="cg")
for _mid in MID_CASES:
    SOLVE_CASES[f"ani4/w/mid_{_mid}"] = _case(cycle="w", mid_case=_mid, mid=["jacobi"], coarsest="identity",
                                              guess="provided")
SOLVE_CASES.update({
    "ani4/f/post_not_pre": _case(cycle="f", post_uses_pre=False, post=["jacobi"], pre=["jacobi"], iters=1),
    "ani4/w/null_entries": _case(cycle="w", mg_level=["halve", "halve"], pre=[None, "jacobi"], iters=1,
                                 coarsest="identity"),
    "ani1/v/min_coarse_rows": _case(matrix="ani1", max_levels=10, min_coarse_rows=10, coarsest="direct"),
    "ani1/v/no_reduction": _case(matrix="ani1", mg_level=["halve", "all_rows"], max_levels=10, min_coarse_rows=1),
    # a smoother without an initial guess that is no Jacobi: build_smoother's Ir around matrix::Identity
    "ani1/w/identity_smoother": _case(matrix="ani1", cycle="w", pre=["eye"], max_levels=10, min_coarse_rows=8,
                                      guess="provided"),
    "ani4/v/residual_norm": _case(max_iters=200, reduction=0.3),
    "ani4/w/residual_norm": _case(cycle="w", max_iters=200, reduction=0.3, guess="provided"),
    "1138_bus/f/residual_norm": _case(matrix="1138_bus", cycle="f", max_iters=300, reduction=0.5),
})


def case_matrix(name):
    return read_mtx(name + ".mtx")


def restated(case, trace=None, make=None, parts=None, matrix=None):
    """(x, iterations, criterion's norms, the Multigrid) of a whole-apply case through `make` (default: the
    restatement).  parts: {"halve", "all_rows", "jacobi", "direct", "identity"} -> factories for another layer."""
    c = SOLVE_CASES[case] if isinstance(case, str) else case
    m = matrix if matrix is not None else case_matrix(c["matrix"])
    parts = parts or {"halve": every_second, "all_rows": no_reduction, "jacobi": lambda mm: _PlainJacobi(mm),
                      "eye": Identity, "direct": Direct, "cg": Cg, "identity": None}
    pick = lambda names: [None if t is None else parts[t] for t in names]
    coarsest = [] if c["coarsest"] == "identity" else [parts[c["coarsest"]]]
    mg = (make or Multigrid)(m, mg_level=pick(c["mg_level"]), pre_smoother=pick(c["pre"]), mid_smoother=pick(c["mid"]),
                             post_smoother=pick(c["post"]), post_uses_pre=c["post_uses_pre"], mid_case=c["mid_case"],
                             max_levels=c["max_levels"], min_coarse_rows=c["min_coarse_rows"], coarsest_solver=coarsest,
                             cycle=c["cycle"], smoother_relax=c["relax"], smoother_iters=c["iters"],
                             default_initial_guess=c["guess"], max_iters=c["max_iters"], reduction=c["reduction"],
                             trace=trace)
    b = right_hand_side(m[0])
    x = initial_guess(m[0])
    return mg, b, x


class _PlainJacobi:
    """preconditioner::Jacobi with max_block_size 1: x = b inv_diag, no initial guess (so Multigrid wraps it)"""
    uses_initial_guess = False

    def __init__(self, m):
        self.inv = inverted_diagonal(m)

    def apply(self, b, x, zero=False):
        x[:] = b * self.inv[:, None]
        return x

    def apply_advanced(self, alpha, b, beta, x):
        """jacobi::scalar_apply (reference/preconditioner/jacobi_kernels.cpp:565-580)"""
        with np.errstate(all="ignore"):
            x[:] = np.float64(beta) * x + (np.float64(alpha) * b) * self.inv[:, None]
        return x


# ---- the cases as ref_driver's verb multigrid takes them; as text for the mirror's examples ----------------

def _ints(a):
    return " ".join(str(int(t)) for t in a)


def _hex(a):
    return " ".join(float(t).hex() for t in np.asarray(a, np.float64).reshape(-1))


def _matrix_text(m):
    return f"{m[0]} {len(m[3])} {_ints(m[2])} {_ints(m[3])} {_hex(m[4])}"


KCYCLE_CASES = {"n5_3rhs": (5, 3), "n65_17rhs": (65, 17), "n0_1rhs": (0, 1)}


def kcycle_operands(n, nrhs):
    """scalars with the special columns the kernels guard: column 0 rho = 0, column 1 NaN alpha, column 2 (step 2)
    beta - gamma^2 / rho = 0"""
    j = np.arange(nrhs, dtype=np.float64)
    alpha, rho = 1.5 + 0.25 * j, 2.0 + 0.5 * j
    gamma, beta, zeta = 0.5 + 0.125 * j, 3.0 + j, 0.75 - 0.0625 * j
    rho[0] = 0.0
    if nrhs > 1:
        alpha[1] = np.nan
    if nrhs > 2:
        gamma[2], rho[2], beta[2] = 2.0, 4.0, 1.0
    grid = np.arange(n * nrhs, dtype=np.float64).reshape(n, nrhs)
    v, g, d, e = np.cos(0.1 * grid), np.sin(0.2 * grid) + 2.0, np.full((n, nrhs), 7.0), np.cos(0.3 * grid) - 0.5
    return alpha, rho, gamma, beta, zeta, v, g, d, e


def _dense(arrays, params, **named):
    for name, a in named.items():
        arr, shape = ref_exec.dense_arrays(name, a)
        arrays.update(arr)
        params.update(shape)


def solve_arguments(c, m):
    """the arrays and parameters of a whole-apply case on the matrix m, as multigrid_solve of oracle/ref_driver.cpp
    reads them (the solve op of the verbs multigrid and pgm)"""
    word, words = ref_exec.word, ref_exec.words
    arrays, params = ref_exec.csr_arrays(*m)
    _dense(arrays, params, b=right_hand_side(m[0]), x=initial_guess(m[0]))
    arrays.update(mg_level=words("mg_level", c["mg_level"]), pre=words("smoother", c["pre"]),
                  mid=words("smoother", c["mid"]), post=words("smoother", c["post"]))
    params.update(cycle=word("cycle", c["cycle"]), mid_case=word("mid_case", c["mid_case"]),
                  post_uses_pre=c["post_uses_pre"], max_levels=c["max_levels"], min_coarse_rows=c["min_coarse_rows"],
                  coarsest=word("coarsest", c["coarsest"]), relax=c["relax"], smoother_iters=c["iters"],
                  guess=word("guess", c["guess"]), max_iters=c["max_iters"], reduction=c["reduction"] or 0.0)
    return arrays, params


def queue_cases(batch):
    """queues every case on a ref_exec.Batch -> {name: index of its result}"""
    where = {}
    for name, (n, nrhs) in KCYCLE_CASES.items():
        alpha, rho, gamma, beta, zeta, v, g, d, e = kcycle_operands(n, nrhs)
        row = lambda t: t.reshape(1, nrhs)
        arrays, params = {}, {}
        _dense(arrays, params, alpha=row(alpha), rho=row(rho), gamma=row(gamma), beta=row(beta), zeta=row(zeta),
               v=v, g=g, d=d, e=e)
        where[name] = batch.add("multigrid", arrays, op=0, **params)
    for name, make in COARSENING_CASES.items():
        m, rows, skip = make()
        arrays, params = ref_exec.csr_arrays(*m)
        arrays["coarse_rows"] = np.asarray(rows, np.int32)
        where[name] = batch.add("multigrid", arrays, op=1, skip_sorting=skip, **params)
    for name, (mat, sweeps, zero, relax) in SMOOTHER_CASES.items():
        m = case_matrix(mat)
        arrays, params = ref_exec.csr_arrays(*m)
        _dense(arrays, params, b=right_hand_side(m[0]), x=initial_guess(m[0]))
        where[name] = batch.add("multigrid", arrays, op=2, sweeps=sweeps, zero_guess=zero, relax=relax, **params)
    for name, c in SOLVE_CASES.items():
        arrays, params = solve_arguments(c, case_matrix(c["matrix"]))
        where[name] = batch.add("multigrid", arrays, op=3, **params)
    return where


def case_arrays(results, where):
    return {name: results[i] for name, i in where.items()}


def fixture_from(records, verb="multigrid"):
    """the committed fixture from the driver's arrays: short arrays in full, long ones as count + digest"""
    fix = {"source": f"oracle/ref_driver.cpp, verb {verb}, over the reference executor; cases: tests/{verb}_util.py"}
    for name, arrays in records.items():
        fix[name] = {what: ref_exec.as_record(a) for what, a in arrays.items()}
    return fix


def dump_fixture(fix, path):
    import json
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v) for k, v in fix.items()) + "\n}\n")


def _csr_records(out, what, m):
    out[what + "/row_ptrs"], out[what + "/col_idxs"], out[what + "/vals"] = m[2], m[3], m[4]


def restated_kcycle(name):
    n, nrhs = KCYCLE_CASES[name]
    alpha, rho, gamma, beta, zeta, v, g, d, e = kcycle_operands(n, nrhs)
    d2, e2 = d.copy(), e.copy()
    kcycle_step_1(alpha, rho, v, g, d, e)
    kcycle_step_2(alpha, rho, gamma, beta, zeta, d2, e2)
    fresh = 0.25 * beta
    equal = kcycle_check_stop(beta, fresh, 0.25)
    fresh[-1] = np.nextafter(fresh[-1], 1e300)
    return {"step_1/g": g, "step_1/d": d, "step_1/e": e, "step_2/e": e2,
            "check_stop/is_stop": [int(equal), int(kcycle_check_stop(beta, fresh, 0.25))]}


def restated_coarsening(name):
    m, rows, skip = COARSENING_CASES[name]()
    lvl = fixed_coarsening(m, rows, skip)
    out = {}
    for what in ("fine", "restrict", "prolong", "coarse"):
        _csr_records(out, what, getattr(lvl, what))
    return out


def restated_smoother(name):
    mat, sweeps, zero, relax = SMOOTHER_CASES[name]
    m = case_matrix(mat)
    return {"x": jacobi_sweeps(m, inverted_diagonal(m), relax, right_hand_side(m[0]), initial_guess(m[0]), sweeps, zero)}


def restated_solve(name):
    mg, b, x = restated(name)
    x, it, _ = mg.apply(b, x)
    return {"x": x, "iterations": [it], "levels": [lvl.coarse[0] for lvl in mg.mg_level_list]}


def restated_records():
    """everything the driver returns, from the restatement: {case: {what: array}}"""
    out = {}
    for cases, fn in ((KCYCLE_CASES, restated_kcycle), (COARSENING_CASES, restated_coarsening),
                      (SMOOTHER_CASES, restated_smoother), (SOLVE_CASES, restated_solve)):
        for name in cases:
            out[name] = fn(name)
    return out


INTEGER_RECORDS = ("row_ptrs", "col_idxs", "iterations", "levels", "is_stop")


def record_matches(rec, what, got):
    return ref_exec.matches(rec, got, integers=what.endswith(INTEGER_RECORDS))


V_CYCLE_PRECONDITIONER = _case(matrix=None, max_iters=1, guess="zero")


def dot(a, b):
    """dense::compute_dot of the reference: the products added in row order"""
    acc = np.zeros(a.shape[1])
    for ra, rb in zip(a, b):
        acc = acc + ra * rb
    return acc


def preconditioned_cg(m, b, max_iters, reduction):
    """solver::Cg (core/solver/cg.cpp) on one right-hand side from x = 0, preconditioned by one V-cycle of the
    three-level hierarchy of the "direct" cases with a zero initial guess; ResidualNorm(reduction, rhs_norm).
    -> (x, iterations)"""
    mg, _, _ = restated(V_CYCLE_PRECONDITIONER, matrix=m)
    x = np.zeros_like(b)
    r = b.copy()
    z, p, q = np.zeros_like(b), np.zeros_like(b), np.zeros_like(b)
    prev_rho = np.ones(1)
    goal = reduction * norm2(b)
    it = 0
    while True:
        mg.apply(r, z)
        rho = dot(r, z)
        if it >= max_iters or np.all(norm2(r) <= goal):
            return x, it
        p = z + (rho / prev_rho) * p if it > 0 else z.copy()
        q = spmv(m, p)
        alpha = rho / dot(p, q)
        x = x + alpha * p
        r = r - alpha * q
        prev_rho = rho
        it += 1
