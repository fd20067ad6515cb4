"""The certificate of tests/exact_systems.py: every kept (solver, case) pair gives the same iterations, the same x as
bits and the same residual norm under three orderings of the unknowns, at the small size and at the size the device
tests use.  That is what entitles test_whole_solves_exact_gpu.py and the exact cases of
test_ref_oracle_parity_solvers.py to bit equality with drivers that sum in another order."""
import numpy as np
import pytest

import exact_systems as xs

# what the oracle gives on each case, per solver: iterations, recorded when the cases were designed.  A cell that is
# missing here is a pair that failed the certificate and is not kept.
ITERATIONS = {
    "Z0": dict(cg=17, fcg=17, bicgstab=17, cgs=17, bicg=17, gmres=17, ir=17),
    "Z1": dict(cg=17, fcg=17, bicgstab=17, cgs=17, bicg=17, ir=17),
    "Zabs": dict(cg=0, fcg=0, bicgstab=0, cgs=0, bicg=0, gmres=0, ir=0),
    "E": dict(cg=0, fcg=0, bicgstab=0, cgs=0, bicg=0, gmres=0, ir=0),
    "O": dict(cg=1, fcg=1, bicgstab=0, cgs=1, bicg=1, ir=1),           # gmres: fails the certificate, see KEPT
    "O16": dict(cg=1, fcg=1, bicgstab=0, cgs=1, bicg=1, gmres=1, ir=1),
    "K": dict(cg=17, bicgstab=17, bicg=17, ir=17),
    # gmres on N and Nodd: not kept, see KEPT (the permutations are blind to a regrouped sum of equal entries, and the
    # device's regrouped sums do differ); N2 is N at n = 256 and 16384, where |b| is a power of two
    "N": dict(cg=17, fcg=17, bicgstab=17, bicg=17, ir=17),
    "Nodd": dict(cg=2, fcg=2, cgs=2, bicg=2, ir=17),
    "N2": dict(cg=17, fcg=17, bicgstab=17, bicg=17, gmres=2, ir=17),
    "H": dict(cg=17, fcg=17, bicgstab=17, cgs=17, bicg=17, gmres=17, ir=17),
    "Mc": dict(cg=1, fcg=1, bicgstab=0, cgs=1, bicg=1, ir=1),
    "Ms": dict(cg=17, bicgstab=17, bicg=17, ir=17),
}


def test_every_cell_of_the_table_is_kept():
    for case, cells in ITERATIONS.items():
        assert set(cells) <= set(xs.KEPT[case]), (case, set(cells) - set(xs.KEPT[case]))


def test_the_pairs_without_a_residual_norm_are_the_ones_that_need_it(oracle):
    """X_ONLY is no wider than it has to be: each of its pairs has a residual whose squares do not add up exactly"""
    for solver, case in xs.X_ONLY:
        assert solver in xs.KEPT[case]
        c = xs.CASES[case]
        inexact = []
        for n in c.sizes():
            A, b, x0 = c.build(n)
            _, x, res = xs.solve(oracle, solver, A, b, x0, c.baseline, c.max_iters, c.krylov_dim)
            assert res is None
            inexact.append(not xs.exact_norm2(xs.residual(A, b, x)))
        assert any(inexact), (solver, case)


@pytest.mark.parametrize("names", xs.column_sets("gmres"), ids="-".join)
@pytest.mark.parametrize("n", [xs.SMALL, xs.LARGE])
def test_gmres_columns_order_independent(oracle, names, n):
    """the multi-column restatement of Gmres under the same three orderings"""
    it, x, res = xs.solve_columns(oracle, "gmres", names, n)
    for perm in (np.arange(n)[::-1].copy(), np.random.default_rng(n).permutation(n)):
        it2, x2, res2 = xs.solve_columns(oracle, "gmres", names, n, perm)
        assert it2 == it and xs.same_bits(x2, x) and xs.same_bits(res2, res)
    # a column alone is ref_gmres_solve; the column that converged first gets its correction again at every restart
    for j, c in enumerate(names):
        _, xj, _ = xs.run(oracle, "gmres", c, n)
        updates = 1 + (it - 1) // 5 if (it > 5 and xs.run(oracle, "gmres", c, n)[0] in (0, 1)) else 1
        x0 = xs.CASES[c].build(n)[2]
        assert xs.same_bits(x[:, j].copy(), x0 + updates * (xj - x0)), (c, updates)


def _sizes():
    return [(s, c, n) for s, c in xs.pairs() for n in xs.CASES[c].sizes()]


@pytest.mark.parametrize("solver,case,n", _sizes(), ids=lambda v: str(v).replace(":", "_"))
def test_order_independent(oracle, solver, case, n):
    ok, first = xs.order_independent(oracle, solver, case, n)
    assert ok, first
    it, x, res = first
    want = ITERATIONS.get(case, {}).get(solver)
    if want is not None:
        assert it == want, f"{solver} on {case}: {it} iterations, the table says {want}"
    # what is known about x
    A, b, x0 = xs.CASES[case].build(n)
    if (case, solver) in {("Z0", "gmres"), ("Z0", "idr")}:
        # Gmres normalises by a zero norm; Idr divides by m_kk = p_k . g_k = 0 (idr_kernels.cpp step_3)
        assert np.isnan(x).all()
    elif (case, solver) == ("Zm", "gmres"):
        assert np.isnan(x).all()
    elif case in ("Z0", "Zabs", "Zm") or (case == "H" and solver in ("gmres", "cb_gmres:keep", "cb_gmres:reduce1")):
        assert not x.any()
    elif case in ("O", "O16") and solver != "ir":
        assert xs.same_bits(x.astype(np.float64), b / 2)
    elif case == "E" or (case in ("K", "Ms") and solver in ("cg", "bicgstab", "bicg", "cg_f32")) or \
            (case == "N" and solver in ("cg", "cg_f32")):
        assert xs.same_bits(x.astype(np.float64), x0)
    if case == "H" and solver == "gmres":
        assert res == 1.0
    if case == "O16" and solver == "gmres":
        assert res == 0.0
    if case in ("H8k8", "H8k10"):
        assert it == 8 and xs.same_bits(x, np.eye(1, 8, 1)[0])
    if case == "H301k400":
        assert it == 301
