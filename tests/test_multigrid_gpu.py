"""solver::Multigrid on the device: the kcycle kernels, the fused Jacobi sweep, FixedCoarsening and whole Multigrid
applies of the Python layer against the numpy restatement (tests/multigrid_util.py) and the reference executor's
recorded results (tests/golden/multigrid_ref.json), compared as integers -- a NaN matches a NaN."""
import json
import os

import numpy as np
import pytest
import torch

import gkomi
import matgen
import multigrid_util as mu
from gkomi import formats, solvers
from gpu_util import dev, host, make_srow, stream_ptr, sync

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REF = json.load(open(os.path.join(HERE, "golden", "multigrid_ref.json")))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "multigrid.json")))
SPLIT = 4


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def padded(a, pad, fill=-77.0):
    """a device copy of the n x nrhs array inside rows of nrhs + pad entries; -> (view, whole buffer)"""
    n, nrhs = a.shape
    buf = torch.full((max(n, 1), nrhs + pad), fill, dtype=torch.float64, device="cuda:0")
    view = buf[:n, :nrhs]
    view.copy_(dev(a))
    return view, buf


# ---- kcycle kernels --------------------------------------------------------------------------------------

@pytest.mark.parametrize("nrhs", [1, 3, 17])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1000])
def test_kcycle_steps(gk, n, nrhs):
    alpha, rho, gamma, beta, zeta, v, g, d, e = mu.kcycle_operands(n, nrhs)
    want = [t.copy() for t in (g, d, e)]
    mu.kcycle_step_1(alpha, rho, v, *want)
    dv_, _ = padded(v, 2)
    (dg, bg), (dd, bd), (de, be) = padded(g, 1), padded(d, 3), padded(e, 5)
    gk.multigrid_kcycle_step_1_f64(stream_ptr(), n, nrhs, dev(alpha), dev(rho), dv_, dv_.stride(0), dg, dg.stride(0), dd,
                                   dd.stride(0), de, de.stride(0))
    sync()
    for got, exp, start, buf, pad in ((dg, want[0], g, bg, 1), (dd, want[1], d, bd, 3), (de, want[2], e, be, 5)):
        assert same_bits(host(got), exp)
        assert n == 0 or np.all(host(buf)[:, nrhs:] == -77.0)      # the padding is not written
    # rho = 0 in column 0 and a NaN alpha in column 1: g and e untouched, d = e still written
    for col in range(min(nrhs, 2)):
        assert same_bits(host(dg)[:, col], g[:, col]) and same_bits(host(de)[:, col], e[:, col])
        assert same_bits(host(dd)[:, col], e[:, col])

    want_e = e.copy()
    mu.kcycle_step_2(alpha, rho, gamma, beta, zeta, d, want_e)
    (dd, _), (de, be) = padded(d, 2), padded(e, 4)
    gk.multigrid_kcycle_step_2_f64(stream_ptr(), n, nrhs, dev(alpha), dev(rho), dev(gamma), dev(beta), dev(zeta), dd,
                                   dd.stride(0), de, de.stride(0))
    sync()
    assert same_bits(host(de), want_e)
    assert n == 0 or np.all(host(be)[:, nrhs:] == -77.0)
    for col in range(min(nrhs, 3)):      # rho = 0, NaN alpha, beta - gamma^2 / rho = 0: e untouched
        assert same_bits(host(de)[:, col], e[:, col])
    if n > 0 and nrhs > 3:
        assert not same_bits(host(de)[:, 3], e[:, 3])


def test_kcycle_steps_match_the_reference_executor(gk):
    for name, (n, nrhs) in mu.KCYCLE_CASES.items():
        alpha, rho, gamma, beta, zeta, v, g, d, e = mu.kcycle_operands(n, nrhs)
        dg, dd, de = dev(g), dev(d), dev(e)
        gk.multigrid_kcycle_step_1_f64(stream_ptr(), n, nrhs, dev(alpha), dev(rho), dev(v), nrhs, dg, nrhs, dd, nrhs, de, nrhs)
        d2, e2 = dev(d), dev(e)
        gk.multigrid_kcycle_step_2_f64(stream_ptr(), n, nrhs, dev(alpha), dev(rho), dev(gamma), dev(beta), dev(zeta), d2,
                                       nrhs, e2, nrhs)
        sync()
        for what, got in (("step_1/g", dg), ("step_1/d", dd), ("step_1/e", de), ("step_2/e", e2)):
            assert mu.record_matches(REF[name][what], what, host(got)), (name, what)


@pytest.mark.parametrize("nrhs", [1, 3])
def test_kcycle_check_stop(gk, nrhs):
    old = 1.0 + np.arange(nrhs, dtype=np.float64) / 3.0
    flag = torch.full((4,), 9, dtype=torch.uint8, device="cuda:0")

    def stop(new, rel_tol=0.25):
        gk.multigrid_kcycle_check_stop_f64(stream_ptr(), nrhs, dev(old), dev(new), rel_tol, flag)
        sync()
        got = host(flag)
        assert list(got[1:]) == [9, 9, 9]
        assert bool(got[0]) == mu.kcycle_check_stop(old, new, rel_tol)
        return bool(got[0])

    assert stop(0.25 * old)                       # new == rel_tol old: `>` does not hold
    above = 0.25 * old
    above[-1] = np.nextafter(above[-1], np.inf)
    assert not stop(above)
    below = 0.25 * old
    below[0] = np.nextafter(below[0], 0.0)
    assert stop(below)
    nan = 0.25 * old
    nan[0] = np.nan
    assert stop(nan)                              # a NaN compares false
    for name, (n, cols) in mu.KCYCLE_CASES.items():
        assert REF[name]["check_stop/is_stop"] == [1, 0]


# ---- the fused sweep -----------------------------------------------------------------------------------------

def banded(n, seed, extra=2):
    """diagonally dominant rows: the diagonal, both neighbours and `extra` random columns, sorted"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        cols = sorted({i, max(i - 1, 0), min(i + 1, n - 1), *rng.integers(0, n, extra).tolist()})
        vals = [4.0 + rng.random() if c == i else -rng.random() for c in cols]
        rows.append((cols, vals))
    return rows


def from_rows(n, rows):
    rp = np.cumsum([0] + [len(c) for c, _ in rows])
    ci = np.array([c for cols, _ in rows for c in cols], np.int32)
    v = np.array([x for _, vals in rows for x in vals], np.float64)
    return mu.csr(n, n, rp, ci, v)


def sweep_matrices():
    out = {"empty": from_rows(0, []), "n1": from_rows(1, [([0], [2.5])])}
    for n in (63, 64, 65, 257):
        out[f"n{n}"] = from_rows(n, banded(n, n))
    rows = banded(65, 1)
    rows[7] = ([], [])                                      # a row with no stored entry
    rows[9] = ([3, 20], [0.5, -0.25])                       # a row without a stored diagonal
    rows[11] = ([40, 11, 2, 40, 12], [-0.5, 3.0, 0.25, -0.125, 1.0])   # unsorted, column 40 twice
    rows[13] = ([12, 13, 14], [-0.0, 5.0, -0.0])            # stored -0.0
    out["odd_rows"] = from_rows(65, rows)
    rng = np.random.default_rng(5)
    rows = banded(2049, 2)
    for row, count in ((100, 70), (1500, 1100)):            # more than a wave and more than 1024 nonzeros
        cols = rng.permutation(2049)[:count].tolist() + [row]
        rows[row] = (cols, [(400.0 if c == row else -rng.random()) for c in cols])
    out["long_rows"] = from_rows(2049, rows)
    return out


SWEEP_MATRICES = sweep_matrices()


def three_calls(gk, m, inv, relax, b, x, sweeps, zero):
    """the same sweeps through the existing entry points: copy, advanced SpMV (split strategy), scalar_apply"""
    n = m[0]
    A = formats.Csr.from_host(gk, n, n, m[2], m[3], m[4], strategy=SPLIT)
    s = stream_ptr()
    one, neg_one, rel = (dev(np.array([t])) for t in (1.0, -1.0, relax))
    r = torch.zeros_like(b)
    if zero:
        gk.dense_fill_f64(s, n, 1, x, 1, 0.0)
    for it in range(sweeps):
        src = b
        if not (it == 0 and zero):
            gk.dense_copy_f64(s, n, 1, b, 1, r, 1)
            if A.nnz >= 2:
                srow, tile = make_srow(gk, A, int(gk.csr_srow_tile_for(A.nnz)))
                gk.csr_spmv_srow_f64_i32(s, n, n, 1, A.nnz, A.row_ptrs, A.col_idxs, A.vals, x, 1, r, 1, neg_one, one, SPLIT,
                                         A.max_row_nnz(), srow, tile)
            else:
                gk.csr_spmv_f64_i32(s, n, n, 1, A.nnz, A.row_ptrs, A.col_idxs, A.vals, x, 1, r, 1, neg_one, one, 1, -1)
            src = r
        gk.jacobi_scalar_apply_f64(s, n, 1, inv, rel, src, 1, one, x, 1)
    return x


@pytest.mark.parametrize("name", list(SWEEP_MATRICES))
def test_fused_sweep(gk, name):
    m = SWEEP_MATRICES[name]
    n = m[0]
    b, x0 = mu.right_hand_side(n), mu.initial_guess(n)
    invs = {"library": None}
    if name == "odd_rows":
        inf = mu.inverted_diagonal(m)
        inf[9] = np.inf                                     # an infinite inverse where no diagonal is stored
        invs["infinite"] = inf
    rp, ci, v = dev(m[2]), dev(m[3]), dev(m[4])
    for which, inv in invs.items():
        if inv is None:
            diag = torch.zeros(max(n, 1), dtype=torch.float64, device="cuda:0")[:n]
            dinv = torch.zeros_like(diag)
            gk.csr_extract_diagonal_f64_i32(stream_ptr(), n, rp, ci, v, diag)
            gk.jacobi_invert_diagonal_f64(stream_ptr(), n, diag, dinv)
            sync()
            inv = host(dinv).copy()
            assert same_bits(inv, mu.inverted_diagonal(m))
        dinv = dev(inv)
        nb = int(gk.multigrid_jacobi_sweeps_workspace_bytes(n))
        ws = torch.zeros(max(nb, 8), dtype=torch.uint8, device="cuda:0")
        for sweeps in (1, 2, 3):
            for zero in (False, True):
                for relax in (0.9, 1.0):
                    want = mu.jacobi_sweeps(m, inv, relax, b, x0, sweeps, zero)
                    db, dx = dev(b), dev(x0)
                    gk.multigrid_jacobi_sweeps_f64_i32(stream_ptr(), n, 1, len(m[3]), rp, ci, v, dinv, relax, db, dx, sweeps,
                                                       int(zero), ws, nb)
                    twin = three_calls(gk, m, dinv, relax, dev(b), dev(x0), sweeps, zero)
                    sync()
                    what = (name, which, sweeps, zero, relax)
                    assert same_bits(host(dx), want), what
                    assert same_bits(host(twin), want), what
                    assert same_bits(host(db), b), what


def test_fused_sweep_matches_the_reference_executor(gk):
    for name, (mat, sweeps, zero, relax) in mu.SMOOTHER_CASES.items():
        m = mu.case_matrix(mat)
        A = formats.Csr.from_host(gk, m[0], m[0], m[2], m[3], m[4], strategy=SPLIT)
        x = dev(mu.initial_guess(m[0]))
        solvers.JacobiSmoother(gk, A, sweeps, relax, fused=True).apply(dev(mu.right_hand_side(m[0])), x, zero=zero)
        sync()
        assert mu.record_matches(REF[name]["x"], "x", host(x)), name


def test_fused_sweep_zero_sweeps(gk):
    m = SWEEP_MATRICES["n65"]
    rp, ci, v, inv = dev(m[2]), dev(m[3]), dev(m[4]), dev(mu.inverted_diagonal(m))
    nb = int(gk.multigrid_jacobi_sweeps_workspace_bytes(65))
    ws = torch.zeros(nb, dtype=torch.uint8, device="cuda:0")
    x0 = mu.initial_guess(65)
    for zero in (0, 1):
        x = dev(x0)
        gk.multigrid_jacobi_sweeps_f64_i32(stream_ptr(), 65, 1, len(m[3]), rp, ci, v, inv, 0.9, dev(x0), x, 0, zero, ws, nb)
        sync()
        assert same_bits(host(x), np.zeros_like(x0) if zero else x0)


def test_fused_sweep_rejects_bad_arguments_before_a_launch(gk):
    vec = torch.zeros(256, dtype=torch.float64, device="cuda:0")
    b, x, ws = vec[:64], vec[64:128], vec[128:256]
    idx = torch.zeros(80, dtype=torch.int32, device="cuda:0")
    vals = torch.zeros(80, dtype=torch.float64, device="cuda:0")
    need = int(gk.multigrid_jacobi_sweeps_workspace_bytes(64))
    assert need >= 64 * 8 and gk.multigrid_jacobi_sweeps_workspace_bytes(0) == 0

    def code(n=64, nrhs=1, nnz=10, sweeps=1, work=ws, nbytes=need, bb=b, xx=x):
        try:
            return gk.multigrid_jacobi_sweeps_f64_i32(None, n, nrhs, nnz, idx, idx, vals, vals, 0.9, bb, xx, sweeps, 0, work,
                                                      nbytes)
        except gkomi.GkomiError as e:
            return e.code

    assert code(nrhs=2) == -1 and code(nrhs=0) == -1
    assert code(n=-1) == -1 and code(nnz=-1) == -1 and code(sweeps=-1) == -1
    assert code(work=None) == -1 and code(nbytes=need - 8) == -1
    assert code(work=x) == -1 and code(work=b) == -1                  # the workspace is x or b
    assert code(work=vec[100:], nbytes=need) == -1                    # ... or overlaps the tail of x
    assert code(work=vec[32:], nbytes=need) == -1                     # ... or the tail of b
    assert code(n=0) == 0


# ---- FixedCoarsening -------------------------------------------------------------------------------------------

def device_level(gk, m, rows, skip_sorting=False):
    return solvers.fixed_coarsening(gk, m[0], dev(m[2]), dev(m[3]), dev(m[4]), rows, skip_sorting, strategy=SPLIT)


def op_arrays(op):
    return {"row_ptrs": host(op.row_ptrs), "col_idxs": host(op.col_idxs), "vals": host(op.vals)}


@pytest.mark.parametrize("name", list(mu.COARSENING_CASES))
def test_fixed_coarsening_matches_the_reference_executor(gk, name):
    m, rows, skip = mu.COARSENING_CASES[name]()
    lvl = device_level(gk, m, rows, skip)
    sync()
    for what, op in (("fine", lvl.get_fine_op()), ("restrict", lvl.get_restrict_op()), ("prolong", lvl.get_prolong_op()),
                     ("coarse", lvl.get_coarse_op())):
        for part, got in op_arrays(op).items():
            key = f"{what}/{part}"
            assert mu.record_matches(REF[name][key], key, got), (name, key)
    assert (lvl.get_restrict_op().nrows, lvl.get_restrict_op().ncols) == (len(rows), m[0])
    assert (lvl.get_prolong_op().nrows, lvl.get_prolong_op().ncols) == (m[0], len(rows))
    assert (lvl.get_coarse_op().nrows, lvl.get_coarse_op().ncols) == (len(rows), len(rows))


def dense_of(op):
    a = np.zeros((op.nrows, op.ncols))
    rp, ci, v = host(op.row_ptrs), host(op.col_idxs), host(op.vals)
    for r in range(op.nrows):
        for k in range(rp[r], rp[r + 1]):
            a[r, ci[k]] += v[k]
    return a


def test_fixed_coarsening_known_answers(gk):
    fc = GOLDEN["fixed_coarsening"]
    tol = fc["precision"]
    near = lambda got, want: np.allclose(got, np.array(want, np.float64), rtol=tol, atol=0.0)
    fine = np.array(fc["fine_dense"], np.float64)
    sorted_m = mu.csr(5, 5, *matgen.dense_to_csr(fine)[-3:])
    u = fc["unsorted_csr"]
    coo = fc["unsorted_coo"]
    from_coo = formats.Csr.from_triplets(gk, 5, 5, dev(np.array(coo["row_idxs"], np.int32)),
                                         dev(np.array(coo["col_idxs"], np.int32)), dev(np.array(coo["vals"], np.float64)),
                                         sum_duplicates=False)
    levels = [device_level(gk, sorted_m, fc["coarse_rows"]),
              device_level(gk, mu.csr(5, 5, u["row_ptrs"], u["col_idxs"], u["vals"]), fc["coarse_rows"]),
              solvers.fixed_coarsening(gk, 5, from_coo.row_ptrs, from_coo.col_idxs, from_coo.vals, fc["coarse_rows"])]
    prolong = np.zeros((5, 3))
    for r, c, val in fc["prolong_entries"]:
        prolong[r, c] = val
    for lvl in levels:
        assert near(dense_of(lvl.get_coarse_op()), fc["coarse_dense"])
        assert near(dense_of(lvl.get_prolong_op()), prolong) and near(dense_of(lvl.get_restrict_op()), prolong.T)
        assert near(dense_of(lvl.get_fine_op()), fine)
    lvl = levels[0]
    x = torch.zeros((3, 2), dtype=torch.float64, device="cuda:0")
    lvl.get_restrict_op().apply(dev(np.array(fc["fine_b"], np.float64)), x)
    assert near(host(x), fc["CoarseFineRestrictApply"]["answer"])
    x = dev(np.array(fc["fine_x"], np.float64))
    lvl.get_prolong_op().apply(dev(np.array(fc["coarse_b"], np.float64)), x)
    assert near(host(x), fc["CoarseFineProlongApply"]["answer"])
    b, x = dev(np.array(fc["fine_x"], np.float64)), dev(np.array(fc["fine_x"], np.float64))
    lvl.apply(b, x)                                         # the level as a LinOp: prolong(coarse(restrict(b)))
    assert near(host(x), fc["Apply"]["answer"])
    x = dev(np.array(fc["fine_x"], np.float64))
    lvl.apply(b, x, fc["AdvancedApply"]["alpha"], fc["AdvancedApply"]["beta"])
    assert near(host(x), fc["AdvancedApply"]["answer"])


# ---- Multigrid, Python layer ---------------------------------------------------------------------------------

class Counting:
    """the dummy operator of the reference's cycle tests: takes a step number, computes nothing"""
    uses_initial_guess = True

    def apply(self, b, x):
        return x


def device_multigrid_for_steps(gk, tweak=None):
    """a constructor with the restatement's signature for mu.cycle_steps: dummy levels whose operators have no entry;
    tweak(multigrid) runs before the apply"""
    def make(m, mg_level, **params):
        def level(a):
            n = a.nrows
            empty = lambda r, c: formats.Csr.from_host(gk, r, c, np.zeros(r + 1, np.int32), [], [], strategy=0)
            return solvers.MultigridLevel(a, empty(n - 1, n), empty(n - 1, n - 1), empty(n, n - 1))
        lists = {k: [None if f is None else (lambda a: Counting()) for f in params.pop(k, [])]
                 for k in ("pre_smoother", "mid_smoother", "post_smoother", "coarsest_solver")}
        n = m[0]
        A = formats.Csr.from_host(gk, n, n, np.zeros(n + 1, np.int32), [], [], strategy=0)
        mg = solvers.Multigrid(gk, A, [level] * len(mg_level), **lists, **params)
        if tweak is not None:
            tweak(mg)

        class Shim:
            def apply(self, b, x):
                return mg.apply(dev(b), dev(x))
        return Shim()
    return make


@pytest.mark.parametrize("name", list(GOLDEN["cycles"]))
def test_cycle_call_sequences(gk, name):
    rec = GOLDEN["cycles"][name]
    got = mu.cycle_steps(device_multigrid_for_steps(gk), rec)
    sync()
    assert mu.steps_match(got, rec), (got, mu.expected_steps(rec))
    assert got == mu.cycle_steps(mu.Multigrid, rec)


def test_can_change_cycle(gk):
    """reference/test/solver/multigrid_kernels.cpp:1248-1275 (CanChangeCycle): generated as V, applied as F"""
    seen = []

    def to_f(mg):
        seen.append(mg.get_cycle())
        mg.set_cycle("f")
        seen.append(mg.get_cycle())
    got = mu.cycle_steps(device_multigrid_for_steps(gk, to_f), GOLDEN["cycles"]["VCycleSame"])
    sync()
    assert seen == ["v", "f"]
    assert got["levels"] == {"0": {"restrict": [0], "prolong": [11]}, "1": {"restrict": [2, 7], "prolong": [4, 9]}}
    assert got["pre"]["1"] == [1, 5, 6, 10] and got["coarsest"] == [3, 8]


def device_parts(gk, fused=None):
    halve = solvers.fixed_coarsening_factory(gk, lambda a: list(range(0, a.nrows, 2)))
    every = solvers.fixed_coarsening_factory(gk, lambda a: list(range(a.nrows)))
    jac = lambda a: solvers.jacobi_generate(gk, a.nrows, a.row_ptrs, a.col_idxs, a.vals, max_block_size=1)
    direct = lambda a: solvers.Direct(gk, solvers.lu_generate(gk, a.nrows, a.row_ptrs, a.col_idxs, a.vals,
                                                              symmetric_sparsity=True))
    def eye(a):     # a plain callable (b, x): x = b, no initial guess -- Multigrid wraps it like build_smoother does
        return lambda b, x: gk.dense_copy_f64(stream_ptr(), a.nrows, b.shape[1], b, b.stride(0), x, x.stride(0))
    def cg(a):      # Cg with an Iteration criterion through the native driver: it takes x as its initial guess
        return lambda b, x: solvers.cg_solve(gk, a.nrows, a.row_ptrs, a.col_idxs, a.vals, b, x=x, max_iters=mu.Cg.ITERATIONS,
                                             reduction=0.0)
    ordered = lambda a: solvers.OrderedCg(gk, a, mu.Cg.ITERATIONS)
    return {"halve": halve, "all_rows": every, "jacobi": jac, "eye": eye, "direct": direct, "cg": ordered, "native_cg": cg,
            "identity": None}


def device_solve(gk, name, fused=None, trace=None, native_cg=False):
    """a whole-apply case of tests/multigrid_util.py through gkomi.solvers.Multigrid, split strategy on every level;
    "cg" on the coarsest level is solvers.OrderedCg, or the native Cg driver with native_cg"""
    def make(m, **params):
        A = formats.Csr.from_host(gk, m[0], m[0], m[2], m[3], m[4], strategy=SPLIT)
        return solvers.Multigrid(gk, A, fused=fused, **params)
    parts = device_parts(gk)
    if native_cg:
        parts["cg"] = parts["native_cg"]
    mg, b, x = mu.restated(name, trace=trace, make=make, parts=parts)
    out = mg.apply(dev(b), dev(x))
    sync()
    return mg, out


CG_CASES = [n for n, c in mu.SOLVE_CASES.items() if c["coarsest"] == "cg"]


@pytest.mark.parametrize("name", [n for n in mu.SOLVE_CASES if n not in CG_CASES])
def test_multigrid_matches_the_reference_executor(gk, name):
    rec = REF[name]
    trace = []
    mg, out = device_solve(gk, name, trace=trace)
    assert [lvl.get_coarse_op().nrows for lvl in mg.get_mg_level_list()] == rec["levels"]
    assert [out["iterations"]] == rec["iterations"]
    assert mu.record_matches(rec["x"], "x", host(out["x"])), name
    # the fused smoother and the three-call sequence: the same bits, the same calls
    trace2 = []
    mg2, out2 = device_solve(gk, name, fused=False, trace=trace2)
    assert same_bits(host(out2["x"]), host(out["x"])) and out2["iterations"] == out["iterations"] and trace2 == trace
    used = [s for s in mg.get_pre_smoother_list() if s is not None]
    if "eye" in mu.SOLVE_CASES[name]["pre"]:
        assert used and all(isinstance(s, solvers._IrSmoother) for s in used)
    else:
        assert used and all(isinstance(s, solvers.JacobiSmoother) and s.fused for s in used)
        assert all(not s.fused for s in mg2.get_pre_smoother_list() if s is not None)


@pytest.mark.parametrize("name", CG_CASES)
def test_native_cg_on_the_coarsest_level(gk, name):
    """The native Cg driver (cg_solve, which takes x as its initial guess) in the coarsest slot.  Its dot products are
    re-ordered on the device, so x is held to the bar the Krylov GPU tests use (1e-6 relative, as smoke() does for Cg),
    not to bits (measured: 4e-17 .. 5e-13); cycle count, level sizes and the call trace are exact.  Bit for bit:
    solvers.OrderedCg, below."""
    rec = REF[name]
    trace, want = [], []
    mg, out = device_solve(gk, name, trace=trace, native_cg=True)
    ref_mg, b, x = mu.restated(name, trace=want)
    ref_x, _, _ = ref_mg.apply(b, x)
    assert trace == want and [out["iterations"]] == rec["iterations"]
    assert [lvl.get_coarse_op().nrows for lvl in mg.get_mg_level_list()] == rec["levels"]
    err = matgen.rel_err(host(out["x"]), ref_x)
    print(name, "relative difference to the reference executor's x:", err)
    assert err < 1e-6


@pytest.mark.parametrize("name", CG_CASES)
def test_cg_on_the_coarsest_level_bit_for_bit(gk, name):
    """x after three cycles equals the reference executor's bit for bit with Cg on the coarsest level: solvers.OrderedCg,
    the reference's kernel sequence with its dot products in the reference's order"""
    mg, out = device_solve(gk, name)
    assert isinstance(mg.get_coarsest_solver(), solvers.OrderedCg)
    got = host(out["x"])
    ref_mg, b, x = mu.restated(name)
    ref_x, _, _ = ref_mg.apply(b, x)
    print(name, "entries that differ:", int(np.sum(got.view(np.int64) != ref_x.view(np.int64))), "of", got.size,
          "largest relative difference:", float(np.max(np.abs(got - ref_x) / np.maximum(np.abs(ref_x), 1e-300))))
    assert mu.record_matches(REF[name]["x"], "x", got), name


def test_call_trace_equals_the_restatement(gk):
    for name in ("ani4/w/mid_standalone", "ani4/f/post_not_pre", "ani4/w/null_entries", "ani1/v/no_reduction"):
        trace, want = [], []
        device_solve(gk, name, trace=trace)
        mg, b, x = mu.restated(name, trace=want)
        mg.apply(b, x)
        assert trace == want, name


def test_zero_guess_ignores_input(gk):
    z = GOLDEN["zero_guess_ignores_input"]
    a = np.array(z["matrix_dense"], np.float64)
    rp, ci, v = matgen.dense_to_csr(a)[-3:]
    A = formats.Csr.from_host(gk, 3, 3, rp, ci, v, strategy=0)
    parts = device_parts(gk)
    common = dict(mg_level=[solvers.fixed_coarsening_factory(gk, lambda m: [0, 2])], pre_smoother=[parts["jacobi"]],
                  coarsest_solver=[parts["direct"]], max_levels=1, min_coarse_rows=1, max_iters=1)
    b = dev(np.array(z["b"], np.float64))
    zero = torch.zeros(3, dtype=torch.float64, device="cuda:0")
    x = dev(np.array(z["x"], np.float64))
    solvers.Multigrid(gk, A, default_initial_guess="provided", **common).apply(b, zero)
    solvers.Multigrid(gk, A, default_initial_guess="zero", **common).apply(b, x)
    sync()
    assert np.allclose(host(zero), host(x), rtol=z["precision"], atol=0.0) and np.any(host(x) != 0.0)


def test_advanced_apply_and_initial_guess_modes(gk):
    m = mu.case_matrix("ani1")
    A = formats.Csr.from_host(gk, m[0], m[0], m[2], m[3], m[4], strategy=SPLIT)
    parts = device_parts(gk)
    mg = solvers.Multigrid(gk, A, [parts["halve"]], pre_smoother=[parts["jacobi"]], min_coarse_rows=10, max_iters=2,
                           coarsest_solver=[parts["direct"]])
    b, x0 = mu.right_hand_side(36), mu.initial_guess(36)
    plain = host(mg.apply(dev(b), dev(x0))["x"])
    x = dev(x0)
    mg.apply_advanced(0.5, dev(b), -2.0, x)
    sync()
    assert same_bits(host(x), -2.0 * x0 + 0.5 * plain)
    from_rhs = host(mg.apply(dev(b), dev(x0), initial_guess="rhs")["x"])
    assert same_bits(from_rhs, host(mg.apply(dev(b), dev(b))["x"]))
    from_zero = host(mg.apply(dev(b), dev(x0), initial_guess="zero")["x"])
    assert same_bits(from_zero, host(mg.apply(dev(b), dev(np.zeros_like(b)))["x"]))


def test_validate(gk):
    A = formats.Csr.from_host(gk, 3, 3, [0, 1, 2, 3], [0, 1, 2], [1.0, 1.0, 1.0])
    f = solvers.fixed_coarsening_factory(gk, lambda m: [0])
    s = lambda a: Counting()
    with pytest.raises(ValueError):
        solvers.Multigrid(gk, A, [])
    with pytest.raises(ValueError):
        solvers.Multigrid(gk, A, [f, None])
    with pytest.raises(ValueError):
        solvers.Multigrid(gk, A, [f, f, f], pre_smoother=[s, s], min_coarse_rows=1)
    with pytest.raises(ValueError):
        solvers.Multigrid(gk, A, [f, f, f], post_uses_pre=False, post_smoother=[s, s], min_coarse_rows=1)
    with pytest.raises(ValueError):
        solvers.Multigrid(gk, A, [f, f, f], mid_smoother=[s, s], min_coarse_rows=1)
    solvers.Multigrid(gk, A, [f, f, f], mid_case="both", mid_smoother=[s, s], min_coarse_rows=1)   # not checked: unused
    with pytest.raises(ValueError):
        solvers.Multigrid(gk, A, [f])                      # 3 rows <= min_coarse_rows: no level


def test_cg_preconditioned_by_one_v_cycle(gk):
    m = mu.case_matrix("1138_bus")
    n = m[0]
    A = formats.Csr.from_host(gk, n, n, m[2], m[3], m[4], strategy=SPLIT)
    parts = device_parts(gk)
    mg = solvers.Multigrid(gk, A, [parts["halve"]], pre_smoother=[parts["jacobi"]], smoother_iters=2, max_levels=2,
                           coarsest_solver=[parts["direct"]], default_initial_guess="zero", max_iters=1)
    b = mu.right_hand_side(n)
    want_x, want_iters = mu.preconditioned_cg(m, b, 500, 1e-6)
    try:
        out = solvers.cg_solve(gk, n, A.row_ptrs, A.col_idxs, A.vals, dev(b[:, 0]), max_iters=500, reduction=1e-6, precond=mg)
    except gkomi.GkomiError:
        if mg.callback().error is not None:
            raise mg.callback().error
        raise
    assert mg.callback().error is None
    print("cg + v-cycle:", out["iterations"], "iterations, restatement", want_iters)
    assert out["converged"] and abs(out["iterations"] - want_iters) <= 1
    assert matgen.rel_err(host(out["x"]), want_x[:, 0]) < 1e-4


def test_multigrid_preconditions_the_other_solvers(gk):
    """through the callback frame of gmres_solve, krylov_solve and solve_op, on the 36-row ani1"""
    m = mu.case_matrix("ani1")
    n = m[0]
    A = formats.Csr.from_host(gk, n, n, m[2], m[3], m[4], strategy=SPLIT)
    parts = device_parts(gk)
    mg = solvers.Multigrid(gk, A, [parts["halve"]], pre_smoother=[parts["jacobi"]], smoother_iters=2, min_coarse_rows=10,
                           coarsest_solver=[parts["direct"]], default_initial_guess="zero", max_iters=1)
    b = dev(mu.right_hand_side(n)[:, 0])
    a = (n, A.row_ptrs, A.col_idxs, A.vals, b)
    for solve in (lambda: solvers.gmres_solve(gk, *a, reduction=1e-8, precond=mg),
                  lambda: solvers.krylov_solve(gk, "bicgstab", *a, reduction=1e-8, precond=mg),
                  lambda: solvers.cg_solve(gk, *a, reduction=1e-8, precond=mg),
                  lambda: solvers.solve_op(gk, "cg", A, b, reduction=1e-8, precond=mg)):
        res = solve()
        assert mg.callback().error is None
        assert res["converged"] and 0 < res["iterations"] <= n, res["iterations"]
