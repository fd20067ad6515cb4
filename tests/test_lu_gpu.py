"""The sparse direct solver on the device against the plain-Python restatement of the reference executor
(tests/lu_util.py): elimination forest, symbolic Cholesky, lu_factorization::initialize / factorize and Direct.
Integers are compared exactly, values bit for bit; out_cols and the factor values sit between sentinel-filled guards."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import gkomi
import ilu_exact_util as xu
import lu_util as lu
from gkomi import solvers
from gpu_util import dev, host, stream_ptr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, "golden", "lu.json")))
GUARD = 64
INT_SENTINEL = -559038737
F64_SENTINEL = -1.2345e300

CASES = {
    "n1": lambda: xu.dense_to_csr([[4.0]]),
    "diagonal_70": lambda: lu.diagonal(70),                                  # every node is a root
    "example": lambda: xu.spd_version(xu.dense_to_csr(G["Example"]["A"])),
    "separable": lambda: xu.spd_version(xu.dense_to_csr(G["Separable"]["A"])),
    "ani1": lambda: lu.read_mtx("ani1.mtx"),
    "ani1_amd": lambda: lu.read_mtx("ani1_amd.mtx"),
    "arrow_150": lambda: xu.arrow(150),                                      # 149 lower entries: 64 + 64 + 21
    "tridiagonal_corners_300": lambda: lu.tridiagonal_with_corners(300),     # one lane climbs 298 steps
    "grid_70x3": lambda: lu.grid_5pt(70, 3),                                 # rows of L of 71 entries
    "grid_24x20": lambda: lu.grid_5pt(24, 20),                               # 480 levels in 480 rows
    "1138_bus": lambda: lu.read_mtx("1138_bus.mtx"),                         # both triangles; nnz(L) = 38312
    "separable_x9_shuffled": lambda: lu.repeated_separable(G["Separable"]["A"]),
    "unsymmetric_values_200": lambda: lu.unsymmetric_values(200),            # L != U^T
}
NAMES = sorted(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """the matrix and everything the restatement says about it, computed once"""
    a = CASES[name]()
    forest = lu.elimination_forest(a)
    L, combined = lu.symbolic_cholesky(a)
    init, diag = lu.lu_initialize(a, combined)
    factor = lu.lu_factorize(init, diag)
    for arr in a + L + combined + init + factor + (diag,) + tuple(forest.values()):
        arr.setflags(write=False)
    return {"a": a, "n": len(a[0]) - 1, "forest": forest, "row_nnz": lu.cholesky_symbolic_count(a, forest), "L": L,
            "combined": combined, "init": init, "diag": diag, "factor": factor}


def dev_csr(m):
    return dev(np.array(m[0], np.int32)), dev(np.array(m[1], np.int32)), dev(np.array(m[2], np.float64))


def guarded(count, dtype, sentinel):
    """a device array of `count` entries between two guards of GUARD sentinels: (whole allocation, the view)"""
    whole = torch.full((count + 2 * GUARD,), sentinel, dtype=dtype, device="cuda:0")
    return whole, whole[GUARD:GUARD + count]


def guards_intact(whole, sentinel):
    h = host(whole)
    return bool(np.all(h[:GUARD] == sentinel) and np.all(h[len(h) - GUARD:] == sentinel))


def dev_forest(forest):
    return {k: dev(np.array(v)) for k, v in forest.items()}


def test_the_cases_are_what_the_table_says():
    assert len(case("1138_bus")["L"][1]) == 38312 and int(np.diff(case("1138_bus")["combined"][0]).max()) == 515
    assert int(np.diff(case("grid_70x3")["L"][0]).max()) == 71
    assert int(np.diff(case("arrow_150")["a"][0])[-1]) == 150
    c = case("separable_x9_shuffled")
    assert c["n"] == 90 and xu.sort_by_column_index(c["a"])[1].tolist() != c["a"][1].tolist()
    assert sum(1 for r, cols in enumerate(lu.pattern_rows(c["a"])) if r not in cols) == 30
    f = case("tridiagonal_corners_300")["forest"]
    assert f["parents"].tolist() == list(range(1, 301))


@pytest.mark.parametrize("name", NAMES)
def test_forest_and_symbolic_cholesky(gk, name):
    c = case(name)
    n, a = c["n"], c["a"]
    rp, ci, _ = dev_csr(a)
    nnz = len(a[1])
    forest = solvers.elimination_forest(gk, n, rp, ci)
    for k in lu.FOREST_FIELDS:
        assert np.array_equal(host(forest[k]), c["forest"][k]), k
    # count and factorize through the C ABI, out_cols between guards
    nb = gk.cholesky_symbolic_workspace_bytes(n, nnz)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda:0")
    lrp = torch.zeros(n + 1, dtype=torch.int32, device="cuda:0")
    total = ctypes.c_int64(-1)
    gk.cholesky_symbolic_count_i32(stream_ptr(), n, nnz, rp, ci, forest["inv_postorder"], forest["postorder_parents"],
                                   lrp, ws, nb, ctypes.addressof(total))
    assert np.array_equal(host(lrp)[:n], c["row_nnz"])
    assert total.value == int(c["row_nnz"].sum()) == len(c["L"][1])
    ptrs = dev(np.array(c["L"][0]))
    whole, out_cols = guarded(total.value, torch.int32, INT_SENTINEL)
    gk.cholesky_symbolic_factorize_i32(stream_ptr(), n, nnz, rp, ci, forest["postorder"], forest["inv_postorder"],
                                       forest["postorder_parents"], ptrs, out_cols, ws, nb)
    assert guards_intact(whole, INT_SENTINEL)
    got = host(out_cols)
    want = lu.pattern_rows(c["L"])
    for row in range(n):
        r = got[c["L"][0][row]:c["L"][0][row + 1]]
        assert r[-1] == row and sorted(r.tolist()) == want[row], row
    # the whole chain
    L, combined = solvers.symbolic_cholesky(gk, n, rp, ci)
    for got_m, want_m in ((L, c["L"]), (combined, c["combined"])):
        assert np.array_equal(host(got_m[0]), want_m[0]) and np.array_equal(host(got_m[1]), want_m[1])
        assert not host(got_m[2]).any()


@pytest.mark.parametrize("name", NAMES)
def test_initialize(gk, name):
    c = case(name)
    n = c["n"]
    rp, ci, v = dev_csr(c["a"])
    frp, fci, _ = dev_csr(c["combined"])
    fnnz = len(c["combined"][1])
    whole, fv = guarded(fnnz, torch.float64, F64_SENTINEL)
    diag = torch.full((n,), -5, dtype=torch.int32, device="cuda:0")
    flag = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
    gk.lu_initialize_f64_i32(stream_ptr(), n, rp, ci, v, fnnz, frp, fci, fv, diag, flag, 8)
    assert guards_intact(whole, F64_SENTINEL)
    assert xu.bits_equal(host(fv), c["init"][2])
    assert np.array_equal(host(diag), c["diag"])


@pytest.mark.parametrize("name", NAMES)
def test_factorize_and_refactorize(gk, name):
    c = case(name)
    n = c["n"]
    rp, ci, v = dev_csr(c["a"])
    f = solvers.lu_generate(gk, n, rp, ci, v, symmetric_sparsity=True)
    assert np.array_equal(host(f.combined[0]), c["combined"][0]) and np.array_equal(host(f.combined[1]), c["combined"][1])
    assert np.array_equal(host(f.diag_idxs), c["diag"])
    assert xu.bits_equal(host(f.combined[2]), c["factor"][2])
    # new values, the same analysis
    a2 = (c["a"][0], c["a"][1], np.random.default_rng(7).uniform(0.5, 1.5, len(c["a"][2])) * c["a"][2])
    want = lu.lu_factorize(*lu.lu_initialize(a2, c["combined"]))
    f.refactorize(dev(a2[2]))
    assert xu.bits_equal(host(f.combined[2]), want[2])


def test_zero_pivot_puts_inf_and_nan_where_the_restatement_does(gk):
    a = lu.with_zero_pivot()
    want, _ = lu.lu_generate(a)
    assert np.isinf(want[2]).any() and np.isnan(want[2]).any()
    rp, ci, v = dev_csr(a)
    f = solvers.lu_generate(gk, 4, rp, ci, v, symmetric_sparsity=True)
    assert xu.bits_equal(host(f.combined[2]), want[2])


def test_caller_supplied_dense_symbolic_pattern(gk):
    n = 40
    a = xu.random_dominant(n, 2, 7, 31)
    dense = xu.dense_to_csr(np.ones((n, n)), keep_zeros=True)
    want, diag = lu.lu_generate(a, symbolic=dense)
    rp, ci, v = dev_csr(a)
    srp, sci, _ = dev_csr(dense)
    f = solvers.lu_generate(gk, n, rp, ci, v, symbolic=(srp, sci))
    assert f.combined[0].data_ptr() != srp.data_ptr() and f.combined[1].data_ptr() != sci.data_ptr()   # copied
    assert np.array_equal(host(f.diag_idxs), diag)
    assert xu.bits_equal(host(f.combined[2]), want[2])
    with pytest.raises(gkomi.GkomiError) as e:
        solvers.lu_generate(gk, n, rp, ci, v)
    assert e.value.code == solvers.GKOMI_ENOTSUPPORTED


def test_unsymmetric_pattern_with_symmetric_sparsity_is_an_error(gk):
    """(3, 40) without (40, 3): the symbolic phase reads the lower triangle only, so the entry has no place"""
    n = 50
    rows = xu.to_rows(xu.tridiagonal(n))
    rows[3][40] = 0.5
    a = xu.from_rows(rows)
    rp, ci, v = dev_csr(a)
    _, combined = solvers.symbolic_cholesky(gk, n, rp, ci)
    fnnz = int(combined[1].numel())
    assert fnnz == 3 * n - 2
    whole, fv = guarded(fnnz, torch.float64, F64_SENTINEL)
    diag = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    flag = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(gkomi.GkomiError) as e:
        gk.lu_initialize_f64_i32(stream_ptr(), n, rp, ci, v, fnnz, combined[0], combined[1], fv, diag, flag, 8)
    assert e.value.code == -1
    assert guards_intact(whole, F64_SENTINEL)
    # every other entry arrived
    rows[3].pop(40)
    assert xu.bits_equal(host(fv), lu.lu_initialize(xu.from_rows(rows), (host(combined[0]), host(combined[1])))[0][2])
    with pytest.raises(gkomi.GkomiError) as e:
        solvers.lu_generate(gk, n, rp, ci, v, symmetric_sparsity=True)
    assert e.value.code == -1
    torch.cuda.synchronize()


def strided(values, extra):
    """a device matrix whose row stride is its column count + extra, the padding filled with a sentinel"""
    n, k = values.shape
    whole = torch.full((n, k + extra), F64_SENTINEL, dtype=torch.float64, device="cuda:0")
    view = whole[:, :k]
    view.copy_(dev(values))
    return whole, view


@pytest.mark.parametrize("name,nrhs", [("ani1", 1), ("ani1_amd", 3), ("1138_bus", 2)])
def test_direct(gk, name, nrhs):
    c = case(name)
    n = c["n"]
    rng = np.random.default_rng(93671)
    x_ref = rng.standard_normal((n, nrhs))
    b = lu.spmv(c["a"], x_ref)
    want = lu.direct_apply(c["factor"], b)
    rp, ci, v = dev_csr(c["a"])
    f = solvers.lu_generate(gk, n, rp, ci, v, symmetric_sparsity=True)
    direct = solvers.Direct(gk, f, nrhs=nrhs)
    _, bd = strided(b, 2)
    x_whole, xd = strided(np.zeros((n, nrhs)), 3)
    direct.apply(bd, xd)
    assert not direct.overrun()
    got = host(xd)
    assert xu.bits_equal(got, want)
    assert np.all(host(x_whole)[:, nrhs:] == F64_SENTINEL)
    # the solution itself, under the reference's own criterion (reference/test/solver/direct.cpp:112)
    if name != "1138_bus":
        assert np.linalg.norm(got - x_ref) <= 10 * np.finfo(np.float64).eps * np.linalg.norm(x_ref)
    # LowerTrs(unit) + UpperTrs on the split factors
    Lm, Um = xu.initialize_l_u(c["factor"])
    lrp, lci, lv = dev_csr(Lm)
    urp, uci, uv = dev_csr(Um)
    tb = gk.trs_workspace_bytes()
    tws = torch.zeros(tb, dtype=torch.uint8, device="cuda:0")
    y = torch.zeros((n, nrhs), dtype=torch.float64, device="cuda:0")
    x2 = torch.zeros((n, nrhs), dtype=torch.float64, device="cuda:0")
    gk.lower_trs_solve_f64_i32(stream_ptr(), n, nrhs, lrp, lci, lv, 1, bd, bd.stride(0), y, nrhs, tws, tb)
    gk.upper_trs_solve_f64_i32(stream_ptr(), n, nrhs, urp, uci, uv, 0, y, nrhs, x2, nrhs, tws, tb)
    assert xu.bits_equal(host(x2), got)
    # x = alpha A^-1 b + beta x: scale, then add_scaled of the plain result
    alpha, beta = 0.5, -2.0
    x0 = rng.standard_normal((n, nrhs))
    _, x3 = strided(x0, 1)
    direct.apply(alpha, bd, beta, x3)
    x4 = dev(x0)
    gk.dense_scale_f64(stream_ptr(), n, nrhs, dev(np.array([beta])), 1, x4, nrhs)
    gk.dense_add_scaled_f64(stream_ptr(), n, nrhs, dev(np.array([alpha])), 1, xd, xd.stride(0), x4, nrhs)
    assert xu.bits_equal(host(x3), host(x4))
    assert xu.bits_equal(host(x3), beta * x0 + alpha * got)


def test_ani4_symbolic_phase(gk):
    """nnz(L) and every row's column set; the numeric comparison is left out for this matrix (the Python yardstick
    would take tens of seconds)"""
    a = lu.read_mtx("ani4.mtx")
    n = len(a[0]) - 1
    want_L, want_combined = lu.symbolic_cholesky(a)
    assert len(want_L[1]) == 179798
    rp, ci, _ = dev_csr(a)
    L, combined = solvers.symbolic_cholesky(gk, n, rp, ci)
    assert np.array_equal(host(L[0]), want_L[0]) and np.array_equal(host(L[1]), want_L[1])
    assert np.array_equal(host(combined[0]), want_combined[0]) and np.array_equal(host(combined[1]), want_combined[1])


def test_mirror_example_runs_on_the_device():
    """Direct over Lu through the C++ mirror on ani1, three right-hand sides, as a fresh child process"""
    import subprocess
    pkg = os.path.join(os.path.dirname(HERE), "repo-8852-ginkgo_amd")
    ex = os.path.join(pkg, "examples")
    r = subprocess.run(["make", "-C", ex, "bin/direct_solver_mirror"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    run = subprocess.run([os.path.join(ex, "bin", "direct_solver_mirror"), os.path.join(HERE, "golden", "ani1.mtx"), "3"],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    checks = [ln for ln in run.stdout.splitlines() if ln.startswith("check ")]
    assert len(checks) == 7 and all(ln.endswith(": ok") for ln in checks), run.stdout
    summary = dict(t.split("=") for t in run.stdout.splitlines()[-1].split()[1:])
    assert summary["rows"] == "36" and summary["factor_nnz"] == "426"
    assert float(summary["residual_norm"]) <= 1e-10 * float(summary["rhs_norm"])


def test_direct_solver_shims_run_on_the_device(tmp_path):
    import subprocess
    from test_lu_reference import build_lu_shim_smoke
    run = subprocess.run([build_lu_shim_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    lines = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("ran ")]
    assert run.returncode == 0 and not [t for t in lines if t[2] != "ok"], run.stdout + run.stderr
    assert [t[1] for t in lines] == ["cholesky::cholesky_symbolic_count", "cholesky::cholesky_symbolic_factorize",
                                     "lu_factorization::initialize", "lu_factorization::factorize"]
