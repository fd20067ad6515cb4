"""CPU side of the sparse direct solver: the plain-Python restatement (tests/lu_util.py) reproduces what the
reference's own tests expect (tests/golden/lu.json, ani1*_chol.mtx, ani1*_lu.mtx), the host elimination-forest entry of
the library equals the restatement, the mirror example builds, the two shims compile against the mirror prelude and link
with shims/test/shim_smoke7.cpp, and the C ABI rejects bad arguments before any HIP call."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import gkomi
import ilu_exact_util as xu
import lu_util as lu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "repo-8852-ginkgo_amd")
G = json.load(open(os.path.join(HERE, "golden", "lu.json")))
R_DOUBLE = 10 * np.finfo(np.float64).eps     # r<double>::value (core/test/utils.hpp:212-219)

FILLED = {
    "example": lambda: xu.spd_version(xu.dense_to_csr(G["Example"]["A"])),
    "separable": lambda: xu.spd_version(xu.dense_to_csr(G["Separable"]["A"])),
    "ani1": lambda: lu.read_mtx("ani1.mtx"),
    "ani1_amd": lambda: lu.read_mtx("ani1_amd.mtx"),
    "arrow_150": lambda: xu.arrow(150),
    "tridiagonal_corners_300": lambda: lu.tridiagonal_with_corners(300),
    "grid_70x3": lambda: lu.grid_5pt(70, 3),
    "grid_24x20": lambda: lu.grid_5pt(24, 20),
    "1138_bus": lambda: lu.read_mtx("1138_bus.mtx"),
    "separable_x9_shuffled": lambda: lu.repeated_separable(G["Separable"]["A"]),
    "unsymmetric_values_200": lambda: lu.unsymmetric_values(200),
    "zero_pivot": lu.with_zero_pivot,
    "diagonal_70": lambda: lu.diagonal(70),
    "n1": lambda: xu.dense_to_csr([[4.0]]),
}


@pytest.mark.parametrize("name", ["Example", "Separable"])
def test_restatement_reproduces_the_known_answers(name):
    c = G[name]
    a = xu.dense_to_csr(c["A"])
    forest = lu.elimination_forest(a)
    assert lu.cholesky_symbolic_count(a, forest).tolist() == c["row_nnz"]
    rp, ci = lu.cholesky_symbolic_factorize(a, forest)
    want = lu.pattern_rows(xu.dense_to_csr(c["L"]))
    for row in range(10):
        r = ci[rp[row]:rp[row + 1]].tolist()
        assert r[-1] == row and sorted(r) == want[row]
    assert lu.pattern_rows(lu.symbolic_cholesky(a)[0]) == want


@pytest.mark.parametrize("name,l_nnz,lu_nnz", [("ani1", 231, 426), ("ani1_amd", 183, 330)])
def test_restatement_reproduces_the_reference_s_factor_files(name, l_nnz, lu_nnz):
    a = lu.read_mtx(name + ".mtx")
    if name == "ani1":
        assert lu.cholesky_symbolic_count(a, lu.elimination_forest(a)).tolist() == G["ani1_row_nnz"]
    L, combined = lu.symbolic_cholesky(a)
    assert len(L[1]) == l_nnz and len(combined[1]) == lu_nnz
    assert lu.pattern_rows(L) == lu.pattern_rows(lu.read_mtx(name + "_chol.mtx"))
    ref = lu.read_mtx(name + "_lu.mtx")
    assert np.array_equal(combined[0], ref[0]) and np.array_equal(combined[1], ref[1])
    factor, diag = lu.lu_generate(a)
    assert [int(factor[1][d]) for d in diag] == list(range(len(diag)))
    # GKO_ASSERT_MTX_NEAR(..., r<double>::value), reference/test/factorization/lu_kernels.cpp:187
    assert np.linalg.norm(factor[2] - ref[2]) <= R_DOUBLE * np.linalg.norm(ref[2])
    print(name, "largest absolute difference", np.abs(factor[2] - ref[2]).max())


@pytest.mark.parametrize("name", sorted(FILLED))
def test_factorize_is_compute_lu_on_a_filled_pattern(name):
    a = FILLED[name]()
    init, diag = lu.lu_initialize(a, lu.symbolic_cholesky(a)[1])
    assert xu.bits_equal(lu.lu_factorize(init, diag)[2], xu.compute_lu(init)[2])


def test_factorize_is_compute_lu_on_a_dense_symbolic_pattern():
    a = xu.random_dominant(40, 2, 7, 31)
    init, diag = lu.lu_initialize(a, xu.dense_to_csr(np.ones((40, 40)), keep_zeros=True))
    assert xu.bits_equal(lu.lu_factorize(init, diag)[2], xu.compute_lu(init)[2])


def host_forest(gk, m):
    n = len(m[0]) - 1
    out = [np.full(n + 2 if k == "child_ptrs" else max(n, 1), -7, np.int32) for k in lu.FOREST_FIELDS]
    gk.elimination_forest_host_i32(n, np.ascontiguousarray(m[0]), np.ascontiguousarray(m[1]), *out)
    return {k: (o if k == "child_ptrs" else o[:n]) for k, o in zip(lu.FOREST_FIELDS, out)}


@pytest.mark.parametrize("name", sorted(set(FILLED) - {"zero_pivot"}) + ["Separable", "ani4"])
def test_host_forest_entry_equals_the_restatement(gk, name):
    a = (xu.dense_to_csr(G["Separable"]["A"]) if name == "Separable" else lu.read_mtx("ani4.mtx") if name == "ani4"
         else FILLED[name]())
    want = lu.elimination_forest(a)
    got = host_forest(gk, a)
    for k in lu.FOREST_FIELDS:
        assert np.array_equal(got[k], want[k]), k
    # a forest: every parent is larger than its node, the postorder is a permutation that lists children first
    n = len(a[0]) - 1
    assert all(want["parents"][i] > i for i in range(n))
    assert sorted(want["postorder"].tolist()) == list(range(n))
    assert all(want["postorder_parents"][i] > i for i in range(n))


@pytest.mark.parametrize("name,nrhs", [("ani1", 1), ("ani1_amd", 3)])
def test_restated_direct_solves_the_reference_s_cases(name, nrhs):
    """reference/test/solver/direct.cpp:104-125: x drawn from N(0, 1), b = A x, GKO_ASSERT_MTX_NEAR(x, x_ref, r<double>)"""
    a = lu.read_mtx(name + ".mtx")
    x_ref = np.random.default_rng(93671).standard_normal((36, nrhs))
    b = lu.spmv(a, x_ref)
    factor, _ = lu.lu_generate(a)
    x = lu.direct_apply(factor, b)
    err = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
    print(name, "error / bound", err / R_DOUBLE)
    assert err <= R_DOUBLE
    # the combined matrix and the split factors give the same bits
    L, U = xu.initialize_l_u(factor)
    assert xu.bits_equal(lu.upper_trs(U, lu.lower_trs(L, b, True), False), x)


def test_mirror_example_builds():
    ex = os.path.join(PKG, "examples")
    r = subprocess.run(["make", "-C", ex, "bin/direct_solver_mirror"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(os.path.join(ex, "bin", "direct_solver_mirror"))


def build_lu_shim_smoke(tmp_path):
    """shims/hip/factorization/{cholesky,lu}_kernels.hip.cpp against the mirror, linked with shims/test/shim_smoke7.cpp"""
    objs = []
    for name in ("cholesky_kernels", "lu_kernels"):
        obj = tmp_path / f"{name}.o"
        r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Wno-unused-parameter", f"-I{ROOT}/include", f"-I{PKG}/include",
                            "-include", os.path.join(ROOT, "shims", "test", "prelude_mirror.hpp"), "-c",
                            os.path.join(ROOT, "shims", "hip", "factorization", f"{name}.hip.cpp"), "-o", str(obj)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        objs.append(str(obj))
    exe = tmp_path / "shim_smoke7"
    r = subprocess.run(["g++", "-std=c++14", f"-I{ROOT}/include", f"-I{PKG}/include", f"-I{ROOT}/shims/test",
                        os.path.join(ROOT, "shims", "test", "shim_smoke7.cpp"), *objs, "-o", str(exe), f"-L{PKG}/lib", "-lgkomi",
                        f"-Wl,-rpath,{PKG}/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_direct_solver_shims_compile_against_the_mirror(tmp_path):
    assert os.path.exists(build_lu_shim_smoke(tmp_path))


def raises(code, fn, *args):
    with pytest.raises(gkomi.GkomiError) as e:
        fn(*args)
    assert e.value.code == code, (e.value.code, code)


def test_abi_rejects_bad_arguments_before_any_hip_call(gk):
    EINVAL, ENOTSUPPORTED, EWORKSPACE = -1, -2, -4
    out = [np.zeros(8, np.int32) for _ in range(6)]
    rp = np.array([0, 1, 2], np.int32)
    # forest: negative size, missing arrays, decreasing row_ptrs, a negative column
    raises(EINVAL, gk.elimination_forest_host_i32, -1, rp, rp, *out)
    raises(EINVAL, gk.elimination_forest_host_i32, 2, None, rp, *out)
    raises(EINVAL, gk.elimination_forest_host_i32, 2, rp, rp, out[0], None, *out[2:])
    raises(EINVAL, gk.elimination_forest_host_i32, 2, rp, None, *out)
    raises(EINVAL, gk.elimination_forest_host_i32, 2, np.array([0, 2, 1], np.int32), np.array([0, 0], np.int32), *out)
    raises(EINVAL, gk.elimination_forest_host_i32, 2, rp, np.array([0, -1], np.int32), *out)
    raises(ENOTSUPPORTED, gk.elimination_forest_host_i32, 2 ** 31, rp, rp, *out)
    raises(EINVAL, gk.elimination_forest_i32, None, -1, 8, 8, 8, 8, 8, 8, 8, 8)
    raises(EINVAL, gk.elimination_forest_i32, None, 2, None, 8, 8, 8, 8, 8, 8, 8)
    raises(EINVAL, gk.elimination_forest_i32, None, 2, 8, 8, 8, 8, 8, 8, 8, None)
    # n = 0 is an empty forest: child_ptrs = {0, 0}
    cp = np.full(2, -1, np.int32)
    assert gk.elimination_forest_host_i32(0, np.zeros(1, np.int32), None, None, cp, None, None, None, None) == 0
    assert cp.tolist() == [0, 0]
    # symbolic Cholesky
    assert gk.cholesky_symbolic_workspace_bytes(-1, 0) == 0 and gk.cholesky_symbolic_workspace_bytes(4, -1) == 0
    need = gk.cholesky_symbolic_workspace_bytes(4, 10)
    assert need >= 4 * (10 + 10 + 4)
    total = ctypes.c_int64(-1)
    at = ctypes.addressof(total)
    raises(EINVAL, gk.cholesky_symbolic_count_i32, None, -1, 0, 8, 8, 8, 8, 8, 8, need, at)
    raises(EINVAL, gk.cholesky_symbolic_count_i32, None, 4, -1, 8, 8, 8, 8, 8, 8, need, at)
    raises(EINVAL, gk.cholesky_symbolic_count_i32, None, 4, 10, 8, 8, 8, 8, 8, 8, need, None)
    raises(EINVAL, gk.cholesky_symbolic_count_i32, None, 4, 10, 8, 8, None, 8, 8, 8, need, at)
    raises(EINVAL, gk.cholesky_symbolic_count_i32, None, 4, 10, 8, None, 8, 8, 8, 8, need, at)
    raises(EWORKSPACE, gk.cholesky_symbolic_count_i32, None, 4, 10, 8, 8, 8, 8, 8, 8, need - 1, at)
    raises(EWORKSPACE, gk.cholesky_symbolic_count_i32, None, 4, 10, 8, 8, 8, 8, 8, None, need, at)
    raises(ENOTSUPPORTED, gk.cholesky_symbolic_count_i32, None, 2 ** 31, 10, 8, 8, 8, 8, 8, 8, need, at)
    assert gk.cholesky_symbolic_count_i32(None, 0, 0, None, None, None, None, None, None, 0, at) == 0 and total.value == 0
    raises(EINVAL, gk.cholesky_symbolic_factorize_i32, None, -1, 0, 8, 8, 8, 8, 8, 8, 8, 8, need)
    raises(EINVAL, gk.cholesky_symbolic_factorize_i32, None, 4, 10, 8, 8, 8, 8, 8, 8, None, 8, need)
    raises(EINVAL, gk.cholesky_symbolic_factorize_i32, None, 4, 10, 8, 8, None, 8, 8, 8, 8, 8, need)
    raises(EWORKSPACE, gk.cholesky_symbolic_factorize_i32, None, 4, 10, 8, 8, 8, 8, 8, 8, 8, 8, need - 1)
    assert gk.cholesky_symbolic_factorize_i32(None, 0, 0, None, None, None, None, None, None, None, None, 0) == 0
    # lu_factorization
    raises(EINVAL, gk.lu_initialize_f64_i32, None, -1, 8, 8, 8, 0, 8, 8, 8, 8, 8, 8)
    raises(EINVAL, gk.lu_initialize_f64_i32, None, 4, 8, 8, 8, -1, 8, 8, 8, 8, 8, 8)
    raises(EINVAL, gk.lu_initialize_f64_i32, None, 4, None, 8, 8, 10, 8, 8, 8, 8, 8, 8)
    raises(EINVAL, gk.lu_initialize_f64_i32, None, 4, 8, 8, 8, 10, 8, 8, None, 8, 8, 8)
    raises(EINVAL, gk.lu_initialize_f64_i32, None, 4, 8, 8, 8, 10, 8, 8, 8, None, 8, 8)
    raises(EWORKSPACE, gk.lu_initialize_f64_i32, None, 4, 8, 8, 8, 10, 8, 8, 8, 8, 8, 3)
    raises(EWORKSPACE, gk.lu_initialize_f64_i32, None, 4, 8, 8, 8, 10, 8, 8, 8, 8, None, 8)
    raises(ENOTSUPPORTED, gk.lu_initialize_f64_i32, None, 4, 8, 8, 8, 2 ** 31, 8, 8, 8, 8, 8, 8)
    assert gk.lu_initialize_f64_i32(None, 0, None, None, None, 0, None, None, None, None, None, 0) == 0
    raises(EINVAL, gk.lu_factorize_f64_i32, None, -1, None, None, None, None, 0)
    raises(EWORKSPACE, gk.lu_factorize_f64_i32, None, 4, 8, 8, 8, 8, 16)
    raises(EWORKSPACE, gk.lu_factorize_f64_i32, None, 4, 8, 8, 8, None, 1 << 20)
    # Lu::generate without a symbolic factorization and without symmetric_sparsity (lu.cpp:98)
    raises(ENOTSUPPORTED, gk.lu_symbolic_supported, 0, 0)
    assert gk.lu_symbolic_supported(0, 1) == 0 and gk.lu_symbolic_supported(1, 0) == 0 and gk.lu_symbolic_supported(1, 1) == 0


def test_python_layer_refuses_before_it_touches_a_device(gk):
    from gkomi import solvers
    with pytest.raises(gkomi.GkomiError) as e:
        solvers.lu_generate(gk, 4, None, None, None)
    assert e.value.code == solvers.GKOMI_ENOTSUPPORTED
