"""CPU checks of the SpGEMM / SpGEAM yardstick: the restatement of the reference loops (spgemm_util.py) reproduces the
reference's own known answers (tests/golden/spgemm.json) exactly, agrees bit for bit with the pinned C oracle's CSR
SpMV and with an independent numpy union; the mirror example and the shim compile; the ABI rejects bad arguments."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import matgen
import spgemm_util as su

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "repo-8852-ginkgo_amd")
G = json.load(open(os.path.join(HERE, "golden", "spgemm.json")))


def arrays(s):
    return (np.array(s["row_ptrs"], np.int32), np.array(s["col_idxs"], np.int32), np.array(s["values"], np.float64))


def test_restatement_applies_to_csr_matrix():
    c = G["applies_to_csr_matrix"]
    assert su.same(su.spgemm(arrays(G[c["a"]]), arrays(G[c["b"]])), arrays(c["expect"]))


def test_restatement_applies_linear_combination_to_csr_matrix():
    c = G["applies_linear_combination_to_csr_matrix"]
    got = su.spgemm(arrays(G[c["a"]]), arrays(G[c["b"]]), c["alpha"], c["beta"], arrays(G[c["d"]]))
    assert su.same(got, arrays(c["expect"]))


def test_restatement_applies_linear_combination_to_identity_matrix():
    c = G["applies_linear_combination_to_identity_matrix"]
    got = su.spgeam(c["alpha"], matgen.dense_to_csr(c["a_dense"]), c["beta"], matgen.dense_to_csr(c["b_dense"]))
    # GKO_ASSERT_MTX_NEAR + GKO_ASSERT_MTX_EQ_SPARSITY against initialize<Mtx>(expect): here every value is exact
    assert su.same(got, matgen.dense_to_csr(c["expect_dense"]))


def test_restatement_spgemm_equals_the_oracle_csr_spmv(oracle):
    """ties the new checker to the pinned one: with B a dense matrix written as CSR with full rows, every entry of
    A B starts at zero and receives a * b in A's storage order on both sides"""
    rng = np.random.default_rng(20)
    a = su.random_rows(300, 40, rng.integers(1, 10, 300), rng, sort=False)
    bd = rng.uniform(-1.0, 1.0, (40, 3))
    b = (np.arange(0, 3 * 40 + 1, 3, dtype=np.int32), np.tile(np.arange(3, dtype=np.int32), 40), bd.ravel().copy())
    rp, ci, v = su.spgemm(a, b)
    expect = np.empty((300, 3))
    oracle.ref_csr_spmv(300, 3, a[0], a[1], a[2], bd, 3, expect, 3)
    assert np.array_equal(rp, np.arange(0, 901, 3)) and np.array_equal(ci, np.tile(np.arange(3), 300))
    assert np.array_equal(v.reshape(300, 3).view(np.uint64), expect.view(np.uint64))


def test_restatement_spgeam_equals_the_column_union():
    """sorted, duplicate-free rows: the merge yields the ascending union of the two patterns, alpha a + beta b each"""
    rng = np.random.default_rng(21)
    nrows, ncols, alpha, beta = 60, 50, 0.1, 1.0 / 3.0
    a = su.random_rows(nrows, ncols, rng.integers(0, 12, nrows), rng)
    b = su.random_rows(nrows, ncols, rng.integers(0, 12, nrows), rng)
    rp, ci, v = su.spgeam(alpha, a, beta, b)
    da, db = np.zeros((nrows, ncols)), np.zeros((nrows, ncols))
    pa, pb = np.zeros((nrows, ncols), bool), np.zeros((nrows, ncols), bool)
    for m, dm, pm in ((a, da, pa), (b, db, pb)):
        rows = np.repeat(np.arange(nrows), np.diff(m[0]))
        dm[rows, m[1]] = m[2]
        pm[rows, m[1]] = True
    union = pa | pb
    rows, cols = np.nonzero(union)
    assert np.array_equal(rp, np.concatenate([[0], np.cumsum(union.sum(axis=1))])) and np.array_equal(ci, cols)
    assert np.array_equal(v.view(np.uint64), (alpha * da + beta * db)[rows, cols].view(np.uint64))


def test_mirror_example_compiles():
    """examples/spgemm_mirror.cpp: Csr::apply with Csr and Identity operands, a Galerkin product and a Cg solve on it"""
    src = open(os.path.join(PKG, "examples", "spgemm_mirror.cpp")).read()
    for needle in ("gko::matrix::Csr<double, gko::int32>", "transpose()", "gko::matrix::Identity<double>", "gko::solver::Cg<double>"):
        assert needle in src
    r = subprocess.run(["make", "-C", os.path.join(PKG, "examples"), "bin/spgemm_mirror"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def build_spgemm_shim_smoke(tmp_path):
    """shims/hip/matrix/csr_kernels.hip.cpp against the mirror, linked with shims/test/shim_smoke5.cpp"""
    obj, exe = tmp_path / "csr_kernels.o", tmp_path / "shim_smoke5"
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Wno-unused-parameter", f"-I{ROOT}/include", f"-I{PKG}/include", "-include",
                        os.path.join(ROOT, "shims", "test", "prelude_mirror.hpp"), "-c",
                        os.path.join(ROOT, "shims", "hip", "matrix", "csr_kernels.hip.cpp"), "-o", str(obj)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(["g++", "-std=c++14", f"-I{ROOT}/include", f"-I{PKG}/include", f"-I{ROOT}/shims/test",
                        os.path.join(ROOT, "shims", "test", "shim_smoke5.cpp"), str(obj), "-o", str(exe), f"-L{PKG}/lib", "-lgkomi",
                        f"-Wl,-rpath,{PKG}/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_spgemm_shim_compiles_against_the_mirror(tmp_path):
    assert os.path.exists(build_spgemm_shim_smoke(tmp_path))


def test_abi_rejects_bad_spgemm_arguments(gk):
    """before any HIP call: inner dimension, alpha without beta or D, D of another shape, negative sizes, null arrays
    with non-zero counts; spgeam operands of different shapes"""
    import gkomi
    nnz = ctypes.c_int64(-1)
    out = (8, None, None, ctypes.addressof(nnz), None, 0)

    def code(fn, *args):
        with pytest.raises(gkomi.GkomiError) as e:
            fn(*args)
        return e.value.code

    a = (2, 3, 1, 8, 8, 8)          # nrows, ncols, nnz, three non-null arrays
    none_d = (None, None, 0, 0, 0, None, None, None)
    assert code(gk.csr_spgemm_f64_i32, None, *a, 4, 2, 1, 8, 8, 8, *none_d, *out) == -1      # 2x3 times 4x2
    assert code(gk.csr_spgemm_f64_i32, None, *a, 3, 2, 1, 8, 8, 8, 8, None, 0, 0, 0, None, None, None, *out) == -1   # alpha alone
    assert code(gk.csr_spgemm_f64_i32, None, *a, 3, 2, 1, 8, 8, 8, 8, 8, 0, 0, 0, None, None, None, *out) == -1      # no D
    assert code(gk.csr_spgemm_f64_i32, None, *a, 3, 2, 1, 8, 8, 8, 8, 8, 2, 3, 1, 8, 8, 8, *out) == -1               # D is 2x3, C 2x2
    assert code(gk.csr_spgemm_f64_i32, None, -1, 3, 0, None, None, None, 3, 2, 1, 8, 8, 8, *none_d, *out) == -1
    assert code(gk.csr_spgemm_f64_i32, None, 2, 3, 1, 8, None, None, 3, 2, 1, 8, 8, 8, *none_d, *out) == -1
    assert code(gk.csr_spgemm_f64_i32, None, *a, 3, 2, 1, 8, 8, 8, *none_d, *out) == -4      # no workspace
    assert code(gk.csr_spgeam_f64_i32, None, 2, 3, 8, 1, 8, 8, 8, 8, 2, 4, 1, 8, 8, 8, *out) == -1
    assert code(gk.csr_spgeam_f64_i32, None, 2, 3, 8, 1, 8, 8, 8, None, 2, 3, 1, 8, 8, 8, *out) == -1
    assert gk.csr_spgemm_workspace_bytes(-1, 4) == 0 and gk.csr_spgemm_workspace_bytes(10, 10) > 0
    assert gk.csr_spgeam_workspace_bytes(10) > 0
    bins = (ctypes.c_int64 * 3)()
    assert gk.csr_spgemm_bins(ctypes.addressof(bins)) == 0
    assert 0 < bins[0] < bins[1] < bins[2]
