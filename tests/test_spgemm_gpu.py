"""csr::spgemm / advanced_spgemm / spgeam on the device against the plain-Python restatement of the reference loops
(spgemm_util.py): row_ptrs and col_idxs by array_equal, values by their 64-bit patterns.  No tolerance anywhere."""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import gkomi
import matgen
import spgemm_util as su
from gkomi import formats
from gpu_util import host

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "repo-8852-ginkgo_amd")
G = json.load(open(os.path.join(HERE, "golden", "spgemm.json")))


def arrays(s):
    return (np.array(s["row_ptrs"], np.int32), np.array(s["col_idxs"], np.int32), np.array(s["values"], np.float64))


def dcsr(gk, nrows, ncols, m):
    return formats.Csr.from_host(gk, nrows, ncols, *m)


def hcsr(c):
    torch.cuda.synchronize()
    return host(c.row_ptrs), host(c.col_idxs), host(c.vals)


def bins(gk):
    out = (ctypes.c_int64 * 3)()
    gk.csr_spgemm_bins(ctypes.addressof(out))
    return list(out)


def check_product(gk, m, k, n, a, b, alpha=None, beta=None, d=None):
    got = dcsr(gk, m, k, a).spgemm(dcsr(gk, k, n, b), alpha, beta, None if d is None else dcsr(gk, m, n, d))
    assert (got.nrows, got.ncols) == (m, n)
    want = su.spgemm(a, b, alpha, beta, d)
    assert su.same(hcsr(got), want)
    return got, want


def count_call(gk, m, k, n, a, b):
    """the first of the two calls alone: row_ptrs and nnz"""
    A, B = dcsr(gk, m, k, a), dcsr(gk, k, n, b)
    nb = gk.csr_spgemm_workspace_bytes(m, n)
    ws = torch.empty(max(nb, 8), dtype=torch.uint8, device="cuda:0")
    ptrs = torch.full((m + 1,), -1, dtype=torch.int32, device="cuda:0")
    nnz = ctypes.c_int64(-1)
    gk.csr_spgemm_f64_i32(torch.cuda.current_stream().cuda_stream, m, k, A.nnz, A.row_ptrs, A.col_idxs, A.vals, k, n, B.nnz,
                          B.row_ptrs, B.col_idxs, B.vals, None, None, 0, 0, 0, None, None, None, ptrs, None, None,
                          ctypes.addressof(nnz), ws, nb)
    return host(ptrs), nnz.value


# ---- 1. the reference's own tests ------------------------------------------------------------------------------

def test_golden_applies_to_csr_matrix(gk):
    c = G["applies_to_csr_matrix"]
    got = dcsr(gk, 2, 3, arrays(G[c["a"]])).spgemm(dcsr(gk, 3, 3, arrays(G[c["b"]])))
    assert su.same(hcsr(got), arrays(c["expect"]))


def test_golden_applies_linear_combination_to_csr_matrix(gk):
    c = G["applies_linear_combination_to_csr_matrix"]
    got = dcsr(gk, 2, 3, arrays(G[c["a"]])).spgemm(dcsr(gk, 3, 3, arrays(G[c["b"]])), c["alpha"], c["beta"],
                                                  dcsr(gk, 2, 3, arrays(G[c["d"]])))
    assert su.same(hcsr(got), arrays(c["expect"]))


def test_golden_applies_linear_combination_to_identity_matrix(gk):
    c = G["applies_linear_combination_to_identity_matrix"]
    a, b = matgen.dense_to_csr(c["a_dense"]), matgen.dense_to_csr(c["b_dense"])
    got = dcsr(gk, 7, 3, a).spgeam(c["alpha"], c["beta"], dcsr(gk, 7, 3, b))
    assert su.same(hcsr(got), matgen.dense_to_csr(c["expect_dense"]))


# ---- 2. A A on stencils, both calls ----------------------------------------------------------------------------

@pytest.mark.parametrize("gen, g", [(matgen.poisson_2d_5pt, 48), (matgen.poisson_3d_7pt, 12)])
def test_stencil_squared_count_and_fill(gk, gen, g):
    n, rp, ci, v = gen(g)
    v = v * np.sin(1.0 + np.arange(v.size))       # products that round
    a = (rp, ci, v)
    _, want = check_product(gk, n, n, n, a, a)
    ptrs, nnz = count_call(gk, n, n, n, a, a)
    assert np.array_equal(ptrs, want[0]) and nnz == want[0][-1]


# ---- 3. Galerkin product ---------------------------------------------------------------------------------------

def test_galerkin_product_2x2_aggregates(gk):
    g = 64
    n, rp, ci, v = matgen.poisson_2d_5pt(g)
    a = (rp, ci, v * (1.0 + 0.1 * np.cos(np.arange(v.size))))
    p = su.aggregation_2x2(g)
    nc = (g // 2) ** 2
    r = su.transpose(n, nc, p)
    A, P, R = dcsr(gk, n, n, a), dcsr(gk, n, nc, p), dcsr(gk, nc, n, r)
    got = R.spgemm(A.spgemm(P))
    assert su.same(hcsr(got), su.spgemm(r, su.spgemm(a, p)))
    assert (got.nrows, got.ncols) == (nc, nc)


# ---- 4. random rectangular -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rectangular(kind):
    """700 x 500 times 500 x 600, 0-40 nonzeros per row; empty rows of A; rows of A (the first and the last among
    them) that meet only empty rows of B"""
    rng = np.random.default_rng(40)
    m, k, n = 700, 500, 600
    b_counts = rng.integers(0, 41, k)
    b_counts[:25] = 0                                         # rows 0..24 of B are empty
    b = su.random_rows(k, n, b_counts, rng, sort=kind != "b_shuffled", repeat=kind == "b_repeats")
    a_counts = rng.integers(0, 41, m)
    a_counts[[5, 6, 300]] = 0
    a = list(su.random_rows(m, k, a_counts, rng, sort=kind != "a_shuffled", repeat=kind == "a_shuffled"))
    for row in (0, 17, 350, m - 1):                           # only empty B rows: C rows of length 0
        lo, hi = a[0][row], a[0][row + 1]
        a[1][lo:hi] = rng.integers(0, 25, hi - lo)
    return m, k, n, tuple(a), b


@pytest.mark.parametrize("kind", ["sorted", "a_shuffled", "b_shuffled", "b_repeats"])
def test_random_rectangular(gk, kind):
    m, k, n, a, b = rectangular(kind)
    _, want = check_product(gk, m, k, n, a, b)
    lens = np.diff(want[0])
    assert lens[0] == 0 and lens[-1] == 0 and lens[17] == 0 and lens[1:17].max() > 0


# ---- 5. bin edges ----------------------------------------------------------------------------------------------

def test_bin_edges(gk):
    """single rows whose product counts sit at, one below and one above every threshold of the kernel's bins (read
    from the library); one row with many products and a single distinct column"""
    rng = np.random.default_rng(50)
    edges = bins(gk)
    n = 4 * edges[-1]
    # B: row j has j entries for j = 0..32, then rows of 32 entries; the last row is the single column 7
    blens = list(range(33)) + [32] * (edges[-1] // 32 + 2)
    b_counts = np.array(blens + [1])
    k = b_counts.size
    b = list(su.random_rows(k, n, b_counts, rng))
    b[1][-1] = 7
    a_rows = []
    for e in edges:
        for u in (e - 1, e, e + 1):
            full, rest = divmod(u, 32)
            cols = list(33 + np.arange(full)) + ([rest] if rest else [])
            a_rows.append(cols)
            assert sum(blens[c] for c in cols) == u
    a_rows.append([k - 1] * (edges[1] + 5))                   # u large, one distinct column
    a_rows.append([])
    counts = [len(r) for r in a_rows]
    rp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    ci = np.concatenate([np.asarray(r, np.int32) for r in a_rows])
    a = (rp, ci, rng.uniform(-1.0, 1.0, ci.size))
    _, want = check_product(gk, len(a_rows), k, n, a, tuple(b))
    assert np.diff(want[0])[-2] == 1


# ---- 6. beyond LDS, 11. determinism ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def long_row_case():
    rng = np.random.default_rng(60)
    k, n = 4000, 20000
    b = su.random_rows(k, n, np.full(k, 30), rng)
    counts = rng.integers(0, 12, 201)
    counts[100] = 3000
    a = su.random_rows(201, k, counts, rng, sort=False)
    return 201, k, n, a, b


def test_long_row_among_short_rows(gk):
    m, k, n, a, b = long_row_case()
    assert 3000 * 30 > bins(gk)[-1]
    got, want = check_product(gk, m, k, n, a, b)
    again = dcsr(gk, m, k, a).spgemm(dcsr(gk, k, n, b))
    assert su.same(hcsr(again), hcsr(got))


def test_long_row_with_unsorted_b(gk):
    """the one-lane walk on the dense path: B's rows reversed"""
    m, k, n, a, b = long_row_case()
    rp, ci, v = b[0], b[1].copy(), b[2].copy()
    keep = a[0][100] + 200                                     # shorten the long row: one lane walks it
    a2 = (np.concatenate([a[0][:101], a[0][101:] - (a[0][101] - keep)]).astype(np.int32),
          np.concatenate([a[1][:keep], a[1][a[0][101]:]]), np.concatenate([a[2][:keep], a[2][a[0][101]:]]))
    ci = ci.reshape(k, 30)[:, ::-1].ravel().copy()
    v = v.reshape(k, 30)[:, ::-1].ravel().copy()
    check_product(gk, m, k, n, a2, (rp, ci, v))


# ---- 7. advanced form ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alpha, beta", [(-1.0, 2.0), (0.1, 1.0 / 3.0)])
@pytest.mark.parametrize("d_sorted", [True, False])
def test_advanced_form(gk, alpha, beta, d_sorted):
    rng = np.random.default_rng(70)
    m, k, n = 300, 200, 250
    b = su.random_rows(k, n, rng.integers(0, 30, k), rng)
    a_counts = rng.integers(0, 20, m)
    a_counts[[0, 10, 11, m - 1]] = 0                           # D has rows where A has none
    a = su.random_rows(m, k, a_counts, rng, sort=False)
    plain = su.spgemm(a, b)
    d_counts = rng.integers(1, 25, m)
    d_counts[[3, 4]] = 0
    d = su.random_rows(m, n, d_counts, rng, sort=d_sorted)
    _, want = check_product(gk, m, k, n, a, b, alpha, beta, d)
    inside = sum(np.isin(d[1][d[0][r]:d[0][r + 1]], plain[1][plain[0][r]:plain[0][r + 1]]).sum() for r in range(m))
    assert 0 < inside < d[1].size and want[0][1] == d_counts[0]


def test_advanced_form_takes_device_scalars(gk):
    c = G["applies_linear_combination_to_csr_matrix"]
    al = torch.tensor([c["alpha"]], dtype=torch.float64, device="cuda:0")
    be = torch.tensor([c["beta"]], dtype=torch.float64, device="cuda:0")
    got = dcsr(gk, 2, 3, arrays(G[c["a"]])).spgemm(dcsr(gk, 3, 3, arrays(G[c["b"]])), al, be, dcsr(gk, 2, 3, arrays(G[c["d"]])))
    assert su.same(hcsr(got), arrays(c["expect"]))


# ---- 8. cancellation -------------------------------------------------------------------------------------------

def test_cancelled_entries_stay_with_their_sign(gk):
    # row 0: 1*2 + (-1)*2 = +0.0 at column 0, 0.0 + 1*(-0.0) = +0.0 at column 1; row 1: products -0.0 and 0.0 alone;
    # row 2: (-1)*0.0 = -0.0 added to +0.0 at column 2, and (-2.25)*2 + 1*4.5 = 0.0 at column 0
    a = (np.array([0, 2, 3, 6], np.int32), np.array([0, 1, 2, 2, 0, 3], np.int32), np.array([1.0, -1.0, 1.0, -1.0, -2.25, 1.0]))
    b = (np.array([0, 2, 3, 5, 6], np.int32), np.array([0, 1, 0, 1, 2, 0], np.int32), np.array([2.0, -0.0, 2.0, -0.0, 0.0, 4.5]))
    got, want = check_product(gk, 3, 4, 3, a, b)
    v = hcsr(got)[2]
    assert np.array_equal(hcsr(got)[1], [0, 1, 1, 2, 0, 1, 2])
    assert v[0] == 0.0 and not np.signbit(v[0]) and not np.signbit(v[1])
    # advanced: alpha = -1 flips the products, beta * d = -0.0 first
    d = (np.array([0, 1, 1, 2], np.int32), np.array([2, 1], np.int32), np.array([0.0, -0.0]))
    check_product(gk, 3, 4, 3, a, b, -1.0, 1.0, d)
    check_product(gk, 3, 4, 3, a, b, 1.0, -1.0, d)


# ---- 9. SpGEAM -------------------------------------------------------------------------------------------------

def check_sum(gk, m, n, alpha, a, beta, b):
    got = dcsr(gk, m, n, a).spgeam(alpha, beta, dcsr(gk, m, n, b))
    want = su.spgeam(alpha, a, beta, b)
    assert su.same(hcsr(got), want)
    return want


def test_spgeam_sorted_pairs(gk):
    rng = np.random.default_rng(90)
    m, n = 400, 300
    ca, cb = rng.integers(0, 20, m), rng.integers(0, 20, m)
    ca[[0, 7, 8]] = 0
    cb[[7, 9, m - 1]] = 0
    a, b = su.random_rows(m, n, ca, rng), su.random_rows(m, n, cb, rng)
    check_sum(gk, m, n, 0.1, a, 1.0 / 3.0, b)
    check_sum(gk, m, n, -3.0, a, 2.0, (a[0], a[1], rng.uniform(-1, 1, a[2].size)))        # identical patterns
    lo = su.random_rows(m, n // 2, ca, rng)
    hi = su.random_rows(m, n // 2, cb, rng)
    want = check_sum(gk, m, n, 2.0, lo, 0.5, (hi[0], hi[1] + n // 2, hi[2]))               # disjoint patterns
    assert want[0][-1] == lo[0][-1] + hi[0][-1]


def test_spgeam_infinite_beta_against_a_missing_entry(gk):
    a = (np.array([0, 2, 2], np.int32), np.array([0, 2], np.int32), np.array([1.0, 2.0]))
    b = (np.array([0, 1, 2], np.int32), np.array([2, 1], np.int32), np.array([3.0, 4.0]))
    want = check_sum(gk, 2, 3, 2.0, a, float("inf"), b)
    assert np.isnan(want[2][0]) and np.isinf(want[2][1])


def test_spgeam_unsorted_rows_follow_the_merge(gk):
    rng = np.random.default_rng(91)
    m, n = 100, 40
    a = su.random_rows(m, n, rng.integers(0, 10, m), rng, sort=False)
    b = su.random_rows(m, n, rng.integers(0, 10, m), rng, sort=False, repeat=True)
    check_sum(gk, m, n, 0.1, a, -0.7, b)


# ---- 10. errors ------------------------------------------------------------------------------------------------

def test_errors(gk):
    g = G["mtx"]
    A = dcsr(gk, 2, 3, arrays(g))
    B = dcsr(gk, 3, 3, arrays(G["mtx3_unsorted"]))
    with pytest.raises(gkomi.GkomiError) as e:
        A.spgemm(A)                                            # 2x3 times 2x3
    assert e.value.code == -1
    with pytest.raises(gkomi.GkomiError) as e:
        A.spgemm(B, alpha=2.0)
    assert e.value.code == -1
    nnz = ctypes.c_int64(0)
    ptrs = torch.zeros(3, dtype=torch.int32, device="cuda:0")
    ws = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(gkomi.GkomiError) as e:
        gk.csr_spgemm_f64_i32(None, 2, 3, A.nnz, A.row_ptrs, A.col_idxs, A.vals, 3, 3, B.nnz, B.row_ptrs, B.col_idxs, B.vals,
                              None, None, 0, 0, 0, None, None, None, ptrs, None, None, ctypes.addressof(nnz), ws, 64)
    assert e.value.code == -4
    with pytest.raises(gkomi.GkomiError) as e:
        gk.csr_spgeam_f64_i32(None, 2, 3, ws, A.nnz, A.row_ptrs, A.col_idxs, A.vals, ws, 2, 3, A.nnz, A.row_ptrs, A.col_idxs, A.vals,
                              ptrs, None, None, ctypes.addressof(nnz), ws, 8)
    assert e.value.code == -4
    empty = (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    got = dcsr(gk, 0, 3, empty).spgemm(B)
    assert (got.nrows, got.ncols, got.nnz) == (0, 3, 0) and np.array_equal(host(got.row_ptrs), [0])
    got = dcsr(gk, 2, 3, (np.zeros(3, np.int32), empty[1], empty[2])).spgemm(B)              # an all-empty A
    assert got.nnz == 0 and np.array_equal(host(got.row_ptrs), [0, 0, 0])
    got = dcsr(gk, 0, 3, empty).spgeam(1.0, 1.0, dcsr(gk, 0, 3, empty))
    assert got.nnz == 0


# ---- 12.-14. the mirror and the shim ---------------------------------------------------------------------------

def test_mirror_example(gk):
    ex = os.path.join(PKG, "examples")
    r = subprocess.run(["make", "-C", ex, "bin/spgemm_mirror"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(ex, "bin", "spgemm_mirror")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("spgemm_mirror:")]
    assert len(line) == 1, r.stdout
    kv = dict(t.split("=") for t in line[0].split()[1:])
    assert kv["exact_match"] == "1" and kv["advanced_match"] == "1" and kv["converged"] == "1"
    assert 0 < int(kv["cg_iterations"]) < 500 and int(kv["coarse_rows"]) == 256


def test_spgemm_shims_run_on_the_device(tmp_path):
    from test_spgemm_reference import build_spgemm_shim_smoke
    run = subprocess.run([build_spgemm_shim_smoke(tmp_path)], capture_output=True, text=True)
    ran = {t[1]: t[2] for t in (ln.split() for ln in run.stdout.splitlines()) if len(t) == 3 and t[0] == "ran"}
    assert run.returncode == 0, run.stdout + run.stderr
    assert ran == {k: "ok" for k in ("csr::spgemm", "csr::advanced_spgemm", "csr::spgeam")}, ran


STATE_SRC = r"""
#include <ginkgo/ginkgo.hpp>
#include <cstdio>
using csr = gko::matrix::Csr<double, gko::int32>;
using dense = gko::matrix::Dense<double>;
int main()
{
    auto exec = gko::HipExecutor::create(0, gko::ReferenceExecutor::create());
    const int n = 300;
    gko::matrix_data<double, gko::int32> ad, xd;
    ad.size = {n, n};
    xd.size = {n, n};
    for (int i = 0; i < n; ++i) {
        if (i > 0) ad.nonzeros.emplace_back(i, i - 1, -1.0 - 0.001 * i);
        ad.nonzeros.emplace_back(i, i, 2.0 + 0.01 * i);
        if (i + 1 < n) ad.nonzeros.emplace_back(i, i + 1, -0.5);
        xd.nonzeros.emplace_back(i, (i * 7) % n, 1.0 + i);
    }
    auto A = csr::create(exec), X = csr::create(exec);
    A->read(ad);
    X->read(xd);
    auto b = dense::create(exec->get_master(), gko::dim<2>(n, 1));
    for (int i = 0; i < n; ++i) b->at(i, 0) = 1.0 / (1.0 + i);
    auto db = b->clone(exec);
    auto y = dense::create(exec, gko::dim<2>(n, 1));
    X->apply(gko::lend(db), gko::lend(y));          // X builds its srow and row statistic from the OLD pattern
    A->apply(gko::lend(A), gko::lend(X));           // X = A A through adopt()
    X->apply(gko::lend(db), gko::lend(y));
    gko::matrix_data<double, gko::int32> out;
    X->write(out);
    auto hy = y->clone(exec->get_master());
    std::printf("nnz %zu\n", out.nonzeros.size());
    for (const auto& e : out.nonzeros) std::printf("e %d %d %a\n", (int)e.row, (int)e.column, e.value);
    for (int i = 0; i < n; ++i) std::printf("y %a\n", hy->at(i, 0));
    return 0;
}
"""


def test_apply_after_a_product_sees_the_new_matrix(oracle, tmp_path):
    """the state-coherence rule for adopt(): x->apply(dense, dense) after x received a product equals the oracle SpMV
    of the new matrix"""
    src, exe = tmp_path / "state.cpp", tmp_path / "state"
    src.write_text(STATE_SRC)
    r = subprocess.run(["g++", "-O1", "-std=c++17", f"-I{PKG}/include", str(src), "-o", str(exe), f"-L{PKG}/lib", "-lgkomi",
                        f"-Wl,-rpath,{PKG}/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    n = 300
    ents = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("e ")]
    rows = np.array([int(t[1]) for t in ents])
    ci = np.array([int(t[2]) for t in ents], np.int32)
    v = np.array([float.fromhex(t[3]) for t in ents])
    y = np.array([float.fromhex(ln.split()[1]) for ln in run.stdout.splitlines() if ln.startswith("y ")])
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    assert 3 * n < v.size <= 5 * n and np.all(np.diff(rows) >= 0)
    b = (1.0 / (1.0 + np.arange(n))).reshape(n, 1)
    expect = np.empty((n, 1))
    oracle.ref_csr_spmv(n, 1, rp, ci, v, b, 1, expect, 1)
    assert np.array_equal(y.view(np.uint64), expect[:, 0].view(np.uint64))
