"""ISAI on the device against the plain-Python restatement of the reference executor's kernels (tests/isai_util.py)
and against the results recorded from the reference executor itself (tests/golden/isai_ref.json): bit for bit --
patterns and prefix arrays with array_equal, values by their bytes.  Only where the reference's default excess solver
is iterative (general and spd patterns with long rows) the comparison is the reference's own bound for "a different
excess solver" against its stored inverses."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import ilu_exact_util as xu
import isai_util as iu
import spgemm_util as su
from gkomi import solvers
from gpu_util import DevCsr, csr_apply_srow, dev, host, make_srow

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, "golden", "isai.json")))
REF = json.load(open(os.path.join(HERE, "golden", "isai_ref.json")))
R_DOUBLE = 10 * np.finfo(np.float64).eps     # r<double>::value (core/test/utils.hpp:212-219)
N = 131                                      # neither a wave's two rows nor a workgroup's four divide it


def d3(m):
    return tuple(dev(np.array(a)) for a in m)


def h3(m):
    torch.cuda.synchronize()
    return tuple(host(a) for a in m)


def same_csr(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and xu.bits_equal(got[2], want[2])


def matches(rec, got):
    return iu.digest(got) == rec["sha256"]


def zeroed(m):
    return m[0], m[1], np.zeros(len(m[2]))


def device_kernel(gk, kind, m, pattern):
    """the generate kernel alone -> (inverse, excess_rhs_ptrs, excess_nz_ptrs) on the host, and the device arrays"""
    n = len(m[0]) - 1
    md, pd = d3(m), d3(pattern)
    rhs_ptrs, nz_ptrs = solvers.isai_generate_kernel(gk, kind, n, md, pd)
    return h3(pd), host(rhs_ptrs), host(nz_ptrs), (md, pd, rhs_ptrs, nz_ptrs)


def device_excess_system(gk, n, state, host_rhs_ptrs, host_nz_ptrs, start, end):
    md, pd, rhs_ptrs, nz_ptrs = state
    e_dim = int(host_rhs_ptrs[end] - host_rhs_ptrs[start])
    e_nnz = int(host_nz_ptrs[end] - host_nz_ptrs[start])
    system, rhs = solvers.isai_excess_system(gk, n, md, pd, rhs_ptrs, nz_ptrs, e_dim, e_nnz, start, end)
    return h3(system), host(rhs)


# ---- the recorded cases: kernels alone and generate whole ------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def recorded_case(name):
    kind, power, limit, make = iu.RECORDED_CASES[name]
    m = make()
    for a in m:
        a.setflags(write=False)
    return kind, power, limit, m


@pytest.mark.parametrize("name", list(iu.RECORDED_CASES))
def test_kernels_equal_the_recorded_ones_bit_for_bit(gk, name):
    """generate_tri_inverse / generate_general_inverse on the zeroed pattern, then generate_excess_system of every block of
    the loop over excess_limit"""
    kind, power, limit, m = recorded_case(name)
    rec = REF["cases"][name]["records"]
    n = len(m[0]) - 1
    md = d3(m)
    base = solvers._split_l(gk, n, *md, diag_sqrt=False) if kind == "spd" else md
    pattern = h3(solvers.isai_extend_sparsity(gk, n, base, power) if (kind != "spd" or power > 1) else base)
    direct, rhs_ptrs, nz_ptrs, state = device_kernel(gk, kind, m, zeroed(pattern))
    assert matches(rec["kernel/excess_rhs_ptrs"], rhs_ptrs) and matches(rec["kernel/excess_nz_ptrs"], nz_ptrs)
    assert matches(rec["kernel/direct"], direct)
    blocks = iu.excess_blocks(rhs_ptrs, limit)
    assert len(blocks) == rec["kernel/counts"]["items"][3]
    for b, (start, end) in enumerate(blocks):
        assert rec[f"excess/{b}/range"]["items"] == [start, end]
        system, rhs = device_excess_system(gk, n, state, rhs_ptrs, nz_ptrs, start, end)
        assert matches(rec[f"excess/{b}/system"], system) and matches(rec[f"excess/{b}/rhs_vals"], rhs)


@pytest.mark.parametrize("name", [k for k, c in REF["cases"].items() if "generate/inverse" in c["records"]])
def test_generate_equals_the_recorded_inverse_bit_for_bit(gk, name):
    kind, power, limit, m = recorded_case(name)
    n = len(m[0]) - 1
    trace = {}
    inv = solvers.isai_generate(gk, kind, n, *d3(m), sparsity_power=power, excess_limit=limit, trace=trace)
    got = h3(inv[0] if kind == "spd" else inv)
    rec = REF["cases"][name]["records"]
    assert len(trace["blocks"]) == rec["kernel/counts"]["items"][3]
    assert matches(rec["generate/inverse"], got)
    if kind == "spd":
        assert same_csr(h3(inv[1]), su.transpose(n, n, got))


# ---- generated cases against the restatement run here ---------------------------------------------------------------

def explicit_pattern(n, cols_of):
    return xu.from_rows([{c: 0.0 for c in cols_of(r)} for r in range(n)])


def general_with_pivoting():
    """rows whose dense systems need a swap (a zero leading entry), meet two candidates of equal magnitude, or are
    singular"""
    rng = np.random.RandomState(3)
    rows = []
    for r in range(N):
        row = {c: float(rng.uniform(-1.0, 1.0)) for c in range(max(0, r - 3), min(N, r + 4))}
        if r % 4 == 0:
            row[r] = 0.0                                    # a stored zero on the diagonal: the pivot search must swap
        elif r % 4 == 1:
            for c in row:
                row[c] = 0.5 if (c + r) % 2 else -0.5       # every candidate of the same magnitude
        elif r % 4 == 2 and r + 1 < N:
            row = dict(rows[r - 1]) if set(rows[r - 1]) == set(row) else row
        rows.append(row)
    # rows 40 ... 47: two equal rows over the same columns -> singular blocks
    for r in range(40, 48):
        rows[r] = {c: 1.0 for c in range(38, 50)}
    return xu.from_rows(rows)


def spd_with_negative_entries():
    """a symmetric matrix that is not positive definite: the last entry of some solutions is negative, the root a NaN"""
    m = iu.spd_banded(N, 3)
    rows = xu.to_rows(m)
    for r in range(0, N, 6):
        rows[r][r] = -rows[r][r]
    return xu.from_rows(rows)


def tri_case(name):
    """-> (kind, M, pattern)"""
    lower = not name.startswith("upper")
    kind = "lower" if lower else "upper"
    what = name.split("/", 1)[1]
    if what.startswith("band"):
        m = iu.banded(N, int(what[4:]), lower)
        return kind, m, m
    if what == "alternating":
        m = iu.alternating(N, 3, 40, lower)
        return kind, m, m
    if what == "one_long_at_the_end":
        m = iu.alternating(N, 4, 50, lower, long_if=lambda r: r == (N - 1 if lower else 0))
        return kind, m, m
    if what == "empty_rows":
        m = iu.banded(N, 5, lower)
        return kind, m, explicit_pattern(N, lambda r: [] if r % 3 == 0 else xu.to_rows(m)[r])
    if what == "foreign_columns":
        # pattern columns that row `col` of M does not hold, and columns on the other side of the diagonal
        m = iu.banded(N, 3, lower)
        return kind, m, explicit_pattern(N, lambda r: sorted({max(0, r - 9), max(0, r - 4), r, min(N - 1, r + 2), min(N - 1, r + 7)}))
    if what == "zero_pivot":
        rows = xu.to_rows(iu.banded(N, 6, lower))
        for r in range(0, N, 4):
            rows[r][r] = 0.0
        m = xu.from_rows(rows)
        return kind, m, m
    if what == "missing_diagonal":
        rows = xu.to_rows(iu.banded(N, 6, lower))
        for r in range(1, N - 1, 4):
            rows[r].pop(r)
        m = xu.from_rows(rows)
        return kind, m, m
    raise KeyError(name)


TRI_CASES = [f"{k}/{w}" for k in ("lower", "upper") for w in
             ["band1", "band2", "band31", "band32", "band33", "band40", "band64", "band65", "alternating",
              "one_long_at_the_end", "empty_rows", "foreign_columns", "zero_pivot", "missing_diagonal"]]


def check_kernel_and_excess(gk, kind, m, pattern, ranges=None):
    n = len(m[0]) - 1
    want, want_rhs, want_nz = iu.generic_generate(m, zeroed(pattern), kind)
    got, rhs_ptrs, nz_ptrs, state = device_kernel(gk, kind, m, zeroed(pattern))
    assert np.array_equal(rhs_ptrs, want_rhs) and np.array_equal(nz_ptrs, want_nz)
    assert same_csr(got, want)
    for start, end in ranges if ranges is not None else [(0, n)]:
        w_sys, w_rhs = iu.generate_excess_system(m, pattern, want_rhs, want_nz, start, end)
        g_sys, g_rhs = device_excess_system(gk, n, state, rhs_ptrs, nz_ptrs, start, end)
        assert same_csr(g_sys, w_sys) and xu.bits_equal(g_rhs, w_rhs), (start, end)
    return want_rhs


@pytest.mark.parametrize("name", TRI_CASES)
def test_tri_kernels_equal_the_restatement_bit_for_bit(gk, name):
    kind, m, pattern = tri_case(name)
    rhs_ptrs = check_kernel_and_excess(gk, kind, m, pattern, ranges=[(0, N), (0, 0), (N, N), (7, 90), (64, N)])
    k = int(name.split("band")[1]) if "band" in name else None
    if k is not None:
        # exactly min(k, room) entries per row: long rows from 33 on
        assert (rhs_ptrs[N] > 0) == (k > iu.ROW_SIZE_LIMIT)


@pytest.mark.parametrize("name", [c for c in TRI_CASES if c.split("/")[1] in
                                  ("band32", "band33", "band65", "alternating", "one_long_at_the_end", "zero_pivot")])
@pytest.mark.parametrize("limit", [0, 1, 40, 10 ** 6])
def test_tri_generate_equals_the_restatement_bit_for_bit(gk, name, limit):
    """the whole of generate_inverse: the excess loop with excess_limit 1 (one long row per block), the size of one long
    row of the alternating case (40), and beyond the total; no long row at all skips the loop"""
    kind, m, _ = tri_case(name)
    trace, want_trace = {}, {}
    got = h3(solvers.isai_generate(gk, kind, N, *d3(m), excess_limit=limit, trace=trace))
    want = iu.generate_inverse(m, kind, excess_limit=limit, trace=want_trace)
    assert trace["blocks"] == [(e["start"], e["end"]) for e in want_trace["excess"]]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2], equal_nan=True)
    finite = np.isfinite(want[2])
    assert xu.bits_equal(got[2][finite], want[2][finite])


def test_power_of_the_pattern_follows_square_and_multiply(gk):
    m = iu.banded(N, 3, True)
    for power in (2, 3, 4, 5, 6):
        got = h3(solvers.isai_generate(gk, "lower", N, *d3(m), sparsity_power=power))
        assert same_csr(got, iu.generate_inverse(m, "lower", sparsity_power=power)), power


GENERAL_CASES = {
    "general/band": lambda: ("general", iu.general_banded(N, 2, 3)),
    "general/band32": lambda: ("general", iu.general_banded(N, 15, 16)),
    "general/band33_and_more": lambda: ("general", iu.general_banded(N, 20, 20)),
    "general/every_row_long": lambda: ("general", iu.general_banded(N, 35, 35)),
    "general/pivoting": lambda: ("general", general_with_pivoting()),
    "spd/band": lambda: ("spd", iu.spd_banded(N, 4)),
    "spd/negative_last_entry": lambda: ("spd", spd_with_negative_entries()),
    "spd/long_rows": lambda: ("spd", iu.spd_banded(N, 40)),
}


@pytest.mark.parametrize("name", sorted(GENERAL_CASES))
def test_general_kernels_equal_the_restatement_bit_for_bit(gk, name):
    kind, m = GENERAL_CASES[name]()
    pattern = xu.initialize_l(m) if kind == "spd" else m
    rhs_ptrs = check_kernel_and_excess(gk, kind, m, pattern, ranges=[(0, N), (5, 77)])
    lengths = iu.row_lengths(pattern)
    if name == "general/every_row_long":
        assert lengths.min() > iu.ROW_SIZE_LIMIT and rhs_ptrs[N] == lengths.sum()
    if name == "general/band32":
        assert lengths.max() == iu.ROW_SIZE_LIMIT and rhs_ptrs[N] == 0
    if name == "spd/negative_last_entry":
        # the guard fired: identity rows
        want = xu.to_rows(iu.generic_generate(m, zeroed(pattern), kind)[0])
        assert sum(all(v == (1.0 if c == r else 0.0) for c, v in row.items()) for r, row in enumerate(want)) >= N // 6


def test_the_pivoting_case_swaps_ties_and_meets_singular_blocks():
    """what the case above is there for, on the restatement: a swap, a tie and a singular block are met"""
    m = general_with_pivoting()
    rows = xu.to_rows(m)
    assert rows[4][4] == 0.0 and len({abs(v) for v in rows[5].values()}) == 1 and rows[42] == rows[43]
    inv = xu.to_rows(iu.generic_generate(m, zeroed(m), "general")[0])
    assert all(v == (1.0 if c == 43 else 0.0) for c, v in inv[43].items())     # singular: the guard's identity row


def test_scale_and_scatter_equal_the_restatement(gk):
    rng = np.random.RandomState(1)
    sizes = [0, 3, 0, 33, 1, 70, 0, 5, 64, 0]
    n = len(sizes)
    ptrs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    sol = rng.uniform(0.5, 2.0, int(ptrs[-1]))
    sol[ptrs[4] - 1] = -1.0                                   # block 3 ends in a negative entry: NaN throughout
    rows = [{c: 0.0 for c in range(s)} for s in sizes]
    inverse = xu.from_rows(rows)
    s = torch.cuda.current_stream().cuda_stream
    for start, end in ((0, n), (1, 6), (3, 4), (2, 2)):
        part = sol[ptrs[start]:ptrs[end]].copy()
        want = iu.scale_excess_solution(ptrs, part, start, end)
        got = dev(part)
        gk.isai_scale_excess_solution_f64_i32(s, n, dev(ptrs), got, start, end)
        torch.cuda.synchronize()
        assert np.array_equal(host(got), want, equal_nan=True)
        ok = np.isfinite(want)
        assert xu.bits_equal(host(got)[ok], want[ok])
        inv_d = d3(inverse)
        gk.isai_scatter_excess_solution_f64_i32(s, n, dev(ptrs), dev(part), inv_d[0], inv_d[2], start, end)
        assert same_csr(h3(inv_d), iu.scatter_excess_solution(ptrs, part, inverse, start, end))
    # the reference's KernelScatterExcessSolution
    c = G["kernel_scatter"]
    as_csr = lambda m: (np.array(m["row_ptrs"], np.int32), np.array(m["col_idxs"], np.int32), np.array(m["vals"], np.float64))
    md = d3(as_csr(c["matrix"]))
    gk.isai_scatter_excess_solution_f64_i32(s, 6, dev(np.array(c["ptrs"], np.int32)), dev(np.array(c["solution"], np.float64)),
                                            md[0], md[2], 0, 6)
    assert same_csr(h3(md), as_csr(c["expect"]))


# ---- long rows through the iterative default: the reference's bound for a different excess solver ----------------------

def golden(name):
    return iu.golden_mtx(name, 12345.0)


def distance(got, want):
    g, w = xu.csr_to_dense(got), xu.csr_to_dense(want)
    return np.linalg.norm(g - w) / np.linalg.norm(w)


@pytest.mark.parametrize("kind,matrix,inverse,bound", [("general", "isai_a.mtx", "isai_a_inv.mtx", 2e4),
                                                       ("spd", "isai_spd.mtx", "isai_spd_inv.mtx", 1e3),
                                                       ("lower", "isai_l.mtx", "isai_l_inv.mtx", 1e3),
                                                       ("upper", "isai_u.mtx", "isai_u_inv.mtx", 1e3)])
def test_long_rows_through_gmres_stay_within_the_reference_s_bound(gk, kind, matrix, inverse, bound):
    """ReturnsCorrectInverse{A,Spd,L,U}LongrowWithExcessSolver: equal sparsity, and bound * r<double> against the stored
    inverse.  General and spd take GMRES with block-Jacobi by default; lower and upper are given it."""
    m, want = golden(matrix), golden(inverse)
    n = len(m[0]) - 1
    inv = solvers.isai_generate(gk, kind, n, *d3(m), excess_solver=solvers.isai_gmres_excess_solver)
    got = h3(inv[0] if kind == "spd" else inv)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    dist = distance(got, want)
    print(f"{kind}: distance {dist:.3e}, bound {bound * R_DOUBLE:.3e}")
    assert dist <= bound * R_DOUBLE
    if kind == "spd":
        assert distance(h3(inv[1]), su.transpose(n, n, want)) <= bound * R_DOUBLE


# ---- the apply ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nrhs", [1, 3])
def test_apply_callback_is_the_spmv_entry_point(gk, nrhs):
    L, U = iu.ilu0_factors("ani4.mtx")
    n = len(L[0]) - 1
    li = solvers.isai_generate(gk, "lower", n, *d3(L), sparsity_power=2)
    ui = solvers.isai_generate(gk, "upper", n, *d3(U), sparsity_power=2)
    b = dev(np.cos(0.1 * np.arange(n * nrhs)).reshape(n, nrhs))

    def direct(m, x):
        A = DevCsr(n, n, *h3(m))
        tile = int(gk.csr_srow_tile_for(A.nnz))
        srow, tile = make_srow(gk, A, tile)
        return csr_apply_srow(gk, A, x, srow, tile)
    one = solvers.isai_from_inverses(gk, n, li, nrhs=nrhs)
    x = torch.full((n, nrhs), float("nan"), dtype=torch.float64, device=b.device)
    one.apply(b, x)
    want = direct(li, b)
    torch.cuda.synchronize()
    assert xu.bits_equal(host(x), host(want))
    two = solvers.isai_from_inverses(gk, n, li, ui, nrhs=nrhs)
    y = torch.full((n, nrhs), float("nan"), dtype=torch.float64, device=b.device)
    two.apply(b, y)
    want2 = direct(ui, want)
    torch.cuda.synchronize()
    assert xu.bits_equal(host(y), host(want2))
    assert np.isfinite(host(y)).all()


def test_known_applies_of_the_reference(gk):
    """Apply* and UseWithIluPreconditioner of the reference's tests through the callback"""
    def mat(name):
        return xu.dense_to_csr(np.array(G["matrices"][name]["dense"], np.float64))
    for c in G["apply"]:
        if "alpha" in c:
            continue
        m = mat(c["matrix"])
        pre = solvers.isai_preconditioner(gk, c["kind"], 3, *d3(m))
        x = torch.zeros((3, 1), dtype=torch.float64, device="cuda:0")
        pre.apply(dev(np.array(c["vec"], np.float64).reshape(3, 1)), x)
        torch.cuda.synchronize()
        want = np.array(c["expect"], np.float64)
        assert np.linalg.norm(host(x)[:, 0] - want) <= R_DOUBLE * np.linalg.norm(want), c["test"]
    c = G["ilu"]
    pre = solvers.ilu_isai_from_factors(gk, 3, d3(mat(c["l"])), d3(mat(c["u"])))
    x = torch.zeros((3, 1), dtype=torch.float64, device="cuda:0")
    pre.apply(dev(np.array(c["vec"], np.float64).reshape(3, 1)), x)
    torch.cuda.synchronize()
    want = np.array(c["expect"], np.float64)
    assert np.linalg.norm(host(x)[:, 0] - want) <= R_DOUBLE * np.linalg.norm(want)


# ---- solves ------------------------------------------------------------------------------------------------------------

def true_residual(m, x, b):
    rp, ci, v = m
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    return b - np.bincount(rows, weights=v * x[ci], minlength=len(b))


@pytest.mark.parametrize("power", [1, 2])
def test_gmres_with_ilu_over_isai_on_ani4(gk, power):
    m = iu.golden_mtx("ani4.mtx")
    n = len(m[0]) - 1
    md = d3(m)
    ilu = solvers.ilu_generate(gk, n, *md)
    pre = solvers.ilu_isai_from_factors(gk, n, ilu.L, ilu.U, sparsity_power=power)
    b = np.cos(0.3 * np.arange(n))
    plain = solvers.gmres_solve(gk, n, *md, dev(b), krylov_dim=30, max_iters=5000, reduction=1e-10)
    res = solvers.gmres_solve(gk, n, *md, dev(b), krylov_dim=30, max_iters=5000, reduction=1e-10, precond=pre)
    trs = solvers.gmres_solve(gk, n, *md, dev(b), krylov_dim=30, max_iters=5000, reduction=1e-10, precond=ilu)
    print(f"ani4 power {power}: {res['iterations']} iterations with isai, {trs['iterations']} with the triangular solves, "
          f"{plain['iterations']} without")
    assert res["converged"] and res["iterations"] < plain["iterations"]
    r = true_residual(m, host(res["x"]), b)
    assert np.linalg.norm(r) <= 2e-10 * np.linalg.norm(b) * 10


@pytest.mark.parametrize("which", ["ic_over_isai", "spd_isai"])
def test_cg_with_isai_on_1138_bus(gk, which):
    """Ic over LowerIsai runs at sparsity power 2: the gap between CG's recurrence residual and the true one grows with the
    iteration count on this matrix whatever the preconditioner -- measured (profiles/isai_probe.md): 3.2e-9 after the 3102
    iterations of CG without one, 2.5e-9 after the 1486 of power 1, 1.1e-9 after the 340 of power 2 -- so the tolerance of
    tests/test_gmres_precond_gpu.py (2e-9) says something about the preconditioner only where the solve is short."""
    m = iu.golden_mtx("1138_bus.mtx")
    n = len(m[0]) - 1
    md = d3(m)
    if which == "ic_over_isai":
        ic = solvers.ic_generate(gk, n, *md)
        pre = solvers.ic_isai_from_factor(gk, n, ic.L, sparsity_power=2)
        assert same_csr(h3(pre.u_inverse), su.transpose(n, n, h3(pre.l_inverse)))
    else:
        pre = solvers.isai_preconditioner(gk, "spd", n, *md)
    b = np.ones(n)
    plain = solvers.cg_solve(gk, n, *md, dev(b), max_iters=20000, reduction=1e-10)
    res = solvers.cg_solve(gk, n, *md, dev(b), max_iters=20000, reduction=1e-10, precond=pre)
    print(f"1138_bus {which}: {res['iterations']} iterations, {plain['iterations']} without")
    assert res["converged"] and res["iterations"] < plain["iterations"]
    r = true_residual(m, host(res["x"]), b)
    assert np.linalg.norm(r) <= 2e-10 * np.linalg.norm(b) * 10


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------

MIRROR_SRC = r"""
#include <ginkgo/ginkgo.hpp>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
using dense = gko::matrix::Dense<double>;
using csr = gko::matrix::Csr<double, gko::int32>;
using namespace gko::preconditioner;

static void put(const char* what, const csr* m)
{
    gko::matrix_data<double, gko::int32> d;
    m->write(d);
    std::printf("%s", what);
    for (const auto& e : d.nonzeros) std::printf(" %d:%d:%a", static_cast<int>(e.row), static_cast<int>(e.column), e.value);
    std::printf("\n");
}
static void put(const char* what, const dense* v)
{
    auto h = v->clone(v->get_executor()->get_master());
    std::printf("%s", what);
    for (gko::size_type i = 0; i < h->get_size()[0]; ++i) std::printf(" %a", h->at(i, 0));
    std::printf("\n");
}
static std::unique_ptr<dense> vec(std::shared_ptr<const gko::Executor> exec, const std::vector<double>& v)
{
    auto h = dense::create(exec->get_master(), gko::dim<2>(v.size(), 1));
    for (gko::size_type i = 0; i < v.size(); ++i) h->at(i, 0) = v[i];
    return h->clone(exec);
}
// hides what the preconditioner is: the solver reaches it through the generic callback
struct hidden : gko::LinOp {
    explicit hidden(std::shared_ptr<const gko::LinOp> op) : gko::LinOp(op->get_executor(), op->get_size()), op_(std::move(op)) {}
    void apply_impl(const gko::LinOp* b, gko::LinOp* x) const override { op_->apply(b, x); }
    void apply_impl(const gko::LinOp* a, const gko::LinOp* b, const gko::LinOp* c, gko::LinOp* x) const override { op_->apply(a, b, c, x); }
    std::shared_ptr<const gko::LinOp> op_;
};
template <class Pre>
static void applies(std::shared_ptr<const gko::Executor> exec, const Pre* pre, const std::vector<double>& v)
{
    if (v.empty()) return;
    auto b = vec(exec, v);
    auto x = dense::create(exec, b->get_size());
    pre->apply(b.get(), x.get());
    put("apply", x.get());
    std::vector<double> start(v.size());
    const double init[3] = {2.0, -3.0, 1.0};
    for (gko::size_type i = 0; i < v.size(); ++i) start[i] = init[i % 3];
    auto y = vec(exec, start);
    auto alpha = gko::initialize<dense>({3.0}, exec), beta = gko::initialize<dense>({-4.0}, exec);
    pre->apply(alpha.get(), b.get(), beta.get(), y.get());
    put("advanced", y.get());
}
template <isai_type T>
static int isai_case(std::shared_ptr<const gko::Executor> exec, std::shared_ptr<csr> A, int power, const std::vector<double>& v)
{
    using isai = Isai<T, double, gko::int32>;
    auto pre = isai::build().with_sparsity_power(power).on(exec)->generate(A);
    auto inv = pre->get_approximate_inverse();
    put("inverse", inv.get());
    auto t = pre->transpose();
    auto tt = dynamic_cast<const typename isai::transposed_type*>(t.get());
    if (tt == nullptr) return 5;
    put("transposed", tt->get_approximate_inverse()->transpose().get());
    auto ct = pre->conj_transpose();
    auto ctt = dynamic_cast<const typename isai::transposed_type*>(ct.get());
    if (ctt == nullptr) return 6;
    put("conj_transposed", ctt->get_approximate_inverse()->transpose().get());
    applies(exec, pre.get(), v);
    gkomi_apply_fn fn = nullptr;
    void* ctx = nullptr;
    std::printf("native %d\n", pre->native_callback(fn, ctx, 1) && fn == &gkomi_isai_apply_cb ? 1 : 0);
    return 0;
}
template <>
int isai_case<isai_type::spd>(std::shared_ptr<const gko::Executor> exec, std::shared_ptr<csr> A, int power, const std::vector<double>& v)
{
    using isai = SpdIsai<double, gko::int32>;
    auto pre = isai::build().with_sparsity_power(power).on(exec)->generate(A);
    auto ops = pre->get_approximate_inverse()->get_operators();
    if (ops.size() != 2) return 7;
    put("inverse", dynamic_cast<const csr*>(ops[1].get()));
    put("inverse_t", dynamic_cast<const csr*>(ops[0].get()));
    auto t = pre->transpose();
    auto tt = dynamic_cast<const isai*>(t.get());
    if (tt == nullptr) return 5;
    put("transposed", dynamic_cast<const csr*>(tt->get_approximate_inverse()->get_operators()[1].get()));
    auto ct = pre->conj_transpose();
    auto ctt = dynamic_cast<const isai*>(ct.get());
    if (ctt == nullptr) return 6;
    put("conj_transposed", dynamic_cast<const csr*>(ctt->get_approximate_inverse()->get_operators()[1].get()));
    applies(exec, pre.get(), v);
    gkomi_apply_fn fn = nullptr;
    void* ctx = nullptr;
    std::printf("native %d\n", pre->native_callback(fn, ctx, 1) && fn == &gkomi_isai_apply_cb ? 1 : 0);
    return 0;
}

int main(int argc, char** argv)
{
    try {
        auto exec = gko::HipExecutor::create(0, gko::ReferenceExecutor::create());
        const std::string kind = argv[1];
        const int power = std::atoi(argv[2]);
        auto A = gko::share(gko::read<csr>(std::ifstream(argv[3]), exec));
        std::vector<double> v;
        for (int i = 4; i < argc; ++i) v.push_back(std::strtod(argv[i], nullptr));
        if (kind == "lower") return isai_case<isai_type::lower>(exec, A, power, v);
        if (kind == "upper") return isai_case<isai_type::upper>(exec, A, power, v);
        if (kind == "general") return isai_case<isai_type::general>(exec, A, power, v);
        if (kind == "spd") return isai_case<isai_type::spd>(exec, A, power, v);
        if (kind == "non_square") {
            try {
                GeneralIsai<>::build().on(exec)->generate(A);
            } catch (const gko::DimensionMismatch&) {
                std::printf("refused DimensionMismatch\n");
            }
            return 0;
        }
        if (kind != "ilu" && kind != "ic") return 3;
        // Ilu / Ic over Isai solvers: the apply, then a solve by the native callback and by the generic one
        auto l_factory = LowerIsai<>::build().with_sparsity_power(power).on(exec);
        auto u_factory = UpperIsai<>::build().with_sparsity_power(power).on(exec);
        std::shared_ptr<const gko::LinOp> pre;
        if (kind == "ilu") {
            pre = gko::share(Ilu<>::build().with_factorization_factory(gko::factorization::Ilu<>::build().on(exec)).with_l_solver_factory(l_factory)
                                 .with_u_solver_factory(u_factory).on(exec)->generate(A));
            auto p = dynamic_cast<const Ilu<>*>(pre.get());
            std::printf("solvers %d\n", dynamic_cast<const LowerIsai<>*>(p->get_l_solver().get()) && dynamic_cast<const UpperIsai<>*>(p->get_u_solver().get()) ? 1 : 0);
        } else {
            pre = gko::share(Ic<>::build().with_factorization_factory(gko::factorization::Ic<>::build().on(exec)).with_l_solver_factory(l_factory).on(exec)->generate(A));
            auto p = dynamic_cast<const Ic<>*>(pre.get());
            std::printf("solvers %d\n", dynamic_cast<const LowerIsai<>*>(p->get_l_solver().get()) && dynamic_cast<const UpperIsai<>*>(p->get_lh_solver().get()) ? 1 : 0);
        }
        gkomi_apply_fn fn = nullptr;
        void* ctx = nullptr;
        std::printf("native %d\n", dynamic_cast<const gko::detail::native_preconditioner*>(pre.get())->native_callback(fn, ctx, 1) && fn == &gkomi_isai_apply_cb ? 1 : 0);
        // the defaults stay the triangular solvers
        auto plain = Ilu<>::build().with_factorization_factory(gko::factorization::Ilu<>::build().on(exec)).on(exec)->generate(A);
        std::printf("default_solvers %d\n", dynamic_cast<const gko::solver::LowerTrs<>*>(plain->get_l_solver().get()) && dynamic_cast<const gko::solver::UpperTrs<>*>(plain->get_u_solver().get()) ? 1 : 0);
        applies(exec, pre.get(), v);
        const gko::size_type n = A->get_size()[0];
        std::vector<double> rhs(n);
        for (gko::size_type i = 0; i < n; ++i) rhs[i] = 1.0 + 0.01 * static_cast<double>(i % 7);
        auto b = vec(exec, rhs);
        for (int generic = 0; generic < 2; ++generic) {
            std::shared_ptr<const gko::LinOp> p = generic ? std::make_shared<hidden>(pre) : pre;
            auto x = dense::create(exec, b->get_size());
            x->fill(0.0);
            long iters = 0;
            if (kind == "ilu") {
                auto f = gko::solver::Gmres<double>::build();
                f.with_krylov_dim(30u).with_criteria(gko::stop::Iteration::build().with_max_iters(17u).on(exec));
                auto s = f.with_generated_preconditioner(p).on(exec)->generate(A);
                s->apply(b.get(), x.get());
                iters = static_cast<long>(s->get_last_iteration_count());
            } else {
                auto s = gko::solver::Cg<double>::build().with_criteria(gko::stop::Iteration::build().with_max_iters(17u).on(exec)).with_generated_preconditioner(p).on(exec)->generate(A);
                s->apply(b.get(), x.get());
                iters = static_cast<long>(s->get_last_iteration_count());
            }
            std::printf("iterations %ld\n", iters);
            put(generic ? "generic_x" : "native_x", x.get());
        }
        return 0;
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
"""

PKG = os.path.join(os.path.dirname(HERE), "repo-8852-ginkgo_amd")


@functools.lru_cache(maxsize=None)
def mirror_program():
    import subprocess
    import tempfile
    d = tempfile.mkdtemp(prefix="isai_mirror_")
    src, exe = os.path.join(d, "mirror.cpp"), os.path.join(d, "mirror")
    open(src, "w").write(MIRROR_SRC)
    r = subprocess.run(["g++", "-O1", "-std=c++17", f"-I{PKG}/include", src, "-o", exe, f"-L{PKG}/lib", "-lgkomi", f"-Wl,-rpath,{PKG}/lib"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def write_mtx(path, m, ncols=None):
    rp, ci, v = m
    n = len(rp) - 1
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write(f"{n} {ncols or n} {len(ci)}\n")
        for r in range(n):
            for z in range(rp[r], rp[r + 1]):
                f.write(f"{r + 1} {int(ci[z]) + 1} {float(v[z])!r}\n")


def run_mirror(tmp_path, kind, power, m, vec=(), ncols=None):
    import subprocess
    path = os.path.join(str(tmp_path), "A.mtx")
    write_mtx(path, m, ncols)
    run = subprocess.run([mirror_program(), kind, str(power), path, *[repr(float(x)) for x in vec]], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    out = {}
    for ln in run.stdout.splitlines():
        t = ln.split()
        if t and ":" in "".join(t[1:2]):
            n = len(m[0]) - 1
            a = np.zeros((n, n))
            for e in t[1:]:
                r, c, x = e.split(":")
                a[int(r), int(c)] = float.fromhex(x)
            out[t[0]] = (a, sorted((int(e.split(":")[0]), int(e.split(":")[1])) for e in t[1:]))
        elif t and t[0] in ("apply", "advanced", "native_x", "generic_x"):
            out[t[0]] = np.array([float.fromhex(x) for x in t[1:]])
        elif t:
            out.setdefault(t[0], []).append(t[1] if len(t) > 1 else "")
    return out


def fixture_matrix(name):
    m = G["matrices"][name]
    if "dense" in m:
        return xu.dense_to_csr(np.array(m["dense"], np.float64))
    return np.array(m["row_ptrs"], np.int32), np.array(m["col_idxs"], np.int32), np.array(m["vals"], np.float64)


def pattern_of(m):
    return sorted((r, int(c)) for r in range(len(m[0]) - 1) for c in m[1][m[0][r]:m[0][r + 1]])


def near_dense(got, want, tol):
    return np.linalg.norm(got - want) <= tol * np.linalg.norm(want)


@pytest.mark.parametrize("c", [c for c in G["generate"] if "Longrow" not in c["test"]], ids=lambda c: c["test"])
def test_mirror_returns_the_reference_s_inverses(tmp_path, c):
    """ReturnsCorrectInverse{A,L,U,Spd}, the sparsity powers, GeneratesWithUnsortedCsr, and the transposed and conjugate
    transposed cases of the reference's tests"""
    want = fixture_matrix(c["expect"])
    out = run_mirror(tmp_path, c["kind"], c.get("sparsity_power", 1), fixture_matrix(c["matrix"]))
    dense_want = xu.csr_to_dense(want)
    for key in ("inverse", "transposed", "conj_transposed"):
        assert out[key][1] == pattern_of(want), key
        assert near_dense(out[key][0], dense_want, c["tol_r"] * R_DOUBLE), key
    if c["kind"] == "spd":
        assert near_dense(out["inverse_t"][0], dense_want.T, c["tol_r"] * R_DOUBLE)
    assert out["native"] == ["1"]


def test_mirror_equals_the_python_layer_on_long_rows(gk, tmp_path):
    """the mirror drives the same kernels: isai_l (rows of 33) bit for bit"""
    m = golden("isai_l.mtx")
    out = run_mirror(tmp_path, "lower", 1, m)
    got = h3(solvers.isai_generate(gk, "lower", len(m[0]) - 1, *d3(m)))
    assert out["inverse"][1] == pattern_of(got)
    assert xu.bits_equal(out["inverse"][0], xu.csr_to_dense(got))
    assert near_dense(out["inverse"][0], xu.csr_to_dense(golden("isai_l_inv.mtx")), R_DOUBLE)


@pytest.mark.parametrize("c", [c for c in G["apply"] if "alpha" not in c], ids=lambda c: c["test"])
def test_mirror_applies_like_the_reference(tmp_path, c):
    out = run_mirror(tmp_path, c["kind"], 1, fixture_matrix(c["matrix"]), vec=c["vec"])
    advanced = next(a for a in G["apply"] if "alpha" in a and a["kind"] == c["kind"])
    assert near_dense(out["apply"], np.array(c["expect"], np.float64), R_DOUBLE)
    assert near_dense(out["advanced"], np.array(advanced["expect"], np.float64), R_DOUBLE)


def test_mirror_refuses_a_non_square_matrix(tmp_path):
    m = (np.array([0, 1, 2], np.int32), np.array([0, 2], np.int32), np.array([1.0, 1.0]))
    assert run_mirror(tmp_path, "non_square", 1, m, ncols=3)["refused"] == ["DimensionMismatch"]


def test_mirror_ilu_over_isai_like_the_reference(tmp_path):
    """UseWithIluPreconditioner: Ilu over LowerIsai / UpperIsai on L U; the native callback is the two-SpMV record, the
    defaults stay the triangular solvers"""
    c = G["ilu"]
    a = np.array(G["matrices"][c["l"]]["dense"], np.float64) @ np.array(G["matrices"][c["u"]]["dense"], np.float64)
    out = run_mirror(tmp_path, "ilu", 1, xu.dense_to_csr(a), vec=c["vec"])
    assert out["solvers"] == ["1"] and out["native"] == ["1"] and out["default_solvers"] == ["1"]
    assert near_dense(out["apply"], np.array(c["expect"], np.float64), R_DOUBLE)


@pytest.mark.parametrize("kind,matrix", [("ilu", "ani4.mtx"), ("ic", "1138_bus.mtx")])
def test_mirror_native_and_generic_callbacks_give_identical_iterates(tmp_path, kind, matrix):
    out = run_mirror(tmp_path, kind, 2 if kind == "ilu" else 1, iu.golden_mtx(matrix))
    assert out["solvers"] == ["1"] and out["native"] == ["1"]
    assert out["iterations"] == ["17", "17"]
    assert np.isfinite(out["native_x"]).all() and xu.bits_equal(out["native_x"], out["generic_x"])


def test_mirror_example(tmp_path):
    import subprocess
    ex = os.path.join(PKG, "examples")
    r = subprocess.run(["make", "-C", ex, "bin/isai_preconditioned_solver"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(ex, "bin", "isai_preconditioned_solver"), os.path.join(HERE, "golden", "ani4.mtx"), "2"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    checks = [ln.split(": ") for ln in r.stdout.splitlines() if ln.startswith("check ")]
    assert len(checks) == 4 and all(c[1] == "ok" for c in checks), r.stdout
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("isai_preconditioned_solver:")]
    kv = dict(t.split("=") for t in line[0].split()[1:])
    L, U = iu.ilu0_factors("ani4.mtx")
    assert int(kv["rows"]) == len(L[0]) - 1 and int(kv["power"]) == 2
    # the pattern of the squares of the factors
    assert int(kv["l_inv_nnz"]) == len(su.spgemm(L, L)[1]) and int(kv["u_inv_nnz"]) == len(su.spgemm(U, U)[1])
    assert 0 < int(kv["isai_iterations"]) < int(kv["plain_iterations"])


def test_shims_run_on_the_device(tmp_path):
    import subprocess
    from test_isai_reference import build_isai_shim_smoke
    run = subprocess.run([build_isai_shim_smoke(tmp_path)], capture_output=True, text=True)
    ran = {t[1]: t[2] for t in (ln.split() for ln in run.stdout.splitlines()) if len(t) == 3 and t[0] == "ran"}
    assert run.returncode == 0, run.stdout + run.stderr
    assert ran == {"isai::" + k: "ok" for k in ("generate_tri_inverse", "generate_general_inverse", "generate_excess_system",
                                                "scale_excess_solution", "scatter_excess_solution")}, ran
