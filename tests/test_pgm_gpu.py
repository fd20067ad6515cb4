"""multigrid::Pgm on the device: every kernel entry point and gkomi_pgm_generate_f64_i32 against the sequential numpy
restatement (tests/pgm_util.py) and the reference executor's recorded results (tests/golden/pgm_ref.json), the known
answers of the reference's tests (tests/golden/pgm.json), and whole gkomi.solvers.Multigrid applies over a Pgm
hierarchy.  Integers must be equal and doubles equal bit for bit."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import gkomi
import matgen
import multigrid_util as mu
import pgm_util as pu
from gkomi import formats, solvers
from gpu_util import dev, host, stream_ptr, sync

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REF = json.load(open(os.path.join(HERE, "golden", "pgm_ref.json")))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "pgm.json")))
MG_GOLDEN = json.load(open(os.path.join(HERE, "golden", "multigrid.json")))
SPLIT = 4


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def i32(a):
    return dev(np.ascontiguousarray(a, np.int32))


def f64(a):
    return dev(np.ascontiguousarray(a, np.float64))


def scratch(nbytes):
    return torch.zeros(max(int(nbytes), 8), dtype=torch.uint8, device="cuda:0")


class DeviceW:
    """a weight matrix and its diagonal on the device"""

    def __init__(self, w, diag):
        self.n, self.nnz = w[0], len(w[3])
        self.rp, self.ci, self.v, self.d = i32(w[2]), i32(w[3]), f64(w[4]), f64(diag)


def find(gk, w, agg, strongest, counter):
    gk.pgm_find_strongest_neighbor_f64_i32(stream_ptr(), w.n, w.nnz, w.rp, w.ci, w.v, w.d, agg, strongest, counter, 4)


def count_unagg(gk, agg):
    out = ctypes.c_int64(-1)
    gk.pgm_count_unagg_i32(stream_ptr(), agg.numel(), agg, ctypes.addressof(out), scratch(4), 4)
    return out.value


def assign(gk, w, agg, deterministic):
    nb = gk.pgm_assign_workspace_bytes(w.n)
    mid = torch.full((w.n,), -5, dtype=torch.int32, device="cuda:0") if deterministic else None
    gk.pgm_assign_to_exist_agg_f64_i32(stream_ptr(), w.n, w.nnz, w.rp, w.ci, w.v, w.d, agg, mid, scratch(nb), nb)


def renumber(gk, agg):
    out = ctypes.c_int64(-1)
    nb = gk.pgm_renumber_workspace_bytes(agg.numel())
    gk.pgm_renumber_i32(stream_ptr(), agg.numel(), agg, ctypes.addressof(out), scratch(nb), nb)
    return out.value


# ---- known answers of the reference's tests ----------------------------------------------------------------------

def golden_w():
    g = GOLDEN["weight"]
    return DeviceW(mu.csr(5, 5, g["row_ptrs"], g["col_idxs"], g["vals"]), [5.0] * 5)


def test_kernel_known_answers(gk):
    k = GOLDEN["MatchEdge"]
    agg = i32(k["agg"])
    gk.pgm_match_edge_i32(stream_ptr(), 5, i32(k["strongest_neighbor"]), agg)
    assert host(agg).tolist() == k["agg_after"]
    assert count_unagg(gk, i32(GOLDEN["CountUnagg"]["agg"])) == GOLDEN["CountUnagg"]["num_unagg"]
    k = GOLDEN["Renumber"]
    agg = i32(k["agg"])
    assert renumber(gk, agg) == k["num_agg"] and host(agg).tolist() == k["agg_after"]
    k = GOLDEN["FindStrongestNeighbor"]
    agg, strongest, counter = i32(k["agg"]), i32([-1] * 5), i32([0])
    find(gk, golden_w(), agg, strongest, counter)
    assert host(strongest).tolist() == k["strongest_neighbor"] and host(agg).tolist() == k["agg"] and host(counter).tolist() == [0]
    k = GOLDEN["AssignToExistAgg"]
    for det in (False, True):
        agg = i32(k["agg"])
        assign(gk, golden_w(), agg, det)
        assert host(agg).tolist() == k["agg_after"]


def device_generate(gk, m, strategy=SPLIT, **kw):
    return solvers.pgm(gk, m[0], i32(m[2]), i32(m[3]), f64(m[4]), strategy=strategy, **kw)


def test_generate_known_answers_and_the_level_as_an_operator(gk):
    f, v = GOLDEN["factory"], GOLDEN["vectors"]
    g = GOLDEN["matrix"]
    m = mu.csr(5, 5, g["row_ptrs"], g["col_idxs"], g["vals"])
    lvl = device_generate(gk, m, max_iterations=f["max_iterations"], max_unassigned_ratio=f["max_unassigned_ratio"],
                          skip_sorting=f["skip_sorting"])
    assert host(lvl.agg).tolist() == GOLDEN["agg"]["agg"] and lvl.num_agg == 2
    r, c, p = lvl.get_restrict_op(), lvl.get_coarse_op(), lvl.get_prolong_op()
    assert host(r.row_ptrs).tolist() == GOLDEN["GenerateMgLevel"]["restrict"]["row_ptrs"]
    assert host(r.col_idxs).tolist() == GOLDEN["GenerateMgLevel"]["restrict"]["col_idxs"]
    assert host(p.col_idxs).tolist() == GOLDEN["GenerateMgLevel"]["prolong_row_gather"]
    assert host(c.row_ptrs).tolist() == GOLDEN["coarse"]["row_ptrs"] and host(c.col_idxs).tolist() == GOLDEN["coarse"]["col_idxs"]
    assert same_bits(host(c.vals), GOLDEN["coarse"]["vals"])
    assert (r.nrows, r.ncols, p.nrows, p.ncols, c.nrows, c.ncols) == (2, 5, 5, 2, 2, 2)
    arr = lambda t: f64(np.array(t, np.float64))
    one = f64([1.0])
    x = torch.zeros((2, 2), dtype=torch.float64, device="cuda:0")
    r.apply(arr(v["fine_b"]), x)
    assert same_bits(host(x), v["restrict_ans"])
    x = arr(v["fine_x"])
    p.apply(arr(v["coarse_b"]), x, one, one)
    assert same_bits(host(x), v["prolong_ans"])
    p.apply(arr(v["coarse_b"]), x)
    assert same_bits(host(x), v["prolong_applyans"])
    x = arr(v["fine_x"])
    lvl.apply(arr(v["fine_x"]), x)
    assert same_bits(host(x), GOLDEN["Apply"]["answer"])
    x = arr(v["fine_x"])
    a = GOLDEN["AdvancedApply"]
    lvl.apply(arr(v["fine_x"]), x, f64([a["alpha"]]), f64([a["beta"]]))
    assert same_bits(host(x), a["answer"])
    u = GOLDEN["GenerateMgLevelOnUnsortedMatrix"]
    lvl = device_generate(gk, mu.csr(5, 5, u["row_ptrs"], u["col_idxs"], u["vals"]), max_iterations=u["max_iterations"],
                          max_unassigned_ratio=u["max_unassigned_ratio"])
    assert host(lvl.agg).tolist() == u["prolong_row_gather"] and same_bits(host(lvl.get_coarse_op().vals), GOLDEN["coarse"]["vals"])
    # (the reference's unsorted matrix stores 5 and -3 of row 3 the other way round than its sorted one: same coarse sums)
    fine = mu.sort_by_column_index(mu.csr(5, 5, u["row_ptrs"], u["col_idxs"], u["vals"]))
    assert host(lvl.get_fine_op().col_idxs).tolist() == g["col_idxs"] and same_bits(host(lvl.get_fine_op().vals), fine[4])


# ---- kernel by kernel ---------------------------------------------------------------------------------------------

KERNEL_CASES = ["reference_5x5", "n1", "diagonal_300", "blocks_2x2", "grid5_17x19", "grid5_17x19_it0", "path_301_it1",
                "random_300_sym", "random_300_unsym", "star_ring_200", "grid9_40x40", "1138_bus", "ani4", "random_300_w10",
                "random_300_w10_it1", "grid27_5x6x7", "random_280_w24_it1"]


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("name", KERNEL_CASES)
def test_generate_kernel_by_kernel(gk, name, deterministic):
    """Pgm::generate spelled out with one entry point per reference kernel, each step compared with the sequential
    restatement's state at the same point"""
    kw = dict(dict(max_iterations=15, max_unassigned_ratio=0.05), **pu.CASES[name][1])
    fine = pu.case_matrix(name) if kw.get("skip_sorting") else mu.sort_by_column_index(pu.case_matrix(name))
    n, nnz = fine[0], len(fine[3])
    s = stream_ptr()
    # compute_absolute; W itself is csr::transpose and csr::spgeam, which have their own tests
    absv = torch.full((nnz,), -1.0, dtype=torch.float64, device="cuda:0")
    gk.csr_compute_absolute_f64_i32(s, nnz, f64(fine[4]), absv)
    assert same_bits(host(absv), np.abs(fine[4]))
    w_host = pu._W(*pu.weight_matrix(fine))
    w = DeviceW(*pu.weight_matrix(fine))
    agg_h, strongest_h = [-1] * n, [-1] * n
    agg, strongest, counter = i32(agg_h), i32(strongest_h), i32([0])
    left = n
    for _ in range(kw["max_iterations"]):
        absorbed = pu.find_strongest_neighbor(w_host, agg_h, strongest_h)
        counter.zero_()
        find(gk, w, agg, strongest, counter)
        assert host(agg).tolist() == agg_h and host(strongest).tolist() == strongest_h
        assert host(counter).tolist() == [absorbed]
        pu.match_edge(strongest_h, agg_h)
        gk.pgm_match_edge_i32(s, n, strongest, agg)
        assert host(agg).tolist() == agg_h
        prev, left = left, count_unagg(gk, agg)
        assert left == pu.count_unagg(agg_h)
        if left == 0 or left == prev or left < kw["max_unassigned_ratio"] * n:
            break
    if left:
        pu.assign_to_exist_agg(w_host, agg_h, deterministic)
        assign(gk, w, agg, deterministic)
        assert host(agg).tolist() == agg_h
    num_agg = pu.renumber(agg_h)
    assert renumber(gk, agg) == num_agg and host(agg).tolist() == agg_h
    want = pu.restated(name, deterministic)
    assert agg_h == want.agg.tolist() and num_agg == want.num_agg
    # the restriction: sort_agg on (agg[i], i), convert_idxs_to_ptrs
    rows, cols = agg.clone(), i32(np.arange(n))
    nb = gk.pgm_sort_workspace_bytes(max(n, nnz))
    ws = scratch(nb)
    gk.pgm_sort_agg_i32(s, n, rows, cols, ws, nb)
    rp = torch.zeros(num_agg + 1, dtype=torch.int32, device="cuda:0")
    pb = gk.prefix_sum_workspace_bytes(num_agg + 1)
    gk.convert_idxs_to_ptrs_i32(s, rows, n, num_agg, rp, scratch(pb), pb)
    assert host(cols).tolist() == want.restrict_col_idxs.tolist() and host(rp).tolist() == want.restrict_row_ptrs.tolist()
    # the coarse matrix: map_row, map_col, sort_row_major, count_unrepeated_nnz, compute_coarse_coo, convert_idxs_to_ptrs
    frp, fci = i32(fine[2]), i32(fine[3])
    rows = torch.full((nnz,), -3, dtype=torch.int32, device="cuda:0")
    cols = torch.full((nnz,), -3, dtype=torch.int32, device="cuda:0")
    vals = f64(fine[4])
    gk.pgm_map_row_i32(s, n, frp, agg, rows)
    gk.pgm_map_col_i32(s, nnz, fci, agg, cols)
    rows_h = [agg_h[r] for r in range(n) for _ in range(fine[2][r], fine[2][r + 1])]
    cols_h = [agg_h[c] for c in fine[3].tolist()]
    assert host(rows).tolist() == rows_h and host(cols).tolist() == cols_h
    gk.pgm_sort_row_major_f64_i32(s, nnz, rows, cols, vals, ws, nb)
    rows_h, cols_h, vals_h = pu.sort_row_major(rows_h, cols_h, fine[4].tolist())
    assert host(rows).tolist() == rows_h and host(cols).tolist() == cols_h and same_bits(host(vals), vals_h)
    cb = gk.pgm_coarse_coo_workspace_bytes(nnz)
    cws = scratch(cb)
    cnnz = ctypes.c_int64(-1)
    gk.pgm_count_unrepeated_nnz_i32(s, nnz, rows, cols, ctypes.addressof(cnnz), cws, cb)
    c_rows_h, c_cols_h, c_vals_h = pu.compute_coarse_coo(rows_h, cols_h, vals_h)
    assert cnnz.value == len(c_rows_h) == len(want.coarse[3])
    c_rows, c_cols = (torch.full((cnnz.value,), -3, dtype=torch.int32, device="cuda:0") for _ in range(2))
    c_vals = torch.full((cnnz.value,), -3.0, dtype=torch.float64, device="cuda:0")
    gk.pgm_compute_coarse_coo_f64_i32(s, nnz, rows, cols, vals, cnnz.value, c_rows, c_cols, c_vals, cws, cb)
    assert host(c_rows).tolist() == c_rows_h and host(c_cols).tolist() == c_cols_h and same_bits(host(c_vals), c_vals_h)
    assert same_bits(host(c_vals), want.coarse[4]) and c_cols_h == want.coarse[3].tolist()
    if cnnz.value > 1:      # a count that is not the number of runs is refused and nothing is written
        c_vals.fill_(-3.0)
        with pytest.raises(gkomi.GkomiError):
            gk.pgm_compute_coarse_coo_f64_i32(s, nnz, rows, cols, vals, cnnz.value - 1, c_rows, c_cols, c_vals, cws, cb)
        assert np.all(host(c_vals) == -3.0)


# ---- the native driver ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("name", list(pu.CASES))
def test_generate_matches_the_reference_executor(gk, name, deterministic):
    m = pu.case_matrix(name)
    kw = pu.CASES[name][1]
    rp, ci, v = i32(m[2]), i32(m[3]), f64(m[4])
    before = [host(t).copy() for t in (rp, ci, v)]
    lvl = solvers.pgm(gk, m[0], rp, ci, v, deterministic=deterministic, strategy=SPLIT, **kw)
    sync()
    want, rec = pu.restated(name, deterministic), REF[f"{name}/det{int(deterministic)}"]
    got = {"agg": host(lvl.agg), "num_agg": [lvl.num_agg], "restrict/row_ptrs": host(lvl.get_restrict_op().row_ptrs),
           "restrict/col_idxs": host(lvl.get_restrict_op().col_idxs), "fine/col_idxs": host(lvl.get_fine_op().col_idxs),
           "coarse/row_ptrs": host(lvl.get_coarse_op().row_ptrs), "coarse/col_idxs": host(lvl.get_coarse_op().col_idxs),
           "coarse/vals": host(lvl.get_coarse_op().vals)}
    assert set(got) == set(rec)
    for what, arr in got.items():
        assert pu.record_matches(rec[what], what, arr), (name, what)
    assert np.array_equal(got["agg"], want.agg) and same_bits(got["coarse/vals"], want.coarse[4])
    assert same_bits(host(lvl.get_fine_op().vals), want.fine[4])
    assert same_bits(host(lvl.get_restrict_op().vals), np.ones(m[0])) and same_bits(host(lvl.get_prolong_op().vals), np.ones(m[0]))
    assert np.array_equal(host(lvl.get_prolong_op().col_idxs), want.agg)
    assert np.array_equal(host(lvl.get_prolong_op().row_ptrs), np.arange(m[0] + 1))
    info = pu.restated(name, deterministic, parallel=True).info
    assert lvl.info["iterations"] == info["iterations"] and lvl.info["left"] == info["left"]
    assert lvl.info["exit"] == pu.EXITS[info["exit"]] == solvers.PGM_EXITS[info["exit"]]
    assert lvl.info["jump_rounds"] == (pu.jump_rounds(m[0]) if info["left"] and not deterministic else 0)
    # the inputs are not modified; with skip_sorting the caller's arrays are the fine operator
    assert all(np.array_equal(a, host(t)) for a, t in zip(before, (rp, ci, v)))
    if kw.get("skip_sorting"):
        assert lvl.get_fine_op().col_idxs.data_ptr() == ci.data_ptr() and lvl.get_fine_op().vals.data_ptr() == v.data_ptr()
    else:
        assert lvl.get_fine_op().col_idxs.data_ptr() != ci.data_ptr()
    # the same generate again: identical bytes
    again = solvers.pgm(gk, m[0], rp, ci, v, deterministic=deterministic, strategy=SPLIT, **kw)
    sync()
    for a, b in ((lvl.agg, again.agg), (lvl.get_coarse_op().vals, again.get_coarse_op().vals),
                 (lvl.get_coarse_op().col_idxs, again.get_coarse_op().col_idxs),
                 (lvl.get_restrict_op().col_idxs, again.get_restrict_op().col_idxs)):
        assert host(a).tobytes() == host(b).tobytes()


def test_the_modes_differ_where_the_restatement_says_so(gk):
    m = pu.case_matrix("grid5_17x19")
    a = device_generate(gk, m)
    b = device_generate(gk, m, deterministic=True)
    assert (a.num_agg, b.num_agg) == (pu.restated("grid5_17x19").num_agg, pu.restated("grid5_17x19", True).num_agg)
    assert a.num_agg != b.num_agg


# ---- whole solves -----------------------------------------------------------------------------------------------------

def device_parts(gk, pgm_kw):
    jac = lambda a: solvers.jacobi_generate(gk, a.nrows, a.row_ptrs, a.col_idxs, a.vals, max_block_size=1)
    direct = lambda a: solvers.Direct(gk, solvers.lu_generate(gk, a.nrows, a.row_ptrs, a.col_idxs, a.vals,
                                                              symmetric_sparsity=True))
    return pu.solve_parts(solvers.pgm_factory(gk, **pgm_kw), jacobi=jac, direct=direct,
                          cg=lambda a: solvers.OrderedCg(gk, a, mu.Cg.ITERATIONS))


def device_multigrid(gk, case, matrix):
    def make(m, **params):
        A = formats.Csr.from_host(gk, m[0], m[0], m[2], m[3], m[4], strategy=SPLIT)
        return solvers.Multigrid(gk, A, **params)
    return mu.restated(case, make=make, parts=device_parts(gk, case["pgm"]), matrix=matrix)


@pytest.mark.parametrize("name", list(pu.SOLVE_CASES))
def test_multigrid_over_pgm_matches_the_reference_executor(gk, name):
    c = pu.SOLVE_CASES[name]
    mg, b, x = device_multigrid(gk, c, pu.solve_matrix(c["matrix"]))
    out = mg.apply(dev(b), dev(x))
    sync()
    rec = REF[name]
    assert [lvl.get_coarse_op().nrows for lvl in mg.get_mg_level_list()] == rec["levels"]
    assert [out["iterations"]] == rec["iterations"]
    assert pu.record_matches(rec["x"], "x", host(out["x"])), name
    assert all(hasattr(lvl, "agg") for lvl in mg.get_mg_level_list())


def test_stencil_systems_are_solved_with_pgm(gk):
    """the device counterpart of tests/test_pgm_reference.py::test_stencil_systems_are_solved_with_pgm"""
    st = MG_GOLDEN["stencil_solves"]
    m = mu.csr(3, 3, *matgen.dense_to_csr(np.array(st["matrix_dense"], np.float64))[-3:])
    A = formats.Csr.from_host(gk, 3, 3, m[2], m[3], m[4], strategy=SPLIT)
    parts = device_parts(gk, pu.STENCIL_PGM)
    b = np.array(st["b"], np.float64).reshape(3, 1)
    for cycle in st["cycles"]:
        mg = solvers.Multigrid(gk, A, [parts["pgm"]], pre_smoother=[parts["jacobi"]], smoother_relax=1.0,
                               coarsest_solver=[parts["cg"]], max_levels=2, mid_case="both", cycle=cycle, min_coarse_rows=1,
                               max_iters=4, reduction=st["precision"], baseline="initial_resnorm")
        out = mg.apply(dev(b), dev(np.array(st["x0"], np.float64).reshape(3, 1)))
        sync()
        want = mu.Multigrid(m, [pu.pgm_level_factory(**pu.STENCIL_PGM)], pre_smoother=[lambda a: mu._PlainJacobi(a)],
                            smoother_relax=1.0, coarsest_solver=[mu.Cg], max_levels=2, mid_case="both", cycle=cycle,
                            min_coarse_rows=1, max_iters=4, reduction=st["precision"], baseline="initial_resnorm")
        x, it, _ = want.apply(b, np.array(st["x0"], np.float64).reshape(3, 1))
        err = float(np.max(np.abs(host(out["x"])[:, 0] - np.array(st["x"]))))
        print(cycle, out["iterations"], err)
        assert err <= st["precision"] * 3.0 and out["iterations"] == it and same_bits(host(out["x"]), x)


def restated_pcg(want_mg, m, b, max_iters, reduction):
    """the loop of multigrid_util.preconditioned_cg around a restated hierarchy -> (x, iterations)"""
    x, r, p = np.zeros_like(b), b.copy(), np.zeros_like(b)
    z, prev_rho, goal, it = np.zeros_like(b), np.ones(1), reduction * mu.norm2(b), 0
    while True:
        want_mg.apply(r, z)
        rho = mu.dot(r, z)
        if it >= max_iters or np.all(mu.norm2(r) <= goal):
            return x, it
        p = z + (rho / prev_rho) * p if it > 0 else z.copy()
        q = mu.spmv(m, p)
        alpha = rho / mu.dot(p, q)
        x, r, prev_rho, it = x + alpha * p, r - alpha * q, rho, it + 1


# Multigrid over Pgm as precond= of Cg: (matrix, Pgm's parameters, the rest of the case, Cg's iteration limit, the
# recorded solve case that has the same hierarchy).  On ani4 the Pgm V-cycle with two Jacobi sweeps is a poor
# preconditioner (profiles/pgm_probe.md), so Cg is stopped after 20 iterations there instead of being run to convergence.
PRECOND_CASES = {
    "ani4": ({}, dict(max_levels=3, iters=2), 20, "ani4/{}/pgm"),
    "stencil3": (pu.STENCIL_PGM, dict(max_levels=2, min_coarse_rows=1, mid_case="both", relax=1.0, iters=1), 500, "stencil3/{}/pgm"),
}


@pytest.mark.parametrize("cycle", list(mu.CYCLES))
@pytest.mark.parametrize("matrix", list(PRECOND_CASES))
def test_cg_preconditioned_by_a_pgm_cycle(gk, matrix, cycle):
    """Bit for bit: the preconditioner's own apply through the callback the drivers call (device pointers in, one cycle
    from a zero guess), against the restated Multigrid; and the level sizes, against the recorded ones.
    Looser than the issue's "x bit for bit", and why: the native Cg driver adds its dot products in a tree, the
    restatement (and the reference executor) in row order, so rho and alpha differ in their last bits from the first
    iteration on and x cannot be the same bits.  Each dot product of n terms is off by at most about n eps relative
    (3.4e-13 for ani4); Cg is allowed four orders of magnitude of growth of that over the run: x within 1e-8 relative.
    The residual norm at the last iteration can fall on either side of the threshold: the iteration count within one.
    (tests/test_multigrid_gpu.py holds FixedCoarsening's preconditioned Cg to 1e-4 for the same reason.)"""
    pgm_kw, rest, cg_iters, recorded = PRECOND_CASES[matrix]
    m = pu.solve_matrix(matrix)
    n = m[0]
    case = dict(mu._case(matrix=matrix, mg_level=["pgm"], cycle=cycle, guess="zero", max_iters=1, **rest), pgm=pgm_kw)
    mg, b, _ = device_multigrid(gk, case, m)
    want_mg, _, _ = mu.restated(case, parts=pu.solve_parts(pu.pgm_level_factory(**pgm_kw)), matrix=m)
    levels = [lvl.get_coarse_op().nrows for lvl in mg.get_mg_level_list()]
    assert levels == [lvl.coarse[0] for lvl in want_mg.mg_level_list]
    if recorded:
        assert levels == REF[recorded.format(cycle)]["levels"]
    bd = dev(b)
    z = torch.full((n, 1), 7.0, dtype=torch.float64, device="cuda:0")
    assert mg.callback()._keep(None, stream_ptr(), bd.data_ptr(), z.data_ptr()) == 0 and mg.callback().error is None
    sync()
    want_z, _, _ = want_mg.apply(b, np.full((n, 1), 7.0))
    assert same_bits(host(z), want_z)
    x, it = restated_pcg(want_mg, m, b, cg_iters, 1e-6)
    A = mg.matrix
    out = solvers.cg_solve(gk, n, A.row_ptrs, A.col_idxs, A.vals, dev(b[:, 0]), max_iters=cg_iters, reduction=1e-6, precond=mg)
    assert mg.callback().error is None
    print(f"cg + pgm {cycle}-cycle on {matrix}:", out["iterations"], "iterations, restatement", it,
          "rel. difference of x", matgen.rel_err(host(out["x"]), x[:, 0]))
    assert abs(out["iterations"] - it) <= 1 and bool(out["converged"]) == (it < cg_iters)
    assert matgen.rel_err(host(out["x"]), x[:, 0]) < 1e-8
