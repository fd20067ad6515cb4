"""multigrid::Pgm without a device: the sequential numpy restatement (tests/pgm_util.py) against what the reference
executor computed (tests/golden/pgm_ref.json, written by the verb pgm of oracle/ref_driver.cpp, which runs again
wherever it is, so the fixture cannot go stale) and against the known answers transcribed from the reference's own
tests (tests/golden/pgm.json); the parallel form the device kernels compute
against the sequential one, on every case and on seeded random matrices -- the order-independence argument, tested;
the conditions on the cases that keep the GPU tests from hiding a branch; the reference's stencil solves met by the
restated Multigrid over Pgm; and the C ABI's argument checks."""
import ctypes
import json
import os

import numpy as np
import pytest

import multigrid_util as mu
import pgm_util as pu
import ref_exec

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = json.load(open(os.path.join(HERE, "golden", "pgm_ref.json")))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "pgm.json")))
MG_GOLDEN = json.load(open(os.path.join(HERE, "golden", "multigrid.json")))


@pytest.fixture(scope="module")
def restated():
    return pu.restated_records()


def test_the_sequential_restatement_equals_the_reference_executor(restated):
    assert set(restated) == set(REF) - {"source"}
    for name, arrays in restated.items():
        assert set(arrays) == set(REF[name]), name
        for what, got in arrays.items():
            assert pu.record_matches(REF[name][what], what, got), (name, what)
    for name in pu.SOLVE_CASES:         # cycle counts and level sizes are exact
        assert REF[name]["iterations"] == [int(restated[name]["iterations"][0])]
        assert REF[name]["levels"] == [int(t) for t in restated[name]["levels"]]


def test_the_driver_reproduces_the_fixture():
    """oracle/_ref/ref_driver, the reference executor itself, gives the fixture as it is committed: every recorded array
    of every case, the keys compared both ways.  One driver process; a missing driver fails wherever the reference or
    oracle/_ref/ is."""
    if ref_exec.may_skip():
        pytest.skip("neither the reference nor oracle/_ref/ is on this machine")
    assert ref_exec.difference_from_driver("pgm", REF) is None


# ---- known answers transcribed from the reference's tests --------------------------------------------------------

def golden_csr(rec, n=5):
    return mu.csr(n, n, rec["row_ptrs"], rec["col_idxs"], rec["vals"])


def test_weight_matrix_and_generate_known_answers():
    m = golden_csr(GOLDEN["matrix"])
    w, diag = pu.weight_matrix(m)
    for got, want in zip(w[2:], golden_csr(GOLDEN["weight"])[2:]):
        assert np.array_equal(got, want)
    assert diag.tolist() == [5.0] * 5
    f = GOLDEN["factory"]
    for det in (False, True):
        lvl = pu.generate(m, f["max_iterations"], f["max_unassigned_ratio"], det, f["skip_sorting"])
        assert lvl.agg.tolist() == GOLDEN["agg"]["agg"] == GOLDEN["GenerateMgLevel"]["prolong_row_gather"]
        assert lvl.restrict_row_ptrs.tolist() == GOLDEN["GenerateMgLevel"]["restrict"]["row_ptrs"]
        assert lvl.restrict_col_idxs.tolist() == GOLDEN["GenerateMgLevel"]["restrict"]["col_idxs"]
        for got, want in zip(lvl.coarse[2:], golden_csr(GOLDEN["coarse"], 2)[2:]):
            assert np.array_equal(got, want)
        assert lvl.fine is m                                   # skip_sorting: the caller's matrix is the fine operator
    u = GOLDEN["GenerateMgLevelOnUnsortedMatrix"]
    lvl = pu.generate(golden_csr(u), u["max_iterations"], u["max_unassigned_ratio"])
    assert lvl.agg.tolist() == u["prolong_row_gather"]
    assert np.array_equal(lvl.coarse[4], GOLDEN["coarse"]["vals"]) and lvl.fine[3].tolist() == GOLDEN["matrix"]["col_idxs"]


def test_kernel_known_answers():
    w = pu._W(golden_csr(GOLDEN["weight"]), [5.0] * 5)
    k = GOLDEN["MatchEdge"]
    agg = list(k["agg"])
    pu.match_edge(k["strongest_neighbor"], agg)
    assert agg == k["agg_after"]
    assert pu.count_unagg(GOLDEN["CountUnagg"]["agg"]) == GOLDEN["CountUnagg"]["num_unagg"]
    k = GOLDEN["Renumber"]
    agg = list(k["agg"])
    assert pu.renumber(agg) == k["num_agg"] and agg == k["agg_after"]
    k = GOLDEN["FindStrongestNeighbor"]
    agg, strongest = list(k["agg"]), [-1] * 5
    assert pu.find_strongest_neighbor(w, agg, strongest) == 0 and strongest == k["strongest_neighbor"] and agg == k["agg"]
    k = GOLDEN["AssignToExistAgg"]
    for form in (pu.assign_to_exist_agg, pu.assign_to_exist_agg_parallel):
        for det in (False, True):
            agg = list(k["agg"])
            form(w, agg, det)
            assert agg == k["agg_after"]


def test_restrict_prolong_and_composition_known_answers():
    f, v = GOLDEN["factory"], GOLDEN["vectors"]
    lvl = pu.generate(golden_csr(GOLDEN["matrix"]), f["max_iterations"], f["max_unassigned_ratio"], False, True).level()
    arr = lambda t: np.array(t, np.float64)
    assert np.array_equal(mu.spmv(lvl.restrict, arr(v["fine_b"])), arr(v["restrict_ans"]))
    assert np.array_equal(mu.advanced_spmv(1.0, lvl.prolong, arr(v["coarse_b"]), 1.0, arr(v["fine_x"])), arr(v["prolong_ans"]))
    assert np.array_equal(mu.spmv(lvl.prolong, arr(v["coarse_b"])), arr(v["prolong_applyans"]))
    compose = lambda b: mu.spmv(lvl.coarse, mu.spmv(lvl.restrict, b))
    assert np.array_equal(mu.spmv(lvl.prolong, compose(arr(v["fine_x"]))), arr(GOLDEN["Apply"]["answer"]))
    a = GOLDEN["AdvancedApply"]
    got = mu.advanced_spmv(a["alpha"], lvl.prolong, compose(arr(v["fine_x"])), a["beta"], arr(v["fine_x"]))
    assert np.array_equal(got, arr(a["answer"]))


def test_every_reference_test_with_data_is_transcribed():
    names = [k for k in GOLDEN if k != "source"]
    assert all(GOLDEN[k]["source"].startswith("reference/test/multigrid/pgm_kernels.cpp:") for k in names)
    assert {"MatchEdge", "CountUnagg", "Renumber", "FindStrongestNeighbor", "AssignToExistAgg", "Apply", "AdvancedApply",
            "GenerateMgLevel", "GenerateMgLevelOnUnsortedMatrix"} <= set(names)


# ---- the parallel form equals the sequential one ------------------------------------------------------------------

def same_level(a, b):
    return (np.array_equal(a.agg, b.agg) and a.num_agg == b.num_agg and
            np.array_equal(a.restrict_row_ptrs, b.restrict_row_ptrs) and np.array_equal(a.restrict_col_idxs, b.restrict_col_idxs) and
            all(np.array_equal(s, t) for s, t in zip(a.coarse[2:], b.coarse[2:])) and
            all(a.info[k] == b.info[k] for k in ("iterations", "absorbed", "exit", "left")))


@pytest.mark.parametrize("name", list(pu.CASES))
def test_parallel_form_equals_sequential_form_on_every_case(name):
    for det in (False, True):
        assert same_level(pu.restated(name, det), pu.restated(name, det, parallel=True)), (name, det)


def test_parallel_form_equals_sequential_form_on_random_matrices():
    """240 seeded matrices, symmetric and unsymmetric patterns, sizes 1 to 60, 1 to 4 off-diagonals per row, iteration
    limits 0 to 3 (so that many rows reach assign_to_exist_agg) and the default, both modes"""
    seen_assign = seen_absorbed = 0
    for seed in range(240):
        rng = np.random.default_rng(1000 + seed)
        n, per_row = int(rng.integers(1, 61)), int(rng.integers(1, 5))
        m = pu.random_matrix(n, per_row, seed, symmetric=seed % 2 == 0)
        its = (0, 1, 2, 3, 15)[seed % 5]
        for det in (False, True):
            a = pu.generate(m, its, 0.05, det)
            b = pu.generate(m, its, 0.05, det, parallel=True)
            assert same_level(a, b), (seed, det)
        seen_assign += a.info["left"] > 0
        seen_absorbed += a.info["absorbed"] > 0
    assert seen_assign >= 100 and seen_absorbed >= 20


# ---- the cases reach every branch ------------------------------------------------------------------------------------

def test_the_cases_reach_every_branch():
    info = {name: pu.restated(name, parallel=True).info for name in pu.CASES}
    assert any(i["absorbed"] > 0 for i in info.values())                            # a row absorbed in find_strongest_neighbor
    d = pu.restated("diagonal_300")
    assert d.num_agg == 300 and d.info["left"] == 0                                 # rows with no neighbour
    left = [n for n, i in info.items() if i["left"] > 0]
    assert len(left) >= 8                                                           # rows left for assign_to_exist_agg
    assert any(not np.array_equal(pu.restated(n).agg, pu.restated(n, True).agg) for n in left)    # the modes differ
    assert info["grid5_17x19"] == dict(info["grid5_17x19"], iterations=15, left=131, chain_depth=18)
    assert info["path_301_it1"]["chain_depth"] == 297 and pu.jump_rounds(301) == 9  # more than 3 rounds of jumping
    assert {i["exit"] for i in info.values()} >= {0, 2, 3}                          # nothing left, ratio, max_iterations
    assert info["blocks_2x2"]["exit"] == 0 and info["random_300_sym"]["exit"] == 2 and info["random_300_sym"]["iterations"] == 4
    assert all(i["longest_run"] > 2 for n, i in info.items() if n.startswith(("grid", "ani4", "1138")))
    # decisions by the column tie-break: in a uniform stencil every weight of a row is the same
    w, _ = pu.weight_matrix(pu.case_matrix("grid5_17x19"))
    assert len(set(w[4][w[3] != np.repeat(np.arange(w[0]), np.diff(w[2]))].tolist())) == 1
    # every sub-wave width of find_strongest_neighbor and assign_to_exist_agg, each with rows left for the assign step
    # in a case whose two modes give different aggregates or in one that ends by the ratio
    widths = {name: pu.case_subwave_width(name) for name in pu.CASES}
    for width in (4, 8, 16, 64):
        assert any(w == width and info[n]["left"] > 0 for n, w in widths.items()), width
        assert any(w == width and info[n]["left"] > 20 and info[n]["chain_depth"] >= 4 for n, w in widths.items()), width
    assert (widths["random_300_w10"], widths["random_300_w10_it1"], widths["grid27_5x6x7"], widths["random_280_w24_it1"]) == (16, 16, 64, 64)
    hub = pu.case_matrix("star_ring_200")
    assert int(np.diff(hub[2]).max()) > 64                                          # the sub-wave loop
    assert int(np.diff(pu.case_matrix("grid9_40x40")[2]).sum()) > 2 * 2048          # several radix-sort tiles


def test_no_new_match_cannot_end_a_round_with_finite_weights():
    assert all(pu.restated(name, det).info["exit"] != 1 for name in pu.CASES for det in (False, True))


# ---- the reference's stencil solves, met with Pgm --------------------------------------------------------------------

def test_stencil_systems_are_solved_with_pgm():
    """SolvesStencilSystemBy{V,W,F}Cycle (reference/test/solver/multigrid_kernels.cpp:1315-1360): Pgm with max_iterations 2
    and max_unassigned_ratio 0.1 (:265-289), Jacobi smoother with relaxation 1, mid_case both, a Cg coarsest solver, four
    cycles or an initial_resnorm reduction of r<double>::value; x within that precision of the known answer.  The CPU
    counterpart of test_stencil_systems_need_pgm, which records what injection gives."""
    import matgen
    st = MG_GOLDEN["stencil_solves"]
    m = mu.csr(3, 3, *matgen.dense_to_csr(np.array(st["matrix_dense"], np.float64))[-3:])
    b = np.array(st["b"], np.float64).reshape(3, 1)
    for cycle in st["cycles"]:
        mg = mu.Multigrid(m, [pu.pgm_level_factory(**pu.STENCIL_PGM)], pre_smoother=[lambda a: mu._PlainJacobi(a)],
                          smoother_relax=1.0, coarsest_solver=[mu.Cg], max_levels=2, mid_case="both", cycle=cycle,
                          min_coarse_rows=1, max_iters=4, reduction=st["precision"], baseline="initial_resnorm")
        x, it, _ = mg.apply(b, np.array(st["x0"], np.float64).reshape(3, 1))
        err = float(np.max(np.abs(x[:, 0] - np.array(st["x"]))))
        print(cycle, it, err)
        assert err <= st["precision"] * max(1.0, float(np.max(np.abs(st["x"])))), (cycle, it, err)


# ---- the C ABI's argument checks: no device is touched -----------------------------------------------------------------

@pytest.fixture(scope="module")
def gk():
    import gkomi
    return gkomi.lib()


def code(fn, *args):
    from gkomi._lib import GkomiError
    try:
        return fn(*args)
    except GkomiError as e:
        return e.code


def test_abi_rejects_bad_arguments_before_any_hip_call(gk):
    # host addresses that are never touched
    A, B, C, D, W = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 64 << 20
    big = 1 << 24
    assert code(gk.csr_compute_absolute_f64_i32, None, -1, A, B) == -1
    assert code(gk.csr_compute_absolute_f64_i32, None, 4, None, B) == -1
    assert code(gk.csr_compute_absolute_f64_i32, None, 4, A, A + 8) == -1          # the output overlaps the input
    assert code(gk.csr_compute_absolute_f64_i32, None, 0, None, None) == 0
    assert code(gk.pgm_match_edge_i32, None, -1, A, B) == -1
    assert code(gk.pgm_match_edge_i32, None, 5, None, B) == -1 and code(gk.pgm_match_edge_i32, None, 5, A, A) == -1
    assert code(gk.pgm_match_edge_i32, None, 0, None, None) == 0
    n_out = ctypes.c_int64(-7)
    out = ctypes.addressof(n_out)
    assert code(gk.pgm_count_unagg_i32, None, -1, A, out, W, 4) == -1
    assert code(gk.pgm_count_unagg_i32, None, 5, A, None, W, 4) == -1
    assert code(gk.pgm_count_unagg_i32, None, 5, A, out, None, 4) == -1 and code(gk.pgm_count_unagg_i32, None, 5, A, out, W, 3) == -1
    assert code(gk.pgm_count_unagg_i32, None, 0, None, out, None, 0) == 0 and n_out.value == 0
    need = gk.pgm_renumber_workspace_bytes(300)
    assert need >= 4 * 301 and gk.pgm_renumber_workspace_bytes(0) == 0
    assert code(gk.pgm_renumber_i32, None, -1, A, out, W, need) == -1
    assert code(gk.pgm_renumber_i32, None, 300, None, out, W, need) == -1
    assert code(gk.pgm_renumber_i32, None, 300, A, out, W, need - 1) == -1
    assert code(gk.pgm_renumber_i32, None, 300, A, out, A + 64, need) == -1       # the workspace overlaps agg
    assert code(gk.pgm_renumber_i32, None, 0, None, out, None, 0) == 0
    need = gk.pgm_sort_workspace_bytes(100)
    assert need > 2 * 8 * 100 and gk.pgm_sort_workspace_bytes(0) == 0
    assert code(gk.pgm_sort_agg_i32, None, -1, A, B, W, need) == -1
    assert code(gk.pgm_sort_agg_i32, None, 100, A, A + 4, W, need) == -1 and code(gk.pgm_sort_agg_i32, None, 100, A, B, W, need - 1) == -1
    assert code(gk.pgm_sort_agg_i32, None, 0, None, None, None, 0) == 0
    assert code(gk.pgm_sort_row_major_f64_i32, None, 100, A, B, None, W, need) == -1
    assert code(gk.pgm_sort_row_major_f64_i32, None, 100, A, B, B + 8, W, need) == -1
    assert code(gk.pgm_sort_row_major_f64_i32, None, -2, A, B, C, W, need) == -1
    assert code(gk.pgm_sort_row_major_f64_i32, None, 0, None, None, None, None, 0) == 0
    assert code(gk.pgm_map_row_i32, None, -1, A, B, C) == -1 and code(gk.pgm_map_row_i32, None, 5, A, B, None) == -1
    assert code(gk.pgm_map_row_i32, None, 5, A, B, B) == -1 and code(gk.pgm_map_row_i32, None, 5, A, B, A + 8) == -1 and code(gk.pgm_map_row_i32, None, 0, None, None, None) == 0
    assert code(gk.pgm_map_col_i32, None, -1, A, B, C) == -1 and code(gk.pgm_map_col_i32, None, 5, A, B, A) == -1
    assert code(gk.pgm_map_col_i32, None, 0, None, None, None) == 0
    need = gk.pgm_coarse_coo_workspace_bytes(100)
    assert need >= 4 * 101 and gk.pgm_coarse_coo_workspace_bytes(0) == 0
    assert code(gk.pgm_count_unrepeated_nnz_i32, None, -1, A, B, out, W, need) == -1
    assert code(gk.pgm_count_unrepeated_nnz_i32, None, 100, A, None, out, W, need) == -1
    assert code(gk.pgm_count_unrepeated_nnz_i32, None, 100, A, B, out, W, need - 1) == -1
    assert code(gk.pgm_count_unrepeated_nnz_i32, None, 0, None, None, out, None, 0) == 0
    coo = lambda **kw: code(gk.pgm_compute_coarse_coo_f64_i32, None, *[dict(
        dict(nnz=100, r=A, c=B, v=C, cnnz=40, cr=D, cc=D + big, cv=D + 2 * big, ws=W, nb=need), **kw)[k]
        for k in ("nnz", "r", "c", "v", "cnnz", "cr", "cc", "cv", "ws", "nb")])
    assert coo(nnz=-1) == -1 and coo(cnnz=101) == -1 and coo(cnnz=-1) == -1 and coo(v=None) == -1 and coo(cv=None) == -1
    assert coo(cr=A) == -1 and coo(cc=D) == -1 and coo(ws=None) == -1 and coo(nb=need - 1) == -1 and coo(ws=C) == -1
    assert coo(nnz=0, cnnz=0) == 0
    find = lambda **kw: code(gk.pgm_find_strongest_neighbor_f64_i32, None, *[dict(
        dict(n=50, nnz=200, rp=A, ci=B, v=C, d=D, agg=D + big, sn=D + 2 * big, ws=W, nb=4), **kw)[k]
        for k in ("n", "nnz", "rp", "ci", "v", "d", "agg", "sn", "ws", "nb")])
    assert find(n=-1) == -1 and find(nnz=-1) == -1 and find(rp=None) == -1 and find(d=None) == -1 and find(ci=None) == -1
    assert find(sn=D + big) == -1 and find(ws=None) == -1 and find(nb=3) == -1 and find(ws=D + big) == -1
    assert find(agg=A) == -1 and find(sn=C + 8) == -1 and find(ws=D) == -1          # an output or the counter inside W or diag
    assert find(n=0) == 0
    need = gk.pgm_assign_workspace_bytes(50)
    assert need >= 3 * 4 * 50 and gk.pgm_assign_workspace_bytes(0) == 0
    assign = lambda **kw: code(gk.pgm_assign_to_exist_agg_f64_i32, None, *[dict(
        dict(n=50, nnz=200, rp=A, ci=B, v=C, d=D, agg=D + big, mid=None, ws=W, nb=need), **kw)[k]
        for k in ("n", "nnz", "rp", "ci", "v", "d", "agg", "mid", "ws", "nb")])
    assert assign(n=-1) == -1 and assign(nnz=-3) == -1 and assign(agg=None) == -1 and assign(v=None) == -1
    assert assign(mid=D + big + 8) == -1 and assign(ws=None) == -1 and assign(nb=need - 1) == -1 and assign(ws=D + big) == -1
    assert assign(agg=B + 4) == -1 and assign(mid=D) == -1 and assign(ws=C) == -1
    assert assign(n=0) == 0
    n, nnz = 300, 1500
    need = gk.pgm_generate_workspace_bytes(n, nnz)
    assert need > 12 * nnz + 2 * 12 * 2 * nnz and gk.pgm_generate_workspace_bytes(0, 0) == 0
    num_agg, cnnz = ctypes.c_int64(-1), ctypes.c_int64(-1)
    base = dict(n=n, nnz=nnz, rp=A, ci=B, v=C, it=15, ratio=0.05, det=0, skip=0, fci=D, fv=D + big, agg=D + 2 * big,
                rrp=D + 3 * big, rci=D + 4 * big, crp=D + 5 * big, cc=None, cv=None, na=ctypes.addressof(num_agg),
                cn=ctypes.addressof(cnnz), info=None, ws=W, nb=need)
    gen = lambda **kw: code(gk.pgm_generate_f64_i32, None, *[dict(base, **kw)[k] for k in base])
    assert gen(n=-1) == -1 and gen(nnz=-1) == -1 and gen(it=-1) == -1 and gen(na=None) == -1 and gen(cn=None) == -1
    assert gen(rp=None) == -1 and gen(ci=None) == -1 and gen(agg=None) == -1 and gen(rrp=None) == -1 and gen(crp=None) == -1
    assert gen(fci=None) == -1 and gen(cc=D + 6 * big) == -1                      # one of cc / cv alone
    assert gen(ws=None) == -1 and gen(nb=need - 1) == -1
    assert gen(agg=A) == -1 and gen(fv=C + 8) == -1 and gen(rci=D + 3 * big + 4) == -1 and gen(ws=B) == -1
    cnnz.value = nnz + 1
    assert gen(cc=D + 6 * big, cv=D + 7 * big) == -1                                 # a count the first call cannot have given
    assert gen(n=0) == 0 and num_agg.value == 0 and cnnz.value == 0


def test_python_layer_refuses_bad_parameters_before_touching_a_device(gk):
    from gkomi import solvers

    class Fake:
        def __init__(self, k):
            self.k = k

        def numel(self):
            return self.k
    with pytest.raises(ValueError):
        solvers.pgm(gk, 0, Fake(1), Fake(0), Fake(0))
    with pytest.raises(ValueError):
        solvers.pgm(gk, 5, Fake(6), Fake(15), Fake(15), max_iterations=-1)
    with pytest.raises(ValueError):
        solvers.pgm(gk, 5, Fake(6), Fake(15), Fake(15), max_unassigned_ratio=1.5)
    with pytest.raises(ValueError):
        solvers.pgm(gk, 5, Fake(5), Fake(15), Fake(15))
    assert callable(solvers.pgm_factory(gk, max_iterations=2))
