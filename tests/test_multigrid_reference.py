"""solver::Multigrid without a device: the numpy restatement (tests/multigrid_util.py) against what the reference
executor computed (tests/golden/multigrid_ref.json, written by the verb multigrid of oracle/ref_driver.cpp) and against
the data transcribed from the reference's own tests (tests/golden/multigrid.json); wherever that driver is, it runs
again and the fixture is compared with what it gives, so the fixture cannot go stale; the C ABI's argument
checks; and the conditions on the cases that keep the GPU tests from hiding a failure."""
import json
import os

import numpy as np
import pytest

import multigrid_util as mu
import ref_exec

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = json.load(open(os.path.join(HERE, "golden", "multigrid_ref.json")))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "multigrid.json")))


@pytest.fixture(scope="module")
def restated():
    return mu.restated_records()


def test_the_restatement_equals_the_reference_executor(restated):
    assert set(restated) == set(REF) - {"source"}
    for name, arrays in restated.items():
        assert set(arrays) == set(REF[name]), name
        for what, got in arrays.items():
            assert mu.record_matches(REF[name][what], what, got), (name, what)
    for name in mu.SOLVE_CASES:         # iteration counts are exact
        assert REF[name]["iterations"] == [int(restated[name]["iterations"][0])]


def test_preconditioned_cg_equals_the_reference_executor():
    """solver::Cg preconditioned by one V-cycle on 1138_bus, the yardstick of the GPU tests' Cg over Multigrid: the
    restatement's x and iteration count are the driver's, bit for bit"""
    if ref_exec.may_skip():
        pytest.skip("neither the reference nor oracle/_ref/ is on this machine")
    m = mu.case_matrix("1138_bus")
    arrays, params = mu.solve_arguments(mu.V_CYCLE_PRECONDITIONER, m)
    arrays["x"] = np.zeros(m[0])
    batch = ref_exec.Batch()
    batch.add("multigrid", arrays, op=3, cg_max_iters=500, cg_reduction=1e-6, **params)
    got = batch.run()[0]
    x, iterations = mu.preconditioned_cg(m, mu.right_hand_side(m[0]), 500, 1e-6)
    assert "error" not in got, got
    assert int(got["iterations"][0]) == iterations
    ref_exec.assert_bits(got["x"], x.reshape(-1), "x")


def test_the_driver_reproduces_the_fixture():
    """oracle/_ref/ref_driver, the reference executor itself, gives the fixture as it is committed: every recorded array
    of every case, the keys compared both ways.  One driver process; a missing driver fails wherever the reference or
    oracle/_ref/ is."""
    if ref_exec.may_skip():
        pytest.skip("neither the reference nor oracle/_ref/ is on this machine")
    assert ref_exec.difference_from_driver("multigrid", REF) is None


# ---- data transcribed from the reference's tests ---------------------------------------------------------------

@pytest.mark.parametrize("name", list(GOLDEN["cycles"]))
def test_cycle_call_sequences(name):
    rec = GOLDEN["cycles"][name]
    assert mu.steps_match(mu.cycle_steps(mu.Multigrid, rec), rec)


def test_sixteen_cycle_tests_are_transcribed():
    names = list(GOLDEN["cycles"])
    assert len(names) == 16 and names[0] == "VCycleIndividual" and names[-1] == "FCycleSameMidUsePre"
    assert {GOLDEN["cycles"][n]["cycle"] for n in names} == {"v", "w", "f"}
    assert all(GOLDEN["cycles"][n]["source"].startswith("reference/test/solver/multigrid_kernels.cpp:") for n in names)


def dense_of(m):
    a = np.zeros((m[0], m[1]))
    for r in range(m[0]):
        for k in range(m[2][r], m[2][r + 1]):
            a[r, m[3][k]] += m[4][k]
    return a


def test_fixed_coarsening_known_answers():
    import matgen
    fc = GOLDEN["fixed_coarsening"]
    tol = fc["precision"]
    near = lambda got, want: np.allclose(got, np.array(want, np.float64), rtol=tol, atol=0.0)
    fine = np.array(fc["fine_dense"], np.float64)
    u, coo = fc["unsorted_csr"], fc["unsorted_coo"]
    order = np.argsort(coo["row_idxs"], kind="stable")      # Coo -> Csr keeps the stored order inside a row
    from_coo = mu.csr(5, 5, np.searchsorted(np.array(coo["row_idxs"])[order], np.arange(6)),
                      np.array(coo["col_idxs"])[order], np.array(coo["vals"], np.float64)[order])
    prolong = np.zeros((5, 3))
    for r, c, val in fc["prolong_entries"]:
        prolong[r, c] = val
    for m in (mu.csr(5, 5, *matgen.dense_to_csr(fine)[-3:]), mu.csr(5, 5, u["row_ptrs"], u["col_idxs"], u["vals"]), from_coo):
        lvl = mu.fixed_coarsening(m, fc["coarse_rows"])
        assert near(dense_of(lvl.coarse), fc["coarse_dense"]) and near(dense_of(lvl.fine), fine)
        assert near(dense_of(lvl.prolong), prolong) and near(dense_of(lvl.restrict), prolong.T)
        assert np.all(np.diff(lvl.fine[3][lvl.fine[2][1]:lvl.fine[2][2]]) > 0)       # sorted unless skipped
    assert near(mu.spmv(lvl.restrict, np.array(fc["fine_b"], np.float64)), fc["CoarseFineRestrictApply"]["answer"])
    assert near(mu.spmv(lvl.prolong, np.array(fc["coarse_b"], np.float64)), fc["CoarseFineProlongApply"]["answer"])
    x = np.array(fc["fine_x"], np.float64)
    # the level as a LinOp: prolong(coarse(restrict(b)))
    inner = mu.spmv(lvl.coarse, mu.spmv(lvl.restrict, x))
    assert near(mu.spmv(lvl.prolong, inner), fc["Apply"]["answer"])
    a = fc["AdvancedApply"]
    assert near(mu.advanced_spmv(a["alpha"], lvl.prolong, inner, a["beta"], x.copy()), a["answer"])
    kept = mu.fixed_coarsening(mu.unsorted_5x5(), fc["coarse_rows"], skip_sorting=True)
    assert list(kept.fine[3]) == u["col_idxs"]


def test_zero_guess_ignores_input():
    import matgen
    z = GOLDEN["zero_guess_ignores_input"]
    m = mu.csr(3, 3, *matgen.dense_to_csr(np.array(z["matrix_dense"], np.float64))[-3:])
    common = dict(mg_level=[lambda a: mu.fixed_coarsening(a, [0, 2])], pre_smoother=[lambda a: mu._PlainJacobi(a)],
                  coarsest_solver=[mu.Direct], max_levels=1, min_coarse_rows=1, max_iters=1)
    b = np.array(z["b"], np.float64).reshape(3, 1)
    zero, x = np.zeros((3, 1)), np.array(z["x"], np.float64).reshape(3, 1)
    mu.Multigrid(m, default_initial_guess="provided", **common).apply(b, zero)
    mu.Multigrid(m, default_initial_guess="zero", **common).apply(b, x)
    assert np.allclose(zero, x, rtol=z["precision"], atol=0.0) and np.any(x != 0.0)


# ---- conditions on the cases -----------------------------------------------------------------------------------

def test_no_residual_norm_check_is_close_to_its_threshold():
    """a ResidualNorm case whose norm came within a relative 1e-6 of the threshold at some check could legitimately
    stop one cycle earlier or later on the device; the cases are chosen so that none does"""
    checked = 0
    for name, c in mu.SOLVE_CASES.items():
        if c["reduction"] is None:
            continue
        mg, b, x = mu.restated(name)
        _, it, seen = mg.apply(b, x)
        assert 0 < it < c["max_iters"] and len(seen) == it + 1, name
        for res, base in seen:
            assert np.all(np.abs(res / (c["reduction"] * base) - 1.0) > 1e-6), (name, res, base)
        checked += 1
    assert checked >= 3


def test_the_cases_cover_what_they_must():
    cases = mu.SOLVE_CASES.values()
    assert {c["cycle"] for c in cases} == set(mu.CYCLES)
    assert {c["mid_case"] for c in cases} == set(mu.MID_CASES)
    assert any(not c["post_uses_pre"] for c in cases)
    assert any(None in c["pre"] for c in cases)
    assert any(len(c["mg_level"]) == 1 and REF[n]["levels"] and len(REF[n]["levels"]) > 1 for n, c in mu.SOLVE_CASES.items())
    assert {c["coarsest"] for c in cases} == {"identity", "direct", "cg"}
    ends = {mu.restated(n)[0].stopped_by for n in ("ani4/v/direct", "ani1/v/min_coarse_rows", "ani1/v/no_reduction")}
    assert ends == {"max_levels", "min_coarse_rows", "no_reduction"}
    assert any(c["reduction"] is not None for c in cases) and any(c["guess"] == "provided" for c in cases)


def test_the_wrapped_jacobi_is_the_jacobi_smoother():
    """build_smoother around a scalar Jacobi (the general path) and the sweep the fused kernel restates: the same bits"""
    m = mu.case_matrix("ani1")
    b, x0 = mu.right_hand_side(36, 2), mu.initial_guess(36, 2)
    for zero in (False, True):
        one = mu._Wrapped(m, mu._PlainJacobi(m), 3, 0.9).apply(b, x0.copy(), zero=zero)
        two = mu.JacobiSmoother(m, 3, 0.9).apply(b, x0.copy(), zero=zero)
        assert np.array_equal(one.view(np.int64), two.view(np.int64))


def test_validate():
    m = mu.case_matrix("ani1")
    s = lambda a: mu._Recording()
    with pytest.raises(ValueError):
        mu.Multigrid(m, [])
    with pytest.raises(ValueError):
        mu.Multigrid(m, [mu.every_second, None])
    with pytest.raises(ValueError):
        mu.Multigrid(m, [mu.every_second] * 3, pre_smoother=[s, s])
    with pytest.raises(ValueError):
        mu.Multigrid(m, [mu.every_second] * 3, post_uses_pre=False, post_smoother=[s, s])
    with pytest.raises(ValueError):
        mu.Multigrid(m, [mu.every_second] * 3, mid_smoother=[s, s])
    mu.Multigrid(m, [mu.every_second] * 3, mid_case="both", mid_smoother=[s, s], max_levels=3, min_coarse_rows=4)


# ---- the C ABI and the Python layer, without a device -------------------------------------------------------------

def code(fn, *args):
    import gkomi
    try:
        return fn(*args)
    except gkomi.GkomiError as e:
        return e.code


def test_abi_rejects_bad_arguments_before_any_hip_call(gk):
    s1, s2, sweeps = gk.multigrid_kcycle_step_1_f64, gk.multigrid_kcycle_step_2_f64, gk.multigrid_jacobi_sweeps_f64_i32
    assert code(s1, None, -1, 1, 8, 8, 8, 1, 8, 1, 8, 1, 8, 1) == -1
    assert code(s1, None, 4, -1, 8, 8, 8, 1, 8, 1, 8, 1, 8, 1) == -1
    assert code(s1, None, 4, 3, 8, 8, 8, 2, 8, 3, 8, 3, 8, 3) == -1           # a stride below nrhs
    assert code(s1, None, 4, 3, 8, 8, 8, 3, 8, 3, 8, 3, None, 3) == -1
    assert code(s1, None, 0, 3, None, None, None, 3, None, 3, None, 3, None, 3) == 0
    assert code(s2, None, 4, 3, 8, 8, 8, 8, 8, 8, 2, 8, 3) == -1
    assert code(s2, None, -4, 3, 8, 8, 8, 8, 8, 8, 3, 8, 3) == -1
    assert code(s2, None, 4, 0, None, None, None, None, None, None, 1, None, 1) == 0
    assert code(gk.multigrid_kcycle_check_stop_f64, None, 1, 8, 8, 0.25, None) == -1
    assert code(gk.multigrid_kcycle_check_stop_f64, None, -1, 8, 8, 0.25, 8) == -1
    # host addresses that are never touched: x at 4096, b at 8192, 64 rows
    need = gk.multigrid_jacobi_sweeps_workspace_bytes(64)
    assert need >= 512 and need % 8 == 0 and gk.multigrid_jacobi_sweeps_workspace_bytes(0) == 0
    ok = dict(n=64, nrhs=1, nnz=10, sweeps=1, ws=1 << 20, nbytes=need)

    def sweep(**kw):
        a = dict(ok, **kw)
        return code(sweeps, None, a["n"], a["nrhs"], a["nnz"], 8, 8, 8, 8, 0.9, 8192, 4096, a["sweeps"], 0, a["ws"], a["nbytes"])
    assert sweep(nrhs=2) == -1 and sweep(nrhs=0) == -1 and sweep(n=-1) == -1 and sweep(nnz=-2) == -1 and sweep(sweeps=-1) == -1
    assert sweep(ws=None) == -1 and sweep(nbytes=need - 1) == -1
    assert sweep(ws=4096) == -1 and sweep(ws=8192) == -1                       # the workspace is x, or b
    assert sweep(ws=4096 + 504) == -1 and sweep(ws=8192 - need + 8) == -1      # ... or overlaps one of them
    assert sweep(n=0) == 0


def test_python_layer_refuses_bad_parameters_before_touching_a_device(gk):
    from gkomi import solvers

    class NoMatrix:
        nrows = 100
    with pytest.raises(ValueError, match="mg_level"):
        solvers.Multigrid(gk, NoMatrix(), [])
    with pytest.raises(ValueError):
        solvers.Multigrid(gk, NoMatrix(), [lambda m: None], cycle="k")
    with pytest.raises(ValueError, match="pre_smoother"):
        solvers.Multigrid(gk, NoMatrix(), [lambda m: None] * 3, pre_smoother=[None, None])
    with pytest.raises(ValueError, match="no level"):
        solvers.Multigrid(gk, NoMatrix(), [lambda m: None], min_coarse_rows=100)


def test_fused_dispatch_rule(monkeypatch):
    """explicit choice, then GKOMI_MG_FUSED, then the size rule"""
    from gkomi import solvers
    monkeypatch.delenv("GKOMI_MG_FUSED", raising=False)
    assert solvers._mg_fused(None, 1571840) and not solvers._mg_fused(None, 1571841)
    assert solvers._mg_fused(True, 10 ** 9) and not solvers._mg_fused(False, 1)
    monkeypatch.setenv("GKOMI_MG_FUSED", "0")
    assert not solvers._mg_fused(None, 1) and solvers._mg_fused(True, 1)
    monkeypatch.setenv("GKOMI_MG_FUSED", "1")
    assert solvers._mg_fused(None, 10 ** 9)


def test_python_callback_serves_one_column_only():
    """a Multigrid as precond= sees bare pointers: a solve with several right-hand sides is refused before any launch"""
    from gkomi import solvers
    cb = solvers._PythonCallback(lambda b, x: None, 10)
    solvers._check_precond(cb, 1)
    with pytest.raises(ValueError, match="nrhs"):
        solvers._check_precond(cb, 3)


def test_stencil_systems_need_pgm():
    """The reference's SolvesStencilSystemBy{V,W,F}Cycle coarsen with multigrid::Pgm, which the library does not have.
    With FixedCoarsening (injection) in its place -- same smoother, relaxation 1, mid_case both, four cycles, an exact
    coarsest solve -- x stays 0.09375 (rows 0 and 2 coarse) away from the known answer, far from that test's precision
    of 10 epsilon.  This test records that, so that the cases are visibly open until Pgm lands."""
    import matgen
    st = GOLDEN["stencil_solves"]
    m = mu.csr(3, 3, *matgen.dense_to_csr(np.array(st["matrix_dense"], np.float64))[-3:])
    b = np.array(st["b"], np.float64).reshape(3, 1)
    for cycle in st["cycles"]:
        mg = mu.Multigrid(m, [lambda a: mu.fixed_coarsening(a, [0, 2])], pre_smoother=[lambda a: mu._PlainJacobi(a)],
                          smoother_relax=1.0, coarsest_solver=[mu.Direct], max_levels=1, mid_case="both", cycle=cycle,
                          min_coarse_rows=1, max_iters=4, reduction=st["precision"], baseline="initial_resnorm")
        x, it, _ = mg.apply(b, np.zeros((3, 1)))
        err = float(np.max(np.abs(x[:, 0] - np.array(st["x"]))))
        assert it == 4 and st["precision"] < err == 0.09375, (cycle, it, err)
