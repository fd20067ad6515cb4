"""CPU side of ParILUT.  The plain-Python restatement (tests/par_ilut_util.py) is pinned to the reference twice: to
the answers the reference's own tests expect (tests/golden/par_ilut.json, the reference's tolerances) and, bit for bit,
to results recorded from the reference executor (tests/golden/par_ilut_ref.json, written by the verb par_ilut of
oracle/ref_driver.cpp).  Wherever that driver is, it runs again and the fixture is compared with what it gives, so the
fixture cannot go stale.  Then the C ABI's argument checks and the Python layer's, none
of which needs a device; the mirror example builds and the shim compiles against the mirror prelude and links with
shims/test/shim_smoke8.cpp."""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import ilu_exact_util as xu
import par_ilut_util as pu
import ref_exec

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "repo-8852-ginkgo_amd")
G = json.load(open(os.path.join(HERE, "golden", "par_ilut.json")))
REF = json.load(open(os.path.join(HERE, "golden", "par_ilut_ref.json")))
R_DOUBLE = 10 * np.finfo(np.float64).eps     # r<double>::value (core/test/utils.hpp:212-219)


def dense(a):
    """a matrix of the fixture, by name or as rows; [p, q] is the fraction p / q as the reference's test writes it"""
    a = G[a] if isinstance(a, str) else a
    return np.array([[x[0] / x[1] if isinstance(x, list) else x for x in row] for row in a], np.float64)


def csr(a):
    return pu.dense_to_csr(dense(a))


def near(got, want, tol):
    """GKO_ASSERT_MTX_NEAR: relative Frobenius norm of the difference"""
    want = dense(want)
    return np.linalg.norm(xu.csr_to_dense(got) - want) <= tol * np.linalg.norm(want)


def same_sparsity(got, want):
    """GKO_ASSERT_MTX_EQ_SPARSITY against gko::initialize<Csr> of the expected rows"""
    w = pu.dense_to_csr(dense(want))
    return np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1])


# ---- the reference's known answers --------------------------------------------------------------------------

@pytest.mark.parametrize("c", G["select"], ids=lambda c: c["test"])
def test_restatement_selects_the_reference_s_threshold(c):
    assert c["tolerance"] == 0 and pu.threshold_select(csr("mtx1"), c["rank"]) == c["expect"]


@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("c", G["filter"], ids=lambda c: c["test"])
def test_restatement_filters_like_the_reference(c, lower):
    m, want = csr("mtx1"), dense(c["expect"])
    if not lower:
        m, want = pu.transpose(m), want.T
    got, rows = pu.threshold_filter(m, c["threshold"], with_coo=True)
    assert same_sparsity(got, want) and near(got, want, 0)
    assert np.array_equal(rows, np.repeat(np.arange(4), np.diff(got[0])))


@pytest.mark.parametrize("c", G["filter_approx"], ids=lambda c: c["test"])
def test_restatement_filters_approximately_like_the_reference(c):
    threshold, got = pu.threshold_filter_approx(csr("mtx1"), c["rank"])
    assert same_sparsity(got, c["expect"]) and near(got, c["expect"], 0)
    again = pu.threshold_filter(csr("mtx1"), threshold)
    assert same_sparsity(again, c["expect"]) and near(again, c["expect"], 0)


def test_restatement_adds_the_reference_s_candidates():
    c = G["add_candidates"]
    l, u = pu.add_candidates(csr("mtx_lu"), csr("mtx_system"), csr("mtx_l"), csr("mtx_u"))
    assert same_sparsity(l, c["l_expect"]) and same_sparsity(u, c["u_expect"])
    assert near(l, c["l_expect"], R_DOUBLE) and near(u, c["u_expect"], R_DOUBLE)


def test_restatement_sweeps_like_the_reference():
    c = G["compute_lu"]
    u0 = csr("mtx_u_system")
    l, u, u_csc = pu.compute_l_u_factors(csr("mtx_system"), csr("mtx_l_system"), u0, pu.transpose(u0))
    assert near(l, c["l_expect"], R_DOUBLE) and near(u_csc, c["u_csc_expect"], R_DOUBLE)
    assert near(u, xu.csr_to_dense(pu.transpose(u_csc)), 0)


@pytest.mark.parametrize("c", G["generate"], ids=lambda c: c["test"])
def test_restatement_generates_the_reference_s_factors(c):
    l, u = pu.generate(csr(c["matrix"]), fill_in_limit=c.get("fill_in_limit", 2.0),
                       approximate_select=c.get("approximate_select", True))
    assert near(l, c["l_expect"], R_DOUBLE) and near(u, c["u_expect"], R_DOUBLE)


# ---- results recorded from the reference executor ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def recorded_case(name):
    m = pu.RECORDED_CASES[name]()
    for a in m:
        a.setflags(write=False)
    return m


matches = ref_exec.matches     # an array or a CSR matrix is the recorded one: the digest, and the items where kept


def test_the_fixture_describes_the_cases_of_the_restatement():
    assert sorted(REF["cases"]) == sorted(pu.RECORDED_CASES)
    for name, c in REF["cases"].items():
        m = recorded_case(name)
        assert (c["n"], c["nnz"]) == (len(m[0]) - 1, len(m[1])), name
    lacking = recorded_case("ani1_without_some_diagonals")
    assert sum(1 for r, row in enumerate(xu.to_rows(lacking)) if r not in row) == 8
    assert os.path.getsize(os.path.join(HERE, "golden", "par_ilut_ref.json")) < 100 * 1024


@pytest.mark.parametrize("name", sorted(pu.RECORDED_CASES))
def test_restatement_kernels_equal_the_recorded_ones_bit_for_bit(name):
    """each kernel alone on the intermediate matrices of the first iteration at fill_in_limit 1.2"""
    m, rec = recorded_case(name), REF["cases"][name]["records"]
    traces = []
    pu.generate(m, iterations=1, fill_in_limit=1.2, approximate_select=False, traces=traces)
    t = traces[0]
    assert matches(rec["kernels/lu"], t["lu"])
    assert matches(rec["kernels/add_candidates.l"], t["l_cand"]) and matches(rec["kernels/add_candidates.u"], t["u_cand"])
    assert matches(rec["kernels/sweep.l"], t["l_new"]) and matches(rec["kernels/sweep.u"], t["u_new"])
    assert matches(rec["kernels/sweep.u_csc"], t["u_new_csc"])
    assert matches(rec["kernels/ranks"], np.array([t["l_rank"], t["u_rank"]], np.int32))
    assert matches(rec["kernels/select"], np.array([t["l_threshold"], t["u_threshold"]]))
    l_filtered, rows = pu.threshold_filter(t["l_new"], t["l_threshold"], with_coo=True)
    assert matches(rec["kernels/filter.l"], l_filtered) and matches(rec["kernels/filter.l.row_idxs"], rows)
    assert matches(rec["kernels/filter.u"], t["u_filtered"])
    l_thr, l_approx = pu.threshold_filter_approx(t["l_new"], t["l_rank"])
    u_thr, ut_approx = pu.threshold_filter_approx(t["u_new_csc"], t["u_rank"])
    assert matches(rec["kernels/approx"], np.array([l_thr, u_thr]))
    assert matches(rec["kernels/filter_approx.l"], l_approx) and matches(rec["kernels/filter_approx.u_csc"], ut_approx)


@pytest.mark.parametrize("name", sorted(pu.RECORDED_CASES))
def test_restatement_generate_equals_the_recorded_factors_bit_for_bit(name):
    """exact and approximate selection, fill_in_limit 0.75 / 1.2 / 2.0: the entry counts after 1 ... 5 iterations, the
    factors after 1 and 5"""
    m, rec = recorded_case(name), REF["cases"][name]["records"]
    for select in ("exact", "approx"):
        for limit in pu.RECORDED_LIMITS:
            traces = []
            l, u = pu.generate(m, iterations=5, fill_in_limit=limit, approximate_select=select == "approx", traces=traces)
            key = f"generate/{select}/{limit:g}"
            assert [[t["l_nnz"], t["u_nnz"]] for t in traces] == rec[key + "/nnz"], key
            assert matches(rec[key + "/5/l"], l) and matches(rec[key + "/5/u"], u), key
            l1, u1 = pu.generate(m, iterations=1, fill_in_limit=limit, approximate_select=select == "approx")
            assert matches(rec[key + "/1/l"], l1) and matches(rec[key + "/1/u"], u1), key


def test_the_driver_reproduces_the_fixture():
    """oracle/_ref/ref_driver, the reference executor itself, gives the fixture as it is committed: every recorded array
    of every case, the keys compared both ways.  One driver process; a missing driver fails wherever the reference or
    oracle/_ref/ is."""
    if ref_exec.may_skip():
        pytest.skip("neither the reference nor oracle/_ref/ is on this machine")
    assert ref_exec.difference_from_driver("par_ilut", REF) is None


# ---- the mirror and the shims build ------------------------------------------------------------------------------

def test_mirror_example_builds():
    ex = os.path.join(PKG, "examples")
    r = subprocess.run(["make", "-C", ex, "bin/par_ilut_preconditioned_solver"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(os.path.join(ex, "bin", "par_ilut_preconditioned_solver"))


def build_par_ilut_shim_smoke(tmp_path):
    """shims/hip/factorization/par_ilut_kernels.hip.cpp against the mirror, linked with shims/test/shim_smoke8.cpp"""
    obj = tmp_path / "par_ilut_kernels.o"
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Wno-unused-parameter", f"-I{ROOT}/include", f"-I{PKG}/include",
                        "-include", os.path.join(ROOT, "shims", "test", "prelude_mirror.hpp"), "-c",
                        os.path.join(ROOT, "shims", "hip", "factorization", "par_ilut_kernels.hip.cpp"), "-o", str(obj)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe = tmp_path / "shim_smoke8"
    r = subprocess.run(["g++", "-std=c++14", f"-I{ROOT}/include", f"-I{PKG}/include", f"-I{ROOT}/shims/test",
                        os.path.join(ROOT, "shims", "test", "shim_smoke8.cpp"), str(obj), "-o", str(exe), f"-L{PKG}/lib", "-lgkomi",
                        f"-Wl,-rpath,{PKG}/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_par_ilut_shim_compiles_against_the_mirror(tmp_path):
    assert os.path.exists(build_par_ilut_shim_smoke(tmp_path))


def test_integration_notes_list_the_shim():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "factorization/par_ilut_kernels.hip.cpp" in text and "shim_smoke8.cpp" in text
    left_out = text.split("leaves `NotCompiled`", 1)[1]
    assert "`par_ilut`" not in left_out and "`par_ict`" in left_out


# ---- the C ABI and the Python layer, without a device -----------------------------------------------------------------

def code(fn, *args):
    import gkomi
    try:
        return fn(*args)
    except gkomi.GkomiError as e:
        return e.code


def test_abi_rejects_bad_arguments_before_any_hip_call(gk):
    out = ctypes.c_double(-1.0)
    total = ctypes.c_int64(-1)
    total2 = ctypes.c_int64(-1)
    o, t, t2 = ctypes.addressof(out), ctypes.addressof(total), ctypes.addressof(total2)
    # threshold_select: rank outside [0, nnz), no output, no workspace
    assert gk.par_ilut_select_workspace_bytes(-1) == 0 and gk.par_ilut_select_workspace_bytes(10) > 0
    for nnz, rank in ((10, -1), (10, 10), (0, 0), (-1, 0)):
        assert code(gk.par_ilut_threshold_select_f64, None, nnz, 8, rank, 8, 1 << 20, o) == -1
    assert code(gk.par_ilut_threshold_select_f64, None, 10, 8, 3, 8, 1 << 20, None) == -1
    assert code(gk.par_ilut_threshold_select_f64, None, 10, 8, 3, 8, 16, o) == -4
    # the approximate threshold
    assert gk.par_ilut_approx_workspace_bytes() >= 8 * 255 + 4 * 256
    for nnz, rank in ((10, -1), (10, 10), (-1, 0)):
        assert code(gk.par_ilut_threshold_approx_f64, None, nnz, 8, rank, 8, 1 << 20, o) == -1
    assert code(gk.par_ilut_threshold_approx_f64, None, 10, None, 3, 8, 1 << 20, o) == -1
    assert code(gk.par_ilut_threshold_approx_f64, None, 10, 8, 3, 8, 16, o) == -4
    # threshold_filter
    assert gk.par_ilut_filter_workspace_bytes(-1) == 0 and gk.par_ilut_filter_workspace_bytes(10) > 0
    assert code(gk.par_ilut_threshold_filter_f64_i32, None, -1, 8, 8, 8, 0.5, 8, None, None, None, t, 8, 1 << 20) == -1
    assert code(gk.par_ilut_threshold_filter_f64_i32, None, 4, 8, 8, 8, 0.5, 8, 8, None, None, t, 8, 1 << 20) == -1   # cols alone
    assert code(gk.par_ilut_threshold_filter_f64_i32, None, 4, 8, 8, 8, 0.5, 8, None, None, 8, t, 8, 1 << 20) == -1   # COO in a count
    assert code(gk.par_ilut_threshold_filter_f64_i32, None, 4, 8, 8, 8, 0.5, 8, None, None, None, None, 8, 1 << 20) == -1
    assert code(gk.par_ilut_threshold_filter_f64_i32, None, 4, 8, 8, 8, 0.5, 8, None, None, None, t, 8, 16) == -4
    # add_candidates
    assert gk.par_ilut_add_candidates_workspace_bytes(-1) == 0 and gk.par_ilut_add_candidates_workspace_bytes(10) > 0
    m = (8, 8, 8)
    assert code(gk.par_ilut_add_candidates_f64_i32, None, -1, *m, *m, *m, *m, 8, None, None, 8, None, None, t, t2, 8, 1 << 20) == -1
    assert code(gk.par_ilut_add_candidates_f64_i32, None, 4, *m, *m, *m, *m, 8, 8, None, 8, None, None, t, t2, 8, 1 << 20) == -1
    assert code(gk.par_ilut_add_candidates_f64_i32, None, 4, *m, *m, *m, *m, 8, None, None, 8, None, None, t, None, 8, 1 << 20) == -1
    assert code(gk.par_ilut_add_candidates_f64_i32, None, 4, *m, *m, *m, *m, 8, None, None, 8, None, None, t, t2, 8, 16) == -4
    # the sweep: a factor with fewer entries than rows has no diagonal everywhere
    info = (ctypes.c_int64 * 6)()
    assert gk.par_ilut_sweep_workspace_bytes(-1, 0, 0) == 0 and gk.par_ilut_sweep_workspace_bytes(10, 20, 20) > 0
    assert code(gk.par_ilut_analyse_i32, None, -1, 0, None, None, 0, None, None, 8, 1 << 20, ctypes.addressof(info)) == -1
    assert code(gk.par_ilut_analyse_i32, None, 4, 3, 8, 8, 6, 8, 8, 8, 1 << 20, ctypes.addressof(info)) == -1
    assert code(gk.par_ilut_analyse_i32, None, 4, 6, 8, 8, 6, 8, 8, 8, 1 << 20, None) == -1
    assert code(gk.par_ilut_analyse_i32, None, 4, 6, 8, 8, 6, 8, 8, 8, 16, ctypes.addressof(info)) == -4
    sweep = gk.par_ilut_compute_l_u_factors_f64_i32
    assert code(sweep, None, -1, *m, 0, *m, 0, *m, None, None, None, 8, 1 << 20) == -1
    assert code(sweep, None, 4, *m, 6, *m, 3, *m, None, None, None, 8, 1 << 20) == -1
    assert code(sweep, None, 4, *m, 6, *m, 6, *m, 8, None, 8, 8, 1 << 20) == -1      # the CSC copy: all of it or none
    assert code(sweep, None, 4, *m, 6, *m, 6, *m, None, None, None, 8, 16) == -4
    assert (out.value, total.value, total2.value) == (-1.0, -1, -1)


def test_abi_accepts_empty_input_without_a_device(gk):
    out = ctypes.c_double(-1.0)
    total = ctypes.c_int64(0)
    total2 = ctypes.c_int64(0)
    assert gk.par_ilut_threshold_approx_f64(None, 0, None, 0, None, 0, ctypes.addressof(out)) == 0 and out.value == 0.0
    # the fill calls of an empty matrix have nothing to write
    assert gk.par_ilut_threshold_filter_f64_i32(None, 0, 8, None, None, 0.5, 8, 8, 8, None, ctypes.addressof(total), None, 0) == 0
    m = (None, None, None)
    assert gk.par_ilut_add_candidates_f64_i32(None, 0, *m, *m, *m, *m, 8, 8, 8, 8, 8, 8, ctypes.addressof(total),
                                              ctypes.addressof(total2), None, 0) == 0
    tuning = (ctypes.c_int64 * 4)()
    gk.par_ilut_tuning(None)
    gk.par_ilut_tuning(ctypes.addressof(tuning))
    assert 0 < tuning[0] < tuning[1] < tuning[2] and tuning[3] > 0


class NoDevice:
    """stands in for a device tensor: any use beyond its size is an error"""

    def __init__(self, count):
        self.count = count

    def numel(self):
        return self.count

    def __getattr__(self, name):
        raise AssertionError(f"the argument check touched .{name}")


def test_python_layer_refuses_bad_parameters_before_touching_a_device(gk):
    from gkomi import solvers
    rp, ci, v = NoDevice(5), NoDevice(7), NoDevice(7)
    for limit in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="fill_in_limit"):
            solvers.par_ilut_generate(gk, 4, rp, ci, v, fill_in_limit=limit)
    with pytest.raises(ValueError, match="square"):
        solvers.par_ilut_generate(gk, 3, rp, ci, v)
    with pytest.raises(ValueError, match="square"):
        solvers.par_ilut_generate(gk, 4, rp, ci, v, ncols=5)
