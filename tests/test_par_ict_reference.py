"""CPU side of ParICT.  The plain-Python restatement (tests/par_ict_util.py) is pinned to the reference twice: to the
answers the reference's own tests expect (tests/golden/par_ict.json, the reference's tolerance) and, bit for bit, to
results recorded from the reference executor (tests/golden/par_ict_ref.json, written by the verb par_ict of
oracle/ref_driver.cpp).  Wherever that driver is, it runs again and the fixture is compared with what it gives, so the
fixture cannot go stale.  Then the C ABI's argument checks and the Python layer's, none of which needs a device; the mirror
example builds and the shim compiles against the mirror prelude and links with shims/test/shim_smoke9.cpp."""
import ctypes
import functools
import json
import math
import os
import subprocess

import numpy as np
import pytest

import ilu_exact_util as xu
import par_ict_util as iu
import par_ilut_util as pu
import ref_exec

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "repo-8852-ginkgo_amd")
G = json.load(open(os.path.join(HERE, "golden", "par_ict.json")))
REF = json.load(open(os.path.join(HERE, "golden", "par_ict_ref.json")))
R_DOUBLE = 10 * np.finfo(np.float64).eps     # r<double>::value (core/test/utils.hpp:212-219)


def dense(a):
    """a matrix of the fixture, by name or as rows; ["sqrt", x] is sqrt(x) as the reference's test writes it"""
    a = G[a] if isinstance(a, str) else a
    return np.array([[math.sqrt(x[1]) if isinstance(x, list) else x for x in row] for row in a], np.float64)


def csr(a):
    return iu.dense_to_csr(dense(a))


def near(got, want, tol):
    """GKO_ASSERT_MTX_NEAR: relative Frobenius norm of the difference"""
    want = dense(want)
    return np.linalg.norm(xu.csr_to_dense(got) - want) <= tol * np.linalg.norm(want)


def same_sparsity(got, want):
    """GKO_ASSERT_MTX_EQ_SPARSITY against gko::initialize<Csr> of the expected rows"""
    w = iu.dense_to_csr(dense(want))
    return np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1])


# ---- the reference's known answers --------------------------------------------------------------------------

def test_fixture_names_its_source():
    assert "reference/test/factorization/par_ict_kernels.cpp" in G["source"]
    assert [c["test"] for c in G["generate"]] == ["GenerateIdentity", "GenerateWithExactSmallLimit", "GenerateWithApproxSmallLimit",
                                                  "GenerateWithExactLargeLimit", "GenerateWithApproxLargeLimit"]


def test_restatement_initializes_the_reference_s_row_ptrs():
    c = G["initialize_row_ptrs_l"]
    assert c["test"] == "KernelInitializeRowPtrsL"
    assert iu.initialize_l(csr(c["matrix"]), True)[0].tolist() == c["expect"]


def test_restatement_initializes_l_like_the_reference():
    c = G["initialize_l"]
    got = iu.initialize_l(csr(c["matrix"]), True)
    assert same_sparsity(got, c["expect"]) and near(got, c["expect"], R_DOUBLE)


def test_restatement_adds_the_reference_s_candidates():
    c = G["add_candidates"]
    got = iu.add_candidates(csr("mtx_llh"), csr("mtx_system"), csr("mtx_l"))
    assert same_sparsity(got, c["expect"]) and near(got, c["expect"], R_DOUBLE)


def test_restatement_sweeps_like_the_reference():
    c = G["compute_factor"]
    got = iu.compute_factor(csr("mtx_system"), csr("mtx_l_system"))
    assert near(got, c["expect"], R_DOUBLE)


@pytest.mark.parametrize("c", G["generate"], ids=lambda c: c["test"])
def test_restatement_generates_the_reference_s_factor(c):
    l, lt = iu.generate(csr(c["matrix"]), fill_in_limit=c.get("fill_in_limit", 2.0),
                        approximate_select=c.get("approximate_select", True))
    assert near(l, c["l_expect"], R_DOUBLE) and near(lt, dense(c["l_expect"]).T.tolist(), R_DOUBLE)


# ---- results recorded from the reference executor ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def recorded_case(name):
    m = iu.RECORDED_CASES[name]()
    for a in m:
        a.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def generated(name, select, limit):
    """5 iterations of one configuration: (L, traces)"""
    traces = []
    l, _ = iu.generate(recorded_case(name), iterations=5, fill_in_limit=limit, approximate_select=select == "approx", traces=traces)
    return l, traces


matches = ref_exec.matches     # an array or a CSR matrix is the recorded one: the digest, and the items where kept


def test_the_fixture_describes_the_cases_of_the_restatement():
    assert sorted(REF["cases"]) == sorted(iu.RECORDED_CASES)
    assert "RECORDED_CASES of tests/par_ict_util.py" in REF["source"]
    for name, c in REF["cases"].items():
        m = recorded_case(name)
        assert (c["n"], c["nnz"]) == (len(m[0]) - 1, len(m[1])), name
    lacking = recorded_case("ani1_without_some_diagonals")
    assert sum(1 for r, row in enumerate(xu.to_rows(lacking)) if r not in row) == 8
    whole, halved = xu.to_rows(recorded_case("ani1")), xu.to_rows(recorded_case("ani1_with_some_diagonals_halved"))
    assert [i for i in range(len(whole)) if halved[i] != whole[i]] == list(range(0, len(whole), 5))
    assert all(halved[i][i] == 0.5 * whole[i][i] for i in range(0, len(whole), 5))
    assert os.path.getsize(os.path.join(HERE, "golden", "par_ict_ref.json")) < 100 * 1024


@pytest.mark.parametrize("name", sorted(iu.RECORDED_CASES))
def test_restatement_kernels_equal_the_recorded_ones_bit_for_bit(name):
    """each kernel alone on the intermediate matrices of the first iteration at fill_in_limit 1.2"""
    m, rec = recorded_case(name), REF["cases"][name]["records"]
    traces = []
    l, _ = iu.generate(m, iterations=1, fill_in_limit=1.2, approximate_select=False, traces=traces)
    t = traces[0]
    assert matches(rec["kernels/initialize_l"], iu.initialize_l(m, True))
    assert matches(rec["kernels/llh"], t["llh"])
    assert matches(rec["kernels/add_candidates"], t["l_cand"])
    assert matches(rec["kernels/sweep"], t["l_new"])
    assert matches(rec["kernels/ranks"], np.array([t["l_rank"]], np.int32))
    assert matches(rec["kernels/select"], np.array([t["l_threshold"]]))
    assert matches(rec["kernels/filter"], t["l_filtered"])
    threshold, l_approx = pu.threshold_filter_approx(t["l_new"], t["l_rank"])
    assert matches(rec["kernels/approx"], np.array([threshold]))
    assert matches(rec["kernels/filter_approx"], l_approx)
    assert matches(rec["kernels/second_sweep"], l)


@pytest.mark.parametrize("name", sorted(iu.RECORDED_CASES))
def test_restatement_generate_equals_the_recorded_factor_bit_for_bit(name):
    """exact and approximate selection, fill_in_limit 0.75 / 1.2 / 2.0: the entry counts after 1 ... 5 iterations, the
    factor after 1 and 5; and every stored value of every such factor is finite (a digest cannot compare the payloads
    of NaNs across machines)"""
    m, rec = recorded_case(name), REF["cases"][name]["records"]
    for select in ("exact", "approx"):
        for limit in iu.RECORDED_LIMITS:
            l, traces = generated(name, select, limit)
            key = f"generate/{select}/{limit:g}"
            assert [t["l_nnz"] for t in traces] == rec[key + "/nnz"], key
            assert matches(rec[key + "/5/l"], l), key
            l1, _ = iu.generate(m, iterations=1, fill_in_limit=limit, approximate_select=select == "approx")
            assert matches(rec[key + "/1/l"], l1), key
            assert np.isfinite(l[2]).all() and np.isfinite(l1[2]).all(), key


def test_recorded_cases_make_both_sweeps_reject_values_that_are_not_finite():
    """The halved diagonals of ani1 make both sweeps of every iteration of every configuration meet values that are not
    finite (and so does ani4 in its second iteration at the larger limits); the factors stay finite
    (test_restatement_generate_equals_the_recorded_factor_bit_for_bit)."""
    first = second = 0
    for select in ("exact", "approx"):
        for limit in iu.RECORDED_LIMITS:
            _, traces = generated("ani1_with_some_diagonals_halved", select, limit)
            counts = [(len(t["rejected"][0]), len(t["rejected"][1])) for t in traces]
            print(select, limit, counts)
            assert all(a >= 1 and b >= 1 for a, b in counts), (select, limit, counts)
            first += sum(a for a, _ in counts)
            second += sum(b for _, b in counts)
    assert first > 0 and second > 0
    every = [c for select in ("exact", "approx") for limit in iu.RECORDED_LIMITS
             for t in generated("ani1_with_some_diagonals_halved", select, limit)[1] for c in map(len, t["rejected"])]
    assert (min(every), max(every)) == (3, 21)
    # ani4: one value in each sweep of iteration 2 at fill_in_limit 2.0, one in its first sweep at 1.2, none at 0.75
    for select in ("exact", "approx"):
        for limit, second_iteration in ((2.0, (1, 1)), (1.2, (1, 0)), (0.75, (0, 0))):
            _, traces = generated("ani4", select, limit)
            counts = [(len(t["rejected"][0]), len(t["rejected"][1])) for t in traces]
            assert counts == [(0, 0), second_iteration, (0, 0), (0, 0), (0, 0)], (select, limit, counts)


def test_the_driver_reproduces_the_fixture():
    """oracle/_ref/ref_driver, the reference executor itself, gives the fixture as it is committed: every recorded array
    of every case, the keys compared both ways.  One driver process; a missing driver fails wherever the reference or
    oracle/_ref/ is."""
    if ref_exec.may_skip():
        pytest.skip("neither the reference nor oracle/_ref/ is on this machine")
    assert ref_exec.difference_from_driver("par_ict", REF) is None


# ---- the mirror and the shims build ------------------------------------------------------------------------------

def test_mirror_example_builds():
    ex = os.path.join(PKG, "examples")
    r = subprocess.run(["make", "-C", ex, "bin/par_ict_preconditioned_solver"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(os.path.join(ex, "bin", "par_ict_preconditioned_solver"))


def build_par_ict_shim_smoke(tmp_path):
    """shims/hip/factorization/par_ict_kernels.hip.cpp against the mirror, linked with shims/test/shim_smoke9.cpp"""
    obj = tmp_path / "par_ict_kernels.o"
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Wno-unused-parameter", f"-I{ROOT}/include", f"-I{PKG}/include",
                        "-include", os.path.join(ROOT, "shims", "test", "prelude_mirror.hpp"), "-c",
                        os.path.join(ROOT, "shims", "hip", "factorization", "par_ict_kernels.hip.cpp"), "-o", str(obj)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe = tmp_path / "shim_smoke9"
    r = subprocess.run(["g++", "-std=c++14", f"-I{ROOT}/include", f"-I{PKG}/include", f"-I{ROOT}/shims/test",
                        os.path.join(ROOT, "shims", "test", "shim_smoke9.cpp"), str(obj), "-o", str(exe), f"-L{PKG}/lib", "-lgkomi",
                        f"-Wl,-rpath,{PKG}/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_par_ict_shim_compiles_against_the_mirror(tmp_path):
    assert os.path.exists(build_par_ict_shim_smoke(tmp_path))


def test_integration_notes_list_the_shim():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "factorization/par_ict_kernels.hip.cpp" in text and "shim_smoke9.cpp" in text
    left_out = text.split("leaves `NotCompiled`", 1)[1]
    # of par_ict only the <double, int32> instantiation is bound
    assert "`par_ict`" in left_out and "<double, int32>" in left_out


# ---- the C ABI and the Python layer, without a device -----------------------------------------------------------------

def code(fn, *args):
    import gkomi
    try:
        return fn(*args)
    except gkomi.GkomiError as e:
        return e.code


def test_abi_rejects_bad_arguments_before_any_hip_call(gk):
    total = ctypes.c_int64(-1)
    t = ctypes.addressof(total)
    m = (8, 8, 8)
    # add_candidates: negative size, values without indices, no total, NULL row pointers, a short workspace, no workspace
    assert gk.par_ict_add_candidates_workspace_bytes(-1) == 0 and gk.par_ict_add_candidates_workspace_bytes(10) > 0
    add = gk.par_ict_add_candidates_f64_i32
    assert code(add, None, -1, *m, *m, *m, 8, None, None, t, 8, 1 << 20) == -1
    assert code(add, None, 4, *m, *m, *m, 8, 8, None, t, 8, 1 << 20) == -1
    assert code(add, None, 4, *m, *m, *m, 8, None, 8, t, 8, 1 << 20) == -1
    assert code(add, None, 4, *m, *m, *m, 8, None, None, None, 8, 1 << 20) == -1
    assert code(add, None, 4, *m, *m, *m, None, None, None, t, 8, 1 << 20) == -1
    assert code(add, None, 4, None, 8, 8, *m, *m, 8, None, None, t, 8, 1 << 20) == -1
    assert code(add, None, 4, *m, None, 8, 8, *m, 8, None, None, t, 8, 1 << 20) == -1
    assert code(add, None, 4, *m, *m, None, 8, 8, 8, None, None, t, 8, 1 << 20) == -1
    assert code(add, None, 4, *m, *m, *m, 8, None, None, t, 8, 16) == -4
    assert code(add, None, 4, *m, *m, *m, 8, None, None, t, None, 1 << 20) == -4
    # the fill call: a total out of range, L without its arrays
    total.value = -5
    assert code(add, None, 4, *m, *m, *m, 8, 8, 8, t, 8, 1 << 20) == -1
    total.value = 3
    assert code(add, None, 4, *m, *m, 8, None, 8, 8, 8, 8, t, 8, 1 << 20) == -1
    total.value = -1
    # the sweep: a factor with fewer entries than rows has no diagonal everywhere
    info = (ctypes.c_int64 * 6)()
    i = ctypes.addressof(info)
    assert gk.par_ict_sweep_workspace_bytes(-1, 0) == 0 and gk.par_ict_sweep_workspace_bytes(10, -1) == 0
    assert gk.par_ict_sweep_workspace_bytes(10, 20) > 0
    analyse = gk.par_ict_analyse_i32
    assert code(analyse, None, -1, 0, None, None, 8, 1 << 20, i) == -1
    assert code(analyse, None, 4, -1, 8, 8, 8, 1 << 20, i) == -1
    assert code(analyse, None, 4, 3, 8, 8, 8, 1 << 20, i) == -1
    assert code(analyse, None, 4, 6, None, 8, 8, 1 << 20, i) == -1
    assert code(analyse, None, 4, 6, 8, None, 8, 1 << 20, i) == -1
    assert code(analyse, None, 4, 6, 8, 8, 8, 1 << 20, None) == -1
    assert code(analyse, None, 0, 2, 8, 8, 8, 1 << 20, i) == -1
    assert code(analyse, None, 4, 6, 8, 8, 8, 16, i) == -4
    assert code(analyse, None, 4, 6, 8, 8, None, 1 << 20, i) == -4
    sweep = gk.par_ict_compute_factor_f64_i32
    assert code(sweep, None, -1, *m, 0, *m, 8, 1 << 20) == -1
    assert code(sweep, None, 4, *m, 3, *m, 8, 1 << 20) == -1
    assert code(sweep, None, 4, None, 8, 8, 6, *m, 8, 1 << 20) == -1
    assert code(sweep, None, 4, *m, 6, None, 8, 8, 8, 1 << 20) == -1
    assert code(sweep, None, 4, *m, 6, 8, None, 8, 8, 1 << 20) == -1
    assert code(sweep, None, 4, *m, 6, 8, 8, None, 8, 1 << 20) == -1
    assert code(sweep, None, 4, *m, 6, *m, 8, 16) == -4
    # a workspace without an analysis
    assert code(sweep, None, 4, *m, 6, *m, None, 1 << 20) == -4
    assert total.value == -1 and list(info) == [0] * 6


def test_abi_accepts_empty_input_without_a_device(gk):
    total = ctypes.c_int64(0)
    m = (None, None, None)
    # the fill call of an empty matrix has nothing to write
    assert gk.par_ict_add_candidates_f64_i32(None, 0, *m, *m, *m, 8, 8, 8, ctypes.addressof(total), None, 0) == 0
    tuning = (ctypes.c_int64 * 4)()
    gk.par_ict_tuning(None)
    gk.par_ict_tuning(ctypes.addressof(tuning))
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
            solvers.par_ict_generate(gk, 4, rp, ci, v, fill_in_limit=limit)
    with pytest.raises(ValueError, match="square"):
        solvers.par_ict_generate(gk, 3, rp, ci, v)
    with pytest.raises(ValueError, match="square"):
        solvers.par_ict_generate(gk, 4, rp, ci, v, ncols=5)
