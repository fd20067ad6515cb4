"""CPU side of ISAI.  The plain-Python restatement (tests/isai_util.py) is pinned to the reference twice: to the answers
the reference's own tests expect (tests/golden/isai.json and the isai_*.mtx files, the reference's tolerance) and, bit for
bit, to results recorded from the reference executor (tests/golden/isai_ref.json, written by the verb isai of
oracle/ref_driver.cpp).  Wherever that driver is, it runs again and the fixture is compared with what it gives, so the
fixture cannot go stale.  Then the C ABI's argument checks and the Python layer's, none of which needs a device."""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import ilu_exact_util as xu
import isai_util as iu
import ref_exec
import spgemm_util as su

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = json.load(open(os.path.join(HERE, "golden", "isai.json")))
REF = json.load(open(os.path.join(HERE, "golden", "isai_ref.json")))
R_DOUBLE = 10 * np.finfo(np.float64).eps     # r<double>::value (core/test/utils.hpp:212-219)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """a matrix of the fixture as CSR: dense rows (zeros not stored), CSR arrays as they are, or a file"""
    m = G["matrices"][name]
    if "dense" in m:
        return xu.dense_to_csr(np.array(m["dense"], np.float64))
    if "file" in m:
        return read_file(m["file"])
    return (np.array(m["row_ptrs"], np.int32), np.array(m["col_idxs"], np.int32), np.array(m["vals"], np.float64))


def read_file(name):
    """square matrices as sorted CSR, a vector as a dense column; 12345 stands for a stored zero"""
    import matgen
    kind, nr, nc, rows, cols, vals = matgen.read_mtx(os.path.join(HERE, "golden", name))
    vals = np.array(vals, np.float64)
    vals[vals == 12345.0] = 0.0
    if kind != "coo":
        return vals.reshape(nr, nc)
    if nc == 1:
        col = np.zeros((nr, 1))
        col[np.asarray(rows), 0] = vals
        return col
    return xu.sort_by_column_index(tuple(matgen.coo_to_csr(nr, rows, cols, vals)))


def transposed(m):
    n = len(m[0]) - 1
    return su.transpose(n, n, m)


def filled(ranges, n):
    """std::fill_n(a.get_data() + begin, count, value) on zeros of n + 1 entries"""
    a = np.zeros(n + 1, np.int32)
    for begin, count, value in ranges or []:
        a[begin:begin + count] = value
    return a


def near(got, want, tol):
    """GKO_ASSERT_MTX_NEAR: relative Frobenius norm of the difference"""
    g, w = xu.csr_to_dense(got), xu.csr_to_dense(want)
    return np.linalg.norm(g - w) <= tol * np.linalg.norm(w)


def same_sparsity(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def minus_ones(m):
    """clone_allocations: the pattern with values of -1"""
    return m[0], m[1], np.full(len(m[2]), -1.0)


# ---- the reference's known answers --------------------------------------------------------------------------

def test_fixture_names_its_source():
    assert "reference/test/preconditioner/isai_kernels.cpp" in G["source"]
    files = sorted(f for f in os.listdir(os.path.join(HERE, "golden")) if f.startswith("isai_") and f.endswith(".mtx"))
    assert len(files) == 20 and max(os.path.getsize(os.path.join(HERE, "golden", f)) for f in files) < 14 * 1024
    assert sorted(m["file"] for m in G["matrices"].values() if "file" in m) == files
    readme = open(os.path.join(HERE, "golden", "README_isai.md")).read()
    assert all(f in readme for f in files)


@pytest.mark.parametrize("c", G["kernel_generate"], ids=lambda c: c["test"])
def test_restatement_generate_kernel_gives_the_reference_s_answer(c):
    m = matrix(c["matrix"])
    if c.get("transposed"):
        m = transposed(m)
    pattern = matrix(c["pattern"]) if "pattern" in c else m
    want = matrix(c["expect_as_is"]) if "expect_as_is" in c else matrix(c["expect"])
    if c.get("transposed") and "expect_as_is" not in c:
        want = transposed(want)
    got, a1, a2 = iu.generic_generate(m, minus_ones(pattern), c["kind"])
    n = len(m[0]) - 1
    assert same_sparsity(got, want) and near(got, want, R_DOUBLE)
    assert np.array_equal(a1, filled(c.get("rhs_ptrs"), n)) and np.array_equal(a2, filled(c.get("nz_ptrs"), n))


@pytest.mark.parametrize("c", G["kernel_excess"], ids=lambda c: c["test"])
def test_restatement_excess_system_is_the_reference_s(c):
    m, pattern = matrix(c["matrix"]), matrix(c["pattern"])
    n = len(m[0]) - 1
    system, rhs = iu.generate_excess_system(m, pattern, filled(c["rhs_ptrs"], n), filled(c["nz_ptrs"], n), 0, n)
    want = matrix(c["system"])
    assert (len(rhs), len(system[2])) == (c["dim"], c["nnz"])
    assert same_sparsity(system, want) and np.array_equal(system[2], want[2])
    assert np.array_equal(rhs, matrix(c["rhs"])[:, 0])


def test_restatement_scatters_like_the_reference():
    c = G["kernel_scatter"]
    as_csr = lambda m: (np.array(m["row_ptrs"], np.int32), np.array(m["col_idxs"], np.int32), np.array(m["vals"], np.float64))
    got = iu.scatter_excess_solution(np.array(c["ptrs"], np.int32), np.array(c["solution"], np.float64), as_csr(c["matrix"]), 0, 6)
    assert np.array_equal(got[2], as_csr(c["expect"])[2])


@pytest.mark.parametrize("c", G["generate"], ids=lambda c: c["test"])
def test_restatement_generates_the_reference_s_inverse(c):
    want = matrix(c["expect"])
    got = iu.generate_inverse(matrix(c["matrix"]), c["kind"], sparsity_power=c.get("sparsity_power", 1))
    assert same_sparsity(got, want) and near(got, want, c["tol_r"] * R_DOUBLE)


@pytest.mark.parametrize("c", G["apply"], ids=lambda c: c["test"])
def test_restatement_applies_like_the_reference(c):
    inv = xu.csr_to_dense(iu.generate_inverse(matrix(c["matrix"]), c["kind"]))
    vec = np.array(c["vec"], np.float64)
    got = inv.T @ (inv @ vec) if c["kind"] == "spd" else inv @ vec
    if "alpha" in c:
        got = c["alpha"] * got + c["beta"] * np.array(c["result"], np.float64)
    want = np.array(c["expect"], np.float64)
    assert np.linalg.norm(got - want) <= R_DOUBLE * np.linalg.norm(want)


def test_restatement_serves_ilu_like_the_reference():
    c = G["ilu"]
    li = xu.csr_to_dense(iu.generate_inverse(matrix(c["l"]), "lower"))
    ui = xu.csr_to_dense(iu.generate_inverse(matrix(c["u"]), "upper"))
    got, want = ui @ (li @ np.array(c["vec"], np.float64)), np.array(c["expect"], np.float64)
    assert np.linalg.norm(got - want) <= R_DOUBLE * np.linalg.norm(want)


# ---- results recorded from the reference executor ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def recorded_case(name):
    kind, power, limit, make = iu.RECORDED_CASES[name]
    m = make()
    for a in m:
        a.setflags(write=False)
    return kind, power, limit, m


@functools.lru_cache(maxsize=None)
def restated(name):
    """(inverse, trace) of the restatement's generate_inverse"""
    kind, power, limit, m = recorded_case(name)
    trace = {}
    inv = iu.generate_inverse(m, kind, sparsity_power=power, excess_limit=limit, trace=trace)
    return inv, trace


matches = ref_exec.matches     # an array or a CSR matrix is the recorded one: the digest, and the items where kept


def counts_of(pattern, trace):
    ln = iu.row_lengths(pattern)
    rows, entries = iu.long_rows(pattern)
    return [rows, entries, int(ln.max()), len(trace["excess"])]


def long_rows_zeroed(m):
    rp, ci, v = m[0], m[1], np.array(m[2], np.float64)
    for row in np.nonzero(iu.row_lengths(m) > iu.ROW_SIZE_LIMIT)[0]:
        v[rp[row]:rp[row + 1]] = 0.0
    return rp, ci, v


def test_the_fixture_describes_the_cases_of_the_restatement():
    assert list(REF["cases"]) == list(iu.RECORDED_CASES)
    assert "RECORDED_CASES of tests/isai_util.py" in REF["source"]
    for name, c in REF["cases"].items():
        kind, power, limit, m = recorded_case(name)
        assert (c["kind"], c["sparsity_power"], c["excess_limit"], c["n"], c["nnz"]) == (kind, power, limit, len(m[0]) - 1, len(m[1])), name
    assert os.path.getsize(os.path.join(HERE, "golden", "isai_ref.json")) < 100 * 1024


def test_the_recorded_cases_exercise_the_paths_they_are_there_for():
    """the counts the driver met: rows over the limit, their entries, the longest row, blocks of the excess loop"""
    met = {name: c["records"]["kernel/counts"]["items"] for name, c in REF["cases"].items()}
    for name, want in iu.EXPECTED_COUNTS.items():
        assert all(w is None or w == g for w, g in zip(want, met[name])), (name, met[name])
    # no row of the powers 1 ... 4 of the factors of ani1 passes 28: all direct, odd and even branch of the powers
    assert max(met[f"ani1_{f}_p{p}"][2] for f in "lu" for p in (1, 2, 3, 4)) == 28
    assert all(met[f"ani1_{f}_p{p}"][0] == 0 for f in "lu" for p in (1, 2, 3, 4))
    # the lower factor of ani4 at power 4 takes several blocks at excess_limit 1000
    assert met["ani4_l_p4_limit1000"][3] > 2 and met["ani4_l_p4_limit0"][3] == 1
    # isai_l, isai_u: 35 rows, rows of 33; the general and spd cases with long rows
    assert met["isai_l"][:3] == [2, 66, 33] and met["isai_u"][:3] == [1, 33, 33]
    assert met["isai_a_general"][0] == 2 and met["isai_spd_spd"][0] == 1


@pytest.mark.parametrize("name", list(iu.RECORDED_CASES))
def test_restatement_equals_the_recorded_results_bit_for_bit(name):
    kind, power, limit, m = recorded_case(name)
    rec = REF["cases"][name]["records"]
    inv, trace = restated(name)
    assert counts_of(inv, trace) == rec["kernel/counts"]["items"]
    assert matches(rec["kernel/excess_rhs_ptrs"], trace["excess_rhs_ptrs"])
    assert matches(rec["kernel/excess_nz_ptrs"], trace["excess_nz_ptrs"])
    assert matches(rec["kernel/direct"], long_rows_zeroed(trace["direct"]))
    for b, e in enumerate(trace["excess"]):
        assert rec[f"excess/{b}/range"]["items"] == [e["start"], e["end"]]
        assert matches(rec[f"excess/{b}/system"], e["system"])
        assert matches(rec[f"excess/{b}/rhs_vals"], e["rhs"])
    # the whole inverse wherever no iterative solver took part
    assert ("generate/inverse" in rec) == (kind in ("lower", "upper") or not trace["excess"])
    if "generate/inverse" in rec:
        assert np.isfinite(inv[2]).all()
        assert matches(rec["generate/inverse"], inv)


def test_the_guard_writes_identity_rows_in_the_recorded_cases():
    """a zero diagonal entry: the row's solve divides by it, every value is not finite and the row becomes the identity's;
    a diagonal entry that the pattern lacks: the row has no 1 to receive, whatever is not finite becomes 0"""
    rows = xu.to_rows(restated("ani1_l_zero_diagonals")[0])
    for i in range(0, len(rows), 5):
        assert all(v == (1.0 if c == i else 0.0) for c, v in rows[i].items()), i
    rows = xu.to_rows(restated("ani1_l_missing_diagonals")[0])
    assert all(i not in rows[i] for i in range(0, len(rows), 5))
    assert all(np.isfinite(v) for row in rows for v in row.values())


def test_the_driver_reproduces_the_fixture():
    """oracle/_ref/ref_driver, the reference executor itself, gives the fixture as it is committed: every recorded array
    of every case, the keys compared both ways.  One driver process; a missing driver fails wherever the reference or
    oracle/_ref/ is."""
    if ref_exec.may_skip():
        pytest.skip("neither the reference nor oracle/_ref/ is on this machine")
    assert ref_exec.difference_from_driver("isai", REF) is None


# ---- the C ABI and the Python layer, without a device -----------------------------------------------------------------

def code(fn, *args):
    import gkomi
    try:
        return fn(*args)
    except gkomi.GkomiError as e:
        return e.code


def test_abi_rejects_bad_arguments_before_any_hip_call(gk):
    big = 1 << 20
    m, i = (8, 8, 8), (8, 8, 8)
    assert gk.isai_generate_workspace_bytes(-1) == 0 and gk.isai_generate_workspace_bytes(10) > 0
    for gen in (gk.isai_generate_tri_inverse_f64_i32, gk.isai_generate_general_inverse_f64_i32):
        assert code(gen, None, -1, *m, *i, 8, 8, 1, 8, big) == -1
        assert code(gen, None, 4, *m, *i, 8, 8, 2, 8, big) == -1
        assert code(gen, None, 4, *m, *i, None, 8, 1, 8, big) == -1
        assert code(gen, None, 4, *m, *i, 8, None, 1, 8, big) == -1
        for k in range(6):
            args = [8] * 6
            args[k] = None
            assert code(gen, None, 4, *args, 8, 8, 0, 8, big) == -1, k
        assert code(gen, None, 4, *m, *i, 8, 8, 1, None, big) == -4
        assert code(gen, None, 4, *m, *i, 8, 8, 1, 8, 4) == -4
    ex = gk.isai_generate_excess_system_f64_i32
    tail = (8, 8, 8, 8)
    assert code(ex, None, -1, *m, 8, 8, 8, 8, 3, 5, *tail, 0, 0) == -1
    assert code(ex, None, 4, *m, 8, 8, 8, 8, 3, 5, *tail, 3, 2) == -1
    assert code(ex, None, 4, *m, 8, 8, 8, 8, 3, 5, *tail, 0, 5) == -1
    assert code(ex, None, 4, *m, 8, 8, 8, 8, 3, 5, *tail, -1, 2) == -1
    assert code(ex, None, 4, *m, 8, 8, 8, 8, -3, 5, *tail, 0, 4) == -1
    assert code(ex, None, 4, *m, 8, 8, 8, 8, 3, -5, *tail, 0, 4) == -1
    assert code(ex, None, 4, None, 8, 8, 8, 8, 8, 8, 3, 5, *tail, 0, 4) == -1
    assert code(ex, None, 4, *m, None, 8, 8, 8, 3, 5, *tail, 0, 4) == -1
    assert code(ex, None, 4, *m, 8, 8, None, 8, 3, 5, *tail, 0, 4) == -1
    assert code(ex, None, 4, *m, 8, 8, 8, None, 3, 5, *tail, 0, 4) == -1
    assert code(ex, None, 4, *m, 8, 8, 8, 8, 3, 5, None, 8, 8, 8, 0, 4) == -1
    assert code(ex, None, 4, *m, 8, 8, 8, 8, 3, 5, 8, None, 8, 8, 0, 4) == -1
    assert code(ex, None, 4, *m, 8, 8, 8, 8, 3, 5, 8, 8, None, 8, 0, 4) == -1
    assert code(ex, None, 4, *m, 8, 8, 8, 8, 3, 5, 8, 8, 8, None, 0, 4) == -1
    scale = gk.isai_scale_excess_solution_f64_i32
    assert code(scale, None, -1, 8, 8, 0, 0) == -1
    assert code(scale, None, 4, None, 8, 0, 4) == -1
    assert code(scale, None, 4, 8, None, 0, 4) == -1
    assert code(scale, None, 4, 8, 8, 2, 1) == -1
    assert code(scale, None, 4, 8, 8, 0, 5) == -1
    scatter = gk.isai_scatter_excess_solution_f64_i32
    assert code(scatter, None, -1, 8, 8, 8, 8, 0, 0) == -1
    assert code(scatter, None, 4, None, 8, 8, 8, 0, 4) == -1
    assert code(scatter, None, 4, 8, None, 8, 8, 0, 4) == -1
    assert code(scatter, None, 4, 8, 8, None, 8, 0, 4) == -1
    assert code(scatter, None, 4, 8, 8, 8, None, 0, 4) == -1
    assert code(scatter, None, 4, 8, 8, 8, 8, 3, 1) == -1
    assert code(scatter, None, 4, 8, 8, 8, 8, 0, 5) == -1


def test_abi_accepts_an_empty_range_without_a_device(gk):
    assert gk.isai_scale_excess_solution_f64_i32(None, 4, 8, None, 2, 2) == 0
    assert gk.isai_scatter_excess_solution_f64_i32(None, 4, 8, None, 8, None, 2, 2) == 0
    assert gk.isai_scale_excess_solution_f64_i32(None, 0, 8, None, 0, 0) == 0


def test_apply_callback_rejects_a_bad_record_before_any_hip_call(gk):
    from gkomi import solvers
    fn = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)(
        ctypes.cast(gk._cdll.gkomi_isai_apply_cb, ctypes.c_void_p).value)
    assert fn(None, None, 8, 8) == -1
    ctx = solvers.IsaiCtx()
    ctx.n, ctx.nrhs, ctx.num_matrices = 4, 1, 3
    assert fn(ctypes.addressof(ctx), None, 8, 8) == -1
    ctx.num_matrices = 1
    ctx.first.nrows, ctx.first.ncols = 4, 5
    assert fn(ctypes.addressof(ctx), None, 8, 8) == -1
    ctx.num_matrices, ctx.first.ncols = 2, 4
    ctx.second.nrows, ctx.second.ncols = 4, 4
    assert fn(ctypes.addressof(ctx), None, 8, 8) == -1       # two matrices and no intermediate vector
    assert ctypes.sizeof(solvers.IsaiCtx) == 3 * 8 + 2 * 80 + 8


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
    for power in (0, -1, 1.5):
        with pytest.raises(ValueError, match="sparsity_power"):
            solvers.isai_generate(gk, "lower", 4, rp, ci, v, sparsity_power=power)
    with pytest.raises(ValueError, match="kind"):
        solvers.isai_generate(gk, "diagonal", 4, rp, ci, v)
    with pytest.raises(ValueError, match="excess_limit"):
        solvers.isai_generate(gk, "upper", 4, rp, ci, v, excess_limit=-1)
    with pytest.raises(ValueError, match="square"):
        solvers.isai_generate(gk, "general", 3, rp, ci, v)
    with pytest.raises(ValueError, match="square"):
        solvers.isai_generate(gk, "spd", 4, rp, ci, v, ncols=5)
    with pytest.raises(ValueError, match="square"):
        solvers.isai_preconditioner(gk, "lower", 3, rp, ci, v)
    with pytest.raises(ValueError, match="sparsity_power"):
        solvers.ilu_isai_from_factors(gk, 4, (rp, ci, v), (rp, ci, v), sparsity_power=0)
    with pytest.raises(ValueError, match="square"):
        solvers.ic_isai_from_factor(gk, 5, (rp, ci, v))


# ---- the mirror and the shims build ------------------------------------------------------------------------------

PKG = os.path.join(ROOT, "repo-8852-ginkgo_amd")


def test_mirror_example_builds():
    ex = os.path.join(PKG, "examples")
    r = subprocess.run(["make", "-C", ex, "bin/isai_preconditioned_solver"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(os.path.join(ex, "bin", "isai_preconditioned_solver"))


def build_isai_shim_smoke(tmp_path):
    """shims/hip/preconditioner/isai_kernels.hip.cpp against the mirror, linked with shims/test/shim_smoke10.cpp"""
    obj = tmp_path / "isai_kernels.o"
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Wno-unused-parameter", f"-I{ROOT}/include", f"-I{PKG}/include",
                        "-include", os.path.join(ROOT, "shims", "test", "prelude_mirror.hpp"), "-c",
                        os.path.join(ROOT, "shims", "hip", "preconditioner", "isai_kernels.hip.cpp"), "-o", str(obj)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe = tmp_path / "shim_smoke10"
    r = subprocess.run(["g++", "-std=c++14", f"-I{ROOT}/include", f"-I{PKG}/include", f"-I{ROOT}/shims/test",
                        os.path.join(ROOT, "shims", "test", "shim_smoke10.cpp"), str(obj), "-o", str(exe), f"-L{PKG}/lib", "-lgkomi",
                        f"-Wl,-rpath,{PKG}/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_isai_shim_compiles_against_the_mirror(tmp_path):
    assert os.path.exists(build_isai_shim_smoke(tmp_path))


def test_integration_notes_list_the_shim():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "preconditioner/isai_kernels.hip.cpp" in text and "shim_smoke10.cpp" in text
    left_out = text.split("leaves `NotCompiled`", 1)[1]
    # isai is off the list of families without a binding; only its <double, int32> instantiation is bound
    assert "`isai`" not in left_out and "`preconditioner/isai_kernels`" in left_out and "`par_ict`" in left_out
