"""CPU side of CB-GMRES.  The numpy restatement (tests/cb_gmres_util.py) in its "truncate" + sequential mode is pinned, bit
for bit, to results recorded from the reference executor (tests/golden/cb_gmres_ref.json, written by the verb cb_gmres of
oracle/ref_driver.cpp): the outputs of the four kernels and whole solves for every storage type.  Wherever that driver
is, it runs again and the fixture is compared with what it gives, so the fixture cannot go stale.  Then what the GPU tests rely on is checked here, without a device: the case set takes 0, 1 and 2
re-orthogonalisation passes and a forced reset, no loop test sits near eta, and the iteration counts do not move by more
than one when the sums are grouped.

The fixture keeps arrays of up to 32 entries in full, as hexadecimal floats (the basis as raw storage integers); a longer
array is kept as its count, the SHA-256 of its bits and its first four entries (ref_exec.as_record), which keeps the
file small.  The comparison is bit for bit either way, but a mismatch in a long array is only reported, not located: to
find the entry, compare with the arrays of cb_gmres_util.case_arrays() for a ref_exec.Batch of queue_cases()."""
import functools
import json
import os

import numpy as np
import pytest

import cb_gmres_util as cu
import ref_exec

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = json.load(open(os.path.join(HERE, "golden", "cb_gmres_ref.json")))
SOLVES = [f"{name}/{storage}" for name in cu.SOLVE_CASES for storage in cu.STORAGES]
KERNELS = [f"{name}/{storage}" for name in cu.KERNEL_CASES for storage in cu.STORAGES]


def same(rec, got):
    """the recorded doubles (hexadecimal floats, or count + digest of a long array) are these, bit for bit"""
    return ref_exec.matches(rec, np.asarray(got, np.float64))


def test_the_fixture_describes_the_cases_of_the_restatement():
    assert list(REF["solves"]) == SOLVES and list(REF["kernels"]) == KERNELS
    assert "oracle/ref_driver.cpp, verb cb_gmres," in REF["source"]
    assert os.path.getsize(os.path.join(HERE, "golden", "cb_gmres_ref.json")) < 1 << 20


@functools.lru_cache(maxsize=None)
def restated(key, half, group=0):
    name, storage = key.split("/")
    trace = []
    x, res = cu.restated_solve(name, storage, half, group, trace)
    res["trace"] = np.array(trace)
    return x, res


@pytest.mark.parametrize("key", SOLVES)
def test_restated_solve_equals_the_recorded_one_bit_for_bit(key):
    rec = REF["solves"][key]
    x, res = restated(key, "truncate")
    assert res["iterations"] == rec["iterations"]
    assert same(rec["x"], x)
    assert same(rec["residual_norm"], res["residual_norm"])
    assert restated(key, "rne")[1]["iterations"] == rec["rne_iterations"]


@pytest.mark.parametrize("key", [k for k in SOLVES if "expect_x" in cu.SOLVE_CASES[k.split("/")[0]]])
def test_known_answers_of_the_reference_s_tests(key):
    """reference/test/solver/cb_gmres_kernels.cpp: SolvesStencilSystem, SolvesBigDenseSystem1 and
    SolveWithImplicitResNormCritIsDisabled's system, with that file's assert_precision per storage type"""
    name, storage = key.split("/")
    case = cu.SOLVE_CASES[name]
    tol = {"keep": 1e-14, "integer": 1e-14, "reduce1": 1e-6, "ireduce1": 1e-6, "reduce2": 1e-2, "ireduce2": 1e-2}[storage]
    if name == "medium_k4":
        tol = np.sqrt(tol)
    x = ref_exec.unhex(REF["solves"][key]["x"])       # (these systems have 3 to 6 rows: kept in full)
    want = np.array(case["expect_x"])
    assert np.linalg.norm(x - want) <= 100 * tol * np.linalg.norm(want)


@pytest.mark.parametrize("key", KERNELS)
def test_restated_kernels_equal_the_recorded_ones_bit_for_bit(key):
    name, storage = key.split("/")
    c = cu.KERNEL_CASES[name]
    rec = REF["kernels"][key]
    n, rp, ci, v, b = cu.solve_problem(c)
    nrhs, kd = b.shape[1], c["krylov_dim"]
    a = cu.CsrOperator(n, rp, ci, v)
    residual, gsin, gcos, status = cu.initialize(b, kd)
    assert same(rec["initialize/residual"], residual)
    basis = cu.Basis(kd, n, nrhs, storage, "truncate")
    an = np.zeros((3, nrhs))
    rn, rnc, nxt, fin = cu.restart(residual, basis, kd, an)
    assert same(rec["restart/residual_norm"], rn) and same(rec["restart/residual_norm_collection"], rnc)
    assert same(rec["restart/next"], nxt)
    assert ref_exec.matches(rec["restart/basis"], basis.raw(), integers=True)
    hess = np.zeros((kd + 1, kd * nrhs))
    buf = np.zeros((kd + 1, nrhs))
    for s in range(c["steps"]):
        if s == c["stop_step"]:
            status[c["stop_col"]] = 0x01
        nxt = a.apply(nxt)
        h_iter = hess[:s + 2, nrhs * s:nrhs * (s + 1)]
        cu.arnoldi(nxt, gsin, gcos, rn, rnc, basis, h_iter, buf[:s + 2], an, s, fin, status != 0)
        at = f"arnoldi/{s}/"
        assert same(rec[at + "next"], nxt), at
        assert same(rec[at + "hessenberg_iter"], h_iter), at
        assert same(rec[at + "arnoldi_norm"], an), at
        assert same(rec[at + "residual_norm"], rn) and same(rec[at + "residual_norm_collection"], rnc), at
        assert ref_exec.matches(rec[at + "final_iter_nums"], fin, integers=True), at
    assert same(rec["givens_sin"], gsin) and same(rec["givens_cos"], gcos)
    y, before = cu.solve_krylov(rnc, basis, hess, fin)
    assert same(rec["solve_krylov/y"], y) and same(rec["solve_krylov/before_preconditioner"], before)
    assert ref_exec.matches(rec["basis"], basis.raw(), integers=True)
    if cu.is_scaled(storage):
        assert same(rec["scalars"], basis.scalars)


def test_the_case_set_exercises_what_it_is_there_for():
    """per the restatement's own count: steps with 0, 1 and 2 re-orthogonalisation passes (2 with a half or int16
    basis), a forced reset, and no loop test within 1e-6 (relative) of eta in either half mode"""
    passes = np.zeros(3, int)
    two = set()
    resets = 0
    for key in SOLVES:
        for half in ("truncate", "rne"):
            _, res = restated(key, half)
            passes += np.array(res["passes"])
            if res["passes"][2]:
                two.add(key.split("/")[1])
            resets += res["forced_resets"]
            t = res["trace"][np.isfinite(res["trace"])]
            assert len(t) == 0 or np.min(np.abs(t / cu.ETA - 1)) >= 1e-6, (key, half)
    assert np.all(passes > 0), passes
    assert two & {"reduce2", "ireduce2"}, two
    assert resets > 0


@pytest.mark.parametrize("key", [k for k in SOLVES if k.startswith("cd")])
def test_the_fixture_knows_which_iteration_counts_survive_a_reordered_sum(key):
    """The GPU tests hold a case to +-1 iteration of the sequential restatement only if the restatement's count stays
    within 1 when its sums are grouped by 64, by 1024 and added in the device's own order.  One case does not qualify:
    GMRES(30) on the 8^3 system with a half basis takes 81 iterations with sequential sums, 82 / 81 with grouped ones
    and 79 in the device's order (small differences grow by a factor of about 4 per iteration behind a half basis); it
    is held to +-1 of the last of these, and cd7_k30 and cd8_k30_r6, which qualify, stand in for it."""
    rec = REF["solves"][key]
    assert rec["reordered_iterations"] == cu.reordered_counts(*key.split("/"))
    # what they are held against: the same solve with sequential sums, which the driver pins in "truncate" mode
    assert rec["rne_iterations"] == cu.restated_solve(*key.split("/"), "rne")[1]["iterations"]
    assert cu.count_is_stable(rec) == (key != "cd8_k30/reduce2"), (key, rec["rne_iterations"], rec["reordered_iterations"])


def test_half_conversions():
    v = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -2.5e-5, 6.0e-8, 70000.0, -0.0, 0.333251953125])
    t = cu.half_bits_to_double(cu.float_to_half_bits(v, "truncate"), "truncate")
    r = cu.half_bits_to_double(cu.float_to_half_bits(v, "rne"), "rne")
    assert list(t) == [1.0, 1.0, 1.0 + 2.0 ** -10, -0.0, 0.0, np.inf, -0.0, 0.333251953125]
    assert list(r[:3]) == [1.0, 1.0, 1.0 + 2.0 ** -9] and r[3] != 0.0 and r[4] == 2.0 ** -24 and r[5] == np.inf


def test_compress_stores_what_a_basis_write_stores():
    """cu.compress, which the GPU tests compare the device's stored basis with, is the write the pinned kernels make:
    a half through cu.float_to_half_bits in either mode, an integer as the quotient by the scalar, cut"""
    v = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -2.5e-5, 6.0e-8, -0.0, 0.333251953125, -0.75])
    for mode in ("truncate", "rne"):
        assert np.array_equal(cu.compress(v, "reduce2", half=mode).view(np.uint16), cu.float_to_half_bits(v, mode))
    assert np.array_equal(cu.compress(v, "keep"), v.view(np.int64))
    assert np.array_equal(cu.compress(v, "reduce1"), v.astype(np.float32).view(np.int32))
    for storage in ("integer", "ireduce1", "ireduce2"):
        scalar = cu.correction(storage)
        assert np.array_equal(cu.compress(v, storage, scalar), np.trunc(v / scalar).astype(np.int64))


def test_the_device_s_sum_is_a_reordering_of_the_sequential_one():
    """cu.device_sum against cu.ssum in row order, which the driver pins: equal where every partial sum is exact
    (small integers), and within 2 gamma_(n-1) sum|p| otherwise -- each of two sums of n terms, in whatever order, is
    within gamma_(n-1) sum|p| of the exact one, gamma_k = k u / (1 - k u), u = 2^-53"""
    rng = np.random.default_rng(7)
    for n in (1, 63, 1025, 5000):           # one lane, one wave, more than one workgroup at 2 rows per lane
        for per_lane in (2, 4, 8):
            for dot in (False, True):
                whole = rng.integers(-1000, 1000, n).astype(np.float64)
                assert cu.device_sum(whole, per_lane, dot) == cu.ssum(whole) == whole.sum()
                assert cu.ssum(whole, ("device", per_lane), dot) == cu.device_sum(whole, per_lane, dot)
                p = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
                gamma = (n - 1) * 2.0 ** -53 / (1 - (n - 1) * 2.0 ** -53)
                assert abs(cu.device_sum(p, per_lane, dot) - cu.ssum(p)) <= 2 * gamma * np.abs(p).sum()


def test_the_driver_reproduces_the_fixture():
    """oracle/_ref/ref_driver, the reference executor itself, gives the fixture as it is committed: every recorded array
    of every case, the keys compared both ways.  One driver process; a missing driver fails wherever the reference or
    oracle/_ref/ is."""
    if ref_exec.may_skip():
        pytest.skip("neither the reference nor oracle/_ref/ is on this machine")
    assert ref_exec.difference_from_driver("cb_gmres", REF) is None


# ---- the C ABI and the Python layer, without a device -----------------------------------------------------------------

def code(fn, *args):
    import gkomi
    try:
        return fn(*args)
    except gkomi.GkomiError as e:
        return e.code


def test_abi_sizes_and_argument_checks(gk):
    assert [gk.cb_gmres_basis_bytes(10, 2, 4, s) for s in range(6)] == [800, 400, 200, 800, 400, 200]
    assert gk.cb_gmres_basis_bytes(10, 2, 4, 6) == 0 and gk.cb_gmres_workspace_bytes(10, 1, 4, 9) == 0
    assert gk.cb_gmres_workspace_bytes(1000, 1, 30, 2) < gk.cb_gmres_workspace_bytes(1000, 1, 30, 1) < \
        gk.cb_gmres_workspace_bytes(1000, 1, 30, 0)
    out = [np.zeros(1, np.int64) for _ in range(4)]
    assert code(gk.cb_gmres_geometry, 7, *out) == -1
    assert gk.cb_gmres_geometry(2, *out) == 0 and int(out[2][0]) == 8
    big = 1 << 26
    # restart / finish_arnoldi: bad storage, bad iter, krylov_dim out of range, no workspace
    assert code(gk.cb_gmres_restart_f64, None, 4, 1, 5, 6, 8, 8, 8, 8, 8, 8, 8, 8, 0, 8, big) == -1
    assert code(gk.cb_gmres_restart_f64, None, 4, 1, 5, 1, 8, 8, 8, 8, 8, 8, 8, 8, 0, None, 0) == -4
    fa = gk.cb_gmres_finish_arnoldi_f64
    assert code(fa, None, 4, 1, 5, 1, 8, 8, 8, 8, 5, 8, 8, 5, 8, None, 8, big) == -1
    assert code(fa, None, 4, 1, 5, 1, 8, 8, 8, 8, 5, 8, 8, -1, 8, None, 8, big) == -1
    assert code(fa, None, 4, 1, 5000, 1, 8, 8, 8, 8, 5, 8, 8, 0, 8, None, 8, big) == -1
    assert code(fa, None, 4, 1, 5, 1, 8, 8, 8, 8, 5, 8, 8, 0, 8, None, 8, 16) == -4
    assert code(fa, None, 4, 0, 5, 1, 8, 8, 8, 8, 5, 8, 8, 0, 8, None, 8, big) == 0
    assert code(gk.cb_gmres_solve_krylov_f64, None, 4, 1, 6, 8, 8, 8, 8, 4, 8, 8, 8) == -1
    info = np.zeros(5)
    sol = gk.cb_gmres_solve_f64_i32
    assert code(sol, None, 4, 1, 4, 8, 8, 8, 0, -1, None, None, 8, 8, 5, 6, 10, 1e-8, 0, 16, big, info) == -1
    assert code(sol, None, 4, 1, 4, 8, 8, 8, 0, -1, None, None, 8, 8, 0, 1, 10, 1e-8, 0, 16, big, info) == -1
    assert code(sol, None, 4, 1, 4, 8, 8, 8, 0, -1, None, None, 8, 8, 5, 1, 10, 1e-8, 0, 16, 64, info) == -4
    # more columns than a grid dimension holds: refused, not a failed launch
    assert code(gk.cb_gmres_restart_f64, None, 4, 65536, 5, 1, 8, 8, 8, 8, 8, 8, 8, 8, 0, 8, big) == -1
    assert code(fa, None, 4, 65536, 5, 1, 8, 8, 8, 8, 5, 8, 8, 0, 8, None, 8, big) == -1
    assert code(gk.cb_gmres_solve_krylov_f64, None, 4, 65536, 1, 8, 8, 8, 8, 4, 8, 8, 8) == -1
    assert code(sol, None, 4, 65536, 4, 8, 8, 8, 0, -1, None, None, 8, 8, 5, 1, 10, 1e-8, 0, 16, big, info) == -1
    assert code(gk.cb_gmres_solve_op_f64, None, 4, 1, None, None, None, None, 8, 8, 5, 1, 10, 1e-8, 0, 16, big, info) == -1


def test_python_layer_refuses_bad_parameters_before_touching_a_device(gk):
    from gkomi import solvers
    with pytest.raises(ValueError, match="storage"):
        solvers.cb_gmres_solve(gk, 4, None, None, None, None, storage="quarter")
    with pytest.raises(ValueError, match="krylov_dim"):
        solvers.cb_gmres_solve(gk, 4, None, None, None, None, krylov_dim=0)
    assert list(solvers.CB_GMRES_STORAGES) == list(cu.STORAGES)
