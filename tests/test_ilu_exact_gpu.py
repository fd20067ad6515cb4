"""Exact ILU(0) / IC(0) on the device against the plain-Python restatement of the reference kernels
(tests/ilu_exact_util.py): bit for bit through the C ABI, the Python layer, the C++ mirror and the shims."""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import gkomi
import ilu_exact_util as xu
import matgen
from gkomi import solvers
from gpu_util import dev, host, stream_ptr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "repo-8852-ginkgo_amd")
G = json.load(open(os.path.join(HERE, "golden", "ilu_exact.json")))

# the constants of csrc/ilu.hip as built (gkomi_ilu_tuning): a row of at most BIN_SHORT entries is factorized by 8
# lanes, one of at most BIN_WAVE by a wave, one of at most BIN_LDS by a workgroup out of LDS, a longer one by a
# workgroup in memory; a level of at most NARROW_LEVEL_ROWS rows is walked by the single-workgroup kernel
BIN_SHORT, BIN_WAVE, BIN_LDS, NARROW_LEVEL_ROWS = 32, 512, 1024, 16


def read_square(name):
    kind, nr, nc, rows, cols, vals = matgen.read_mtx(os.path.join(HERE, "golden", name))
    assert kind == "coo" and nr == nc
    return (nr,) + tuple(matgen.coo_to_csr(nr, rows, cols, vals))


def mtx(name):
    nr, rp, ci, v = read_square(name)
    return xu.add_diagonal_elements(xu.sort_by_column_index((rp, ci, v)))


def grid(gen, *dims):
    n, rp, ci, v = gen(*dims)
    return xu.sort_by_column_index((rp, ci, v))


CASES = {
    "golden_small": lambda: xu.dense_to_csr(G["ilu"]["small"]["A"]),
    "golden_small2_zero_diagonal": lambda: xu.add_diagonal_elements(xu.dense_to_csr(G["ilu"]["small2"]["A"])),
    "golden_big": lambda: xu.dense_to_csr(G["ilu"]["big"]["A"]),
    "golden_big_nodiag": lambda: xu.add_diagonal_elements(xu.dense_to_csr(G["ilu"]["big_nodiag"]["A"])),
    "golden_ic_banded": lambda: xu.dense_to_csr(G["ic"]["banded"]["A"]),
    "golden_ic_system": lambda: xu.add_diagonal_elements(xu.dense_to_csr(G["ic"]["system"]["A"])),
    # u_11 = 0: l_21 = 1 / 0, then inf - inf
    "zero_pivot": lambda: xu.dense_to_csr([[1, 1, 0, 2], [1, 1, 1, 0], [0, 1, 1, 1], [1, 0, 1, 0]], keep_zeros=True),
    "ani1": lambda: mtx("ani1.mtx"),
    "ani4": lambda: mtx("ani4.mtx"),
    "tridiagonal_600": lambda: xu.tridiagonal(600),                  # 600 levels of one row
    "blocks_2x2_3000": lambda: xu.diagonal_blocks_2x2(3000),         # two levels of 3000 rows
    "poisson_2d_40": lambda: grid(matgen.poisson_2d_5pt, 40),
    "poisson_3d_9": lambda: grid(matgen.poisson_3d_7pt, 9),
    "dense_48": lambda: xu.dense_matrix(48, 11),                     # rows longer than BIN_SHORT, 48 levels
    "arrow_700": lambda: xu.arrow(700),                              # last row longer than BIN_WAVE
    "arrow_1100": lambda: xu.arrow(BIN_LDS + 76),                    # last row longer than BIN_LDS
    "random_400": lambda: xu.random_dominant(400, 1, 60, 17),
    # levels of NARROW_LEVEL_ROWS and NARROW_LEVEL_ROWS + 1 rows in turn
    "level_widths": lambda: xu.level_widths([NARROW_LEVEL_ROWS, NARROW_LEVEL_ROWS + 1, NARROW_LEVEL_ROWS,
                                             NARROW_LEVEL_ROWS + 1, 1, 40]),
    # a wide level that holds a row longer than BIN_LDS and one longer than BIN_WAVE
    "wide_level_long_rows": lambda: xu.wide_level_with_long_rows(1300, 20, [BIN_LDS + 76, BIN_WAVE + 88]),
    # 40 diagonal rows, then ONE level of NARROW_LEVEL_ROWS + 1 rows over them: the first with BIN_SHORT + 1 lower
    # entries (a wave in a wide level, also once the pattern is made symmetric for IC), the others with two
    "wide_level_wave_row": lambda: xu.from_rows(
        [{i: 4.0 + 0.125 * i} for i in range(40)] +
        [{**{j: -0.5 - 0.015625 * (j + r) for j in range(r, r + (BIN_SHORT + 1 if r == 0 else 2))}, 40 + r: 6.0 + r}
         for r in range(NARROW_LEVEL_ROWS + 1)]),
    # one run of narrow levels whose widest level is neither its first nor its last
    "levels_1_5_3": lambda: xu.level_widths([1, 5, 3]),
    "n1": lambda: xu.dense_to_csr([[4.0]]),
    "n0": lambda: (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)),
}
# IC needs SPD input except where the reference's own test feeds the matrix as it is
IC_AS_IS = {"golden_ic_banded", "golden_ic_system", "zero_pivot", "n1", "n0"}


@functools.lru_cache(maxsize=None)
def case(name, ic):
    """the matrix and its factorization by the restatement; computed once, never written to"""
    m = CASES[name]()
    if ic and name not in IC_AS_IS:
        m = xu.spd_version(m)
    want = xu.ic_compute(m) if ic else xu.compute_lu(m)
    for a in m + want:
        a.setflags(write=False)
    return m, want


def level_widths_of(m):
    """rows per dependency level, from the entries left of the diagonal"""
    rp, ci, _ = m
    n = len(rp) - 1
    level = np.zeros(n, np.int64)
    for r in range(n):
        deps = [level[c] for c in ci[rp[r]:rp[r + 1]] if c < r]
        level[r] = max(deps) + 1 if deps else 0
    return np.bincount(level) if n else np.zeros(0, np.int64)


def analyse(gk, n, rpd, cid):
    nb = gk.ilu_analysis_workspace_bytes(n)
    ws = torch.zeros(max(nb, 8), dtype=torch.uint8, device="cuda:0")
    out = (ctypes.c_int64 * 6)()
    gk.ilu_analyse_i32(stream_ptr(), n, rpd, cid, ws, nb, ctypes.addressof(out))
    return ws, nb, dict(zip(("nlevels", "longest_row", "widest_level", "launches", "narrow_runs", "nnz"), out))


def factorize(gk, m, ic, analysis=None):
    rp, ci, v = m
    n = len(rp) - 1
    rpd, cid, vd = dev(rp), dev(ci), dev(v)
    ws, nb, info = analysis if analysis is not None else analyse(gk, n, rpd, cid)
    (gk.ic_compute_f64_i32 if ic else gk.ilu_compute_lu_f64_i32)(stream_ptr(), n, rpd, cid, vd, ws, nb)
    torch.cuda.synchronize()
    return host(vd), (ws, nb, info)


def test_constants_are_the_library_s(gk):
    out = (ctypes.c_int64 * 4)()
    gk.ilu_tuning(ctypes.addressof(out))
    assert list(out) == [BIN_SHORT, BIN_WAVE, BIN_LDS, NARROW_LEVEL_ROWS]


@pytest.mark.parametrize("ic", [False, True], ids=["ilu", "ic"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_factors_are_the_restatement_s_bits(gk, name, ic):
    m, want = case(name, ic)
    got, (_, _, info) = factorize(gk, m, ic)
    n = len(m[0]) - 1
    assert info["nnz"] == len(m[2]) and info["longest_row"] == (int(np.diff(m[0]).max()) if n else 0)
    widths = level_widths_of(m)
    assert info["nlevels"] == len(widths) and info["widest_level"] == (int(widths.max()) if n else 0)
    bad = [i for i in range(len(got)) if not xu.bits_equal(got[i:i + 1], want[2][i:i + 1])]
    print(name, "ic" if ic else "ilu", info, "entries that differ:", len(bad), bad[:8])
    assert xu.bits_equal(got, want[2])
    if name == "zero_pivot" and not ic:
        assert np.isinf(got).any() and np.isnan(got).any()


def test_cases_reach_every_path(gk):
    """the cases above sit on both sides of every boundary of the kernels as built"""
    def info(name):
        m, _ = case(name, False)
        return analyse(gk, len(m[0]) - 1, dev(m[0]), dev(m[1]))[2]
    assert info("tridiagonal_600") == dict(nlevels=600, longest_row=3, widest_level=1, launches=1, narrow_runs=1, nnz=1798)
    b = info("blocks_2x2_3000")
    assert (b["nlevels"], b["widest_level"], b["launches"], b["narrow_runs"]) == (2, 3000, 2, 0)
    w = info("level_widths")
    assert (w["nlevels"], w["widest_level"], w["launches"], w["narrow_runs"]) == (6, 40, 6, 3)
    assert BIN_SHORT < info("dense_48")["longest_row"] <= BIN_WAVE and info("dense_48")["nlevels"] == 48
    assert BIN_WAVE < info("arrow_700")["longest_row"] <= BIN_LDS
    assert info("arrow_1100")["longest_row"] > BIN_LDS
    assert info("levels_1_5_3") == dict(nlevels=3, longest_row=3, widest_level=5, launches=1, narrow_runs=1, nnz=24)
    lw = info("wide_level_long_rows")
    assert lw["longest_row"] > BIN_LDS and lw["widest_level"] > NARROW_LEVEL_ROWS
    # two wide levels, each with short rows and rows for a workgroup: a launch per bin, not per level
    assert (lw["nlevels"], lw["narrow_runs"], lw["launches"]) == (2, 0, 4)
    m, _ = case("wide_level_long_rows", False)
    lens = np.diff(m[0])[3:23]          # the 20 rows of the wide level
    assert (lens > BIN_LDS).any() and ((lens > BIN_WAVE) & (lens <= BIN_LDS)).any() and (lens <= BIN_SHORT).any()
    # a row for a wave in a wide level, in the pattern ILU sees and in the symmetric one IC sees
    for ic in (False, True):
        m, _ = case("wide_level_wave_row", ic)
        widths, lens = level_widths_of(m), np.diff(m[0])
        assert list(widths) == [40, NARROW_LEVEL_ROWS + 1] and BIN_SHORT < lens[40] <= BIN_WAVE and (lens[41:] <= BIN_SHORT).all()


@pytest.mark.parametrize("ic", [False, True], ids=["ilu", "ic"])
def test_refactorization_reuses_the_analysis(gk, ic):
    m, want = case("poisson_2d_40", ic)
    got, analysis = factorize(gk, m, ic)
    assert xu.bits_equal(got, want[2])
    rng = np.random.default_rng(5)
    v2 = m[2] * rng.uniform(0.75, 1.0, len(m[2]))
    m2 = (m[0], m[1], v2)
    if ic:
        m2 = xu.spd_version(m2)
        assert np.array_equal(m2[1], m[1])
    want2 = xu.ic_compute(m2) if ic else xu.compute_lu(m2)
    got2, _ = factorize(gk, m2, ic, analysis)
    assert xu.bits_equal(got2, want2[2]) and not xu.bits_equal(got2, got)


@pytest.mark.parametrize("what", ["missing_diagonal", "unsorted_row"])
def test_bad_input_is_rejected_before_any_numeric_launch(gk, what):
    rows = xu.to_rows(xu.tridiagonal(50))
    if what == "missing_diagonal":
        del rows[20][20]
        rp, ci, v = xu.from_rows(rows)
    else:
        rp, ci, v = xu.from_rows(rows)
        ci, v = ci.copy(), v.copy()
        b = rp[30]
        ci[b], ci[b + 1] = ci[b + 1], ci[b]
    n = 50
    rpd, cid, vd = dev(rp), dev(ci), dev(v)
    nb = gk.ilu_analysis_workspace_bytes(n)
    ws = torch.zeros(nb, dtype=torch.uint8, device="cuda:0")
    out = (ctypes.c_int64 * 6)()
    with pytest.raises(gkomi.GkomiError) as e:
        gk.ilu_analyse_i32(stream_ptr(), n, rpd, cid, ws, nb, ctypes.addressof(out))
    assert e.value.code == -1
    for fn in (gk.ilu_compute_lu_f64_i32, gk.ic_compute_f64_i32):
        with pytest.raises(gkomi.GkomiError) as e:
            fn(stream_ptr(), n, rpd, cid, vd, ws, nb)
        assert e.value.code == -1
    torch.cuda.synchronize()
    assert xu.bits_equal(host(vd), v)
    # a workspace that is too small
    with pytest.raises(gkomi.GkomiError) as e:
        gk.ilu_analyse_i32(stream_ptr(), n, rpd, cid, ws, nb - 1, ctypes.addressof(out))
    assert e.value.code == -4


def test_a_workspace_analysed_for_another_size_is_rejected(gk):
    rp, ci, v = xu.tridiagonal(50)
    ws, nb, _ = analyse(gk, 50, dev(rp), dev(ci))
    rp2, ci2, v2 = xu.tridiagonal(49)
    vd = dev(v2)
    for fn in (gk.ilu_compute_lu_f64_i32, gk.ic_compute_f64_i32):
        with pytest.raises(gkomi.GkomiError) as e:
            fn(stream_ptr(), 49, dev(rp2), dev(ci2), vd, ws, nb)
        assert e.value.code == -1
    torch.cuda.synchronize()
    assert xu.bits_equal(host(vd), v2)


def csr_host(f):
    torch.cuda.synchronize()
    return host(f[0]), host(f[1]), host(f[2])


def same_csr(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and xu.bits_equal(got[2], want[2])


def unsorted_without_some_diagonals():
    """ani1 with every row reversed and the diagonal of every fifth row removed: the whole generate chain"""
    nr, rp, ci, v = read_square("ani1.mtx")
    rows = xu.to_rows((rp, ci, v))
    for i in range(0, nr, 5):
        rows[i].pop(i, None)
    nrp, nci, nv = [0], [], []
    for r in rows:
        for c in sorted(r, reverse=True):
            nci.append(c); nv.append(r[c])
        nrp.append(len(nci))
    return nr, np.array(nrp, np.int32), np.array(nci, np.int32), np.array(nv, np.float64)


def test_ilu_generate_splits_into_the_restatement_s_factors(gk):
    n, rp, ci, v = unsorted_without_some_diagonals()
    p = solvers.ilu_generate(gk, n, dev(rp), dev(ci), dev(v))
    L, U = xu.ilu_generate((rp, ci, v))
    assert same_csr(csr_host(p.L), L) and same_csr(csr_host(p.U), U)


def test_ic_generate_splits_into_the_restatement_s_factors(gk):
    m, _ = case("ani1", True)
    n = len(m[0]) - 1
    p = solvers.ic_generate(gk, n, dev(m[0]), dev(m[1]), dev(m[2]))
    L, Lt = xu.ic_generate(m)
    assert same_csr(csr_host(p.L), L) and same_csr(csr_host(p.Lt), Lt)


def spd_tridiagonal(n):
    return xu.from_rows([{j: (2.0 if j == i else -1.0) for j in (i - 1, i, i + 1) if 0 <= j < n} for i in range(n)])


def test_cg_with_exact_ic_of_a_tridiagonal_matrix(gk):
    """IC(0) of a tridiagonal SPD matrix is its Cholesky factor: one iteration in exact arithmetic, one for rounding"""
    n = 500
    rp, ci, v = spd_tridiagonal(n)
    rpd, cid, vd = dev(rp), dev(ci), dev(v)
    b = dev(np.cos(0.01 * np.arange(n)))
    pre = solvers.ic_generate(gk, n, rpd, cid, vd)
    r = solvers.cg_solve(gk, n, rpd, cid, vd, b, max_iters=50, reduction=1e-10, precond=pre)
    print("cg + ic:", r["iterations"], r.get("residual_norm"))
    assert r["converged"] and r["iterations"] <= 2


def test_gmres_with_exact_ilu_of_a_tridiagonal_matrix(gk):
    n = 500
    rp, ci, v = spd_tridiagonal(n)
    rpd, cid, vd = dev(rp), dev(ci), dev(v)
    b = dev(np.cos(0.01 * np.arange(n)))
    pre = solvers.ilu_generate(gk, n, rpd, cid, vd)
    r = solvers.gmres_solve(gk, n, rpd, cid, vd, b, krylov_dim=10, max_iters=50, reduction=1e-10, precond=pre)
    print("gmres + ilu:", r["iterations"])
    assert r["converged"] and r["iterations"] <= 2


# ---- the mirror and the shims ----------------------------------------------------------------------------------

def test_mirror_example(gk):
    ex = os.path.join(PKG, "examples")
    r = subprocess.run(["make", "-C", ex, "bin/ilu_exact_mirror"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(ex, "bin", "ilu_exact_mirror")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    checks = [ln.split(": ") for ln in r.stdout.splitlines() if ln.startswith("check ")]
    assert len(checks) == 7 and all(c[1] == "ok" for c in checks), r.stdout
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ilu_exact_mirror:")]
    kv = dict(t.split("=") for t in line[0].split()[1:])
    assert int(kv["rows"]) == 576 and 0 < int(kv["cg_ic_iterations"]) < int(kv["cg_plain_iterations"])


MIRROR_SRC = r"""
#include <ginkgo/ginkgo.hpp>
#include <cstdio>
#include <fstream>
#include <iostream>
using csr = gko::matrix::Csr<double, gko::int32>;
using dense = gko::matrix::Dense<double>;
static void print(const char* name, const csr* m)
{
    auto exec = m->get_executor();
    std::vector<double> v(m->get_num_stored_elements());
    exec->get_master()->copy_from(exec.get(), v.size(), m->get_const_values(), v.data());
    std::printf("%s", name);
    for (double x : v) std::printf(" %a", x);
    std::printf("\n");
}
int main()
{
    auto exec = gko::HipExecutor::create(0, gko::ReferenceExecutor::create());
    auto A = gko::share(gko::read<csr>(std::ifstream("data/A.mtx"), exec));
    auto b = gko::read<dense>(std::ifstream("data/b.mtx"), exec);
    auto x = gko::read<dense>(std::ifstream("data/x0.mtx"), exec);
    auto fact = gko::factorization::Ilu<double, gko::int32>::build().on(exec)->generate(A);
    print("L", fact->get_l_factor().get());
    print("U", fact->get_u_factor().get());
    auto solver = gko::solver::Gmres<double>::build()
                      .with_criteria(gko::stop::Iteration::build().with_max_iters(100u).on(exec),
                                     gko::stop::ResidualNorm<double>::build().with_reduction_factor(1e-13).on(exec))
                      .with_preconditioner(gko::preconditioner::Ilu<double, gko::int32>::build()
                                               .with_factorization_factory(gko::factorization::Ilu<double, gko::int32>::build().on(exec))
                                               .on(exec))
                      .on(exec)
                      ->generate(A);
    solver->apply(gko::lend(b), gko::lend(x));
    std::cout << "x:" << std::endl;
    gko::write(std::cout, gko::lend(x));
    return 0;
}
"""


def test_mirror_factors_are_the_abi_s_and_the_preconditioner_solves_simple_solver(gk, tmp_path):
    import shutil
    (tmp_path / "data").mkdir()
    for name in ("A", "b", "x0"):
        shutil.copy(os.path.join(HERE, "golden", f"simple_solver_{name}.mtx"), tmp_path / "data" / f"{name}.mtx")
    src, exe = tmp_path / "mirror.cpp", tmp_path / "mirror"
    src.write_text(MIRROR_SRC)
    r = subprocess.run(["g++", "-O1", "-std=c++17", f"-I{PKG}/include", str(src), "-o", str(exe), f"-L{PKG}/lib", "-lgkomi",
                        f"-Wl,-rpath,{PKG}/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    got = {ln.split()[0]: np.array([float.fromhex(t) for t in ln.split()[1:]]) for ln in lines if ln[:2] in ("L ", "U ")}
    # the same factors through the C ABI
    n, rp, ci, v = read_square("simple_solver_A.mtx")
    m = xu.add_diagonal_elements(xu.sort_by_column_index((rp, ci, v)))
    vals, _ = factorize(gk, m, False)
    L, U = xu.initialize_l_u((m[0], m[1], vals))
    assert xu.bits_equal(got["L"], L[2]) and xu.bits_equal(got["U"], U[2])
    # the solution of doc/results.dox to its six printed digits, as tests/test_cpp_mirror.py reads it
    g = json.load(open(os.path.join(HERE, "golden", "cg.json")))["simple_solver"]
    i = lines.index("x:")
    assert lines[i + 2].split() == ["19", "1"]
    x = np.array([float(t) for t in lines[i + 3:i + 22]])
    assert np.array_equal(x, np.array(g["expect_x"]))


def test_exact_factorization_shims_run_on_the_device(tmp_path):
    from test_ilu_exact_reference import build_ilu_shim_smoke
    run = subprocess.run([build_ilu_shim_smoke(tmp_path)], capture_output=True, text=True)
    ran = {t[1]: t[2] for t in (ln.split() for ln in run.stdout.splitlines()) if len(t) == 3 and t[0] == "ran"}
    assert run.returncode == 0, run.stdout + run.stderr
    assert ran == {k: "ok" for k in ("ilu_factorization::compute_lu", "ic_factorization::compute")}, ran
