"""CPU checks of the IDR(s) yardstick: the numpy restatement (idr_util.py) solves the reference's own known-answer
systems (tests/golden/idr.json) to the reference's tolerances, whatever subspace it is given."""
import json
import os

import numpy as np
import pytest

import idr_util
import matgen
from krylov_util import dense_to_csr

G = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "idr.json")))


@pytest.mark.parametrize("seed", [15, 4])
@pytest.mark.parametrize("case", G["solves"], ids=lambda c: c["name"])
def test_restatement_solves_the_known_answers(oracle, case, seed):
    n, rp, ci, v = dense_to_csr(case["A"])
    b = np.array(case["b"], np.float64)
    p = idr_util.subspace(G["subspace_dim"], n, seed)
    res = idr_util.solve(idr_util.csr_apply(oracle, n, rp, ci, v), b, p, subspace_dim=G["subspace_dim"],
                         kappa=G["kappa"], max_iters=case["max_iters"], reduction=case["reduction"])
    err = matgen.rel_err(res["x"], np.array(case["expect_x"]))
    print(case["name"], seed, "iterations", res["iterations"], "rel err", err)
    assert err <= case["tol"], (res["iterations"], err)
    # initialize left the rows of P orthonormal
    assert np.allclose(p @ p.T, np.eye(G["subspace_dim"]), atol=1e-14)


def test_restatement_runs_in_extended_precision(oracle):
    case = G["solves"][2]
    n, rp, ci, v = dense_to_csr(case["A"])
    b = np.array(case["b"], np.longdouble)
    p = idr_util.subspace(2, n, 15).astype(np.longdouble)
    res = idr_util.solve(idr_util.csr_apply(oracle, n, rp, ci, v), b, p, max_iters=case["max_iters"],
                         reduction=case["reduction"])
    assert res["x"].dtype == np.longdouble
    assert matgen.rel_err(res["x"].astype(np.float64), np.array(case["expect_x"])) <= case["tol"]


def test_mirror_example_compiles_with_solver_idr():
    """examples/solve_mtx.cpp builds gko::solver::Idr<double> with every factory parameter of the mirror"""
    import subprocess
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "repo-8852-ginkgo_amd")
    src = open(os.path.join(pkg, "examples", "solve_mtx.cpp")).read()
    for needle in ("gko::solver::Idr<double>", "with_subspace_dim", "with_kappa", "with_deterministic"):
        assert needle in src
    r = subprocess.run(["make", "-C", os.path.join(pkg, "examples"), "bin/solve_mtx"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_mirror_idr_factory_on_the_host():
    """with_complex_subspace(true) throws NotSupported, the getters return what the factory was given"""
    import subprocess
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "repo-8852-ginkgo_amd", "examples")
    r = subprocess.run(["make", "-C", ex, "bin/idr_mirror"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(ex, "bin", "idr_mirror")], capture_output=True, text=True)
    assert r.returncode == 0 and "idr factory ok" in r.stdout, r.stdout + r.stderr


def build_idr_shim_smoke(tmp_path):
    """shims/hip/solver/idr_kernels.hip.cpp against the mirror, linked with shims/test/shim_smoke3.cpp"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "repo-8852-ginkgo_amd")
    obj, exe = tmp_path / "idr_kernels.o", tmp_path / "shim_smoke3"
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Wno-unused-parameter", f"-I{root}/include", f"-I{pkg}/include", "-include",
                        os.path.join(root, "shims", "test", "prelude_mirror.hpp"), "-c",
                        os.path.join(root, "shims", "hip", "solver", "idr_kernels.hip.cpp"), "-o", str(obj)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(["g++", "-std=c++14", f"-I{root}/include", f"-I{pkg}/include", f"-I{root}/shims/test",
                        os.path.join(root, "shims", "test", "shim_smoke3.cpp"), str(obj), "-o", str(exe), f"-L{pkg}/lib", "-lgkomi",
                        f"-Wl,-rpath,{pkg}/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_idr_shim_compiles_against_the_mirror(tmp_path):
    assert os.path.exists(build_idr_shim_smoke(tmp_path))


@pytest.mark.parametrize("s", [1, 4])
def test_the_departures_from_idr_cpp_cost_at_most_one_iteration(oracle, s):
    """idr.cpp hands its criterion the norm taken before the omega step, so it notices convergence one outer iteration
    after the residual got there, or in the same one; on this system the drivers' order (literal=False) does not need more"""
    n, rp, ci, v = matgen.poisson_3d_7pt(8)
    v = v.copy()
    rows = np.repeat(np.arange(n), np.diff(rp))
    v[ci == rows - 1] -= 0.5
    v[ci == rows] += 0.5
    apply = idr_util.csr_apply(oracle, n, rp, ci, v)
    b = apply(np.sin(0.3 * np.arange(n)).reshape(n, 1))
    run = lambda literal: idr_util.solve(apply, b.copy(), idr_util.subspace(s, n, 15), subspace_dim=s, max_iters=500,
                                         reduction=1e-10, literal=literal)
    ref, ours = run(True), run(False)
    assert ref["converged"] and ours["converged"]
    assert ours["iterations"] <= ref["iterations"] <= ours["iterations"] + 1, (ref["iterations"], ours["iterations"])
    assert np.linalg.norm(ours["residual"]) <= 1e-10 * np.linalg.norm(b)
