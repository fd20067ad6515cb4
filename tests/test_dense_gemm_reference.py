"""CPU checks of the dense GEMM yardstick: the numpy restatements (dense_gemm_util.py) reproduce the reference's own known
answers (tests/golden/dense_apply.json) and, on the GPU module's whole case list, the reference executor's Dense::apply
bit for bit (ordered) or within the derived bound (split); the recording that stands in for the driver on a machine
without the reference holds what the driver gives now; the C ABI's argument checks that return before any launch; the
mirror example and the shims compile; formats.Dense checks its arguments."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import dense_gemm_util as du
import ref_exec

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "repo-8852-ginkgo_amd")
G = json.load(open(os.path.join(HERE, "golden", "dense_apply.json")))


# ---- the restatements ------------------------------------------------------------------------------------------------
def test_restatements_reproduce_the_golden_answers():
    g = G["applies_to_dense"]
    assert np.array_equal(du.ordered(g["a"], g["b"]), np.array(g["expect"]))
    assert np.array_equal(du.split(g["a"], g["b"], chunk=1), np.array(g["expect"]))
    g = G["applies_linear_combination_to_dense"]
    assert np.array_equal(du.ordered(g["a"], g["b"], g["c"], g["alpha"], g["beta"]), np.array(g["expect"]))
    assert np.array_equal(du.split(g["a"], g["b"], g["c"], g["alpha"], g["beta"], chunk=2), np.array(g["expect"]))
    for key in ("square_matrix_is_transposable", "non_square_matrix_is_transposable"):
        assert np.array_equal(du.transpose(np.array(G[key]["in"])), np.array(G[key]["expect"]))


def test_restatements_keep_the_contract_of_the_header():
    """+0.0 start, beta == 0 multiplies, alpha * a rounded first, no padded product, the chunked order"""
    neg = np.array([[-0.0]])
    assert not np.signbit(du.ordered(neg, np.array([[1.0]]))[0, 0])                     # (+0.0) + (-0.0)
    c0 = np.array([[np.nan, np.inf, 1.0]])
    out = du.ordered(np.ones((1, 1)), np.ones((1, 3)), c0, 1.0, 0.0)
    assert np.isnan(out[0, 0]) and np.isnan(out[0, 1]) and out[0, 2] == 1.0
    a, b = np.array([[0.1]]), np.array([[0.3]])
    assert du.ordered(a, b, np.zeros((1, 1)), 0.1, 0.0)[0, 0] == (0.1 * 0.1) * 0.3 != 0.1 * (0.1 * 0.3)
    z = du.ordered(np.zeros((2, 3)), -np.ones((3, 2)), np.zeros((2, 2)), 1.0, -1.0)
    assert np.all(np.signbit(z))                                                        # -0.0 + (-0.0) ...: stays -0.0
    a, b = np.array([[1e16, 1.0, -1e16, 1.0]]), np.ones((4, 1))
    assert du.ordered(a, b)[0, 0] == 1.0 and du.split(a, b, chunk=2)[0, 0] == 0.0       # (1e16 + 1) + (-1e16 + 1)
    assert du.ordered(np.zeros((2, 0)), np.zeros((0, 3))).tolist() == [[0.0] * 3] * 2


@pytest.fixture(scope="module")
def geo(gk):
    return du.geometry(gk)


@pytest.fixture(scope="module")
def driver_results(geo):
    """(cases, their results from the driver -- or, where neither the reference nor oracle/_ref/ exists, from the
    recording, which is then only compared with the restatements)"""
    import test_dense_gemm_gpu as gpu
    cases = du.cases(geo)
    batch, idx = du.batch_of(cases)
    results = batch.run(gpu.RECORDING)
    return cases, [results[i] for i in idx]


def test_ordered_restatement_equals_the_reference_executor(driver_results):
    cases, results = driver_results
    assert sum(c.group == "tile" for c in cases) >= 3 * 48 and sum(c.group == "narrow" for c in cases) >= 3 * 60
    for c, r in zip(cases, results):
        assert "error" not in r, r
        if c.group != "split":
            ref_exec.assert_bits(r["x"].reshape(c.m, c.n + du.C_PAD), c.restated(), c.id)


def test_split_restatement_stays_within_the_bound_of_the_reference_executor(driver_results, geo):
    cases, results = driver_results
    seen = 0
    for c, r in zip(cases, results):
        if c.group != "split":
            continue
        seen += 1
        ref = r["x"].reshape(c.m, c.n + du.C_PAD)
        got = c.restated(du.split, chunk=geo["L"])
        a, b, c0 = c.data
        bound = du.split_bound(a, b, c0, c.alpha, c.beta)
        finite = np.isfinite(bound)
        with np.errstate(invalid="ignore"):
            err = np.abs(got[:, :c.n] - ref[:, :c.n])
        assert np.all(err[finite] <= bound[finite]), c.id
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[:, c.n:], ref[:, c.n:])
    assert seen == 3 * 16


def test_the_recorded_results_of_the_gpu_module_are_the_driver_s(geo):
    """tests/golden/ref_parity_dense_gpu.bin must have been recorded for the inputs the GPU module builds now, and hold
    what the driver gives for them now (the rule of test_ref_oracle_table.py)."""
    import test_dense_gemm_gpu as gpu
    batch, _ = du.batch_of(du.cases(geo))
    recorded = batch.unpack(ref_exec.read_recording(gpu.RECORDING, batch.pack()))
    assert os.path.getsize(gpu.RECORDING) < ref_exec.PART_BYTES and not os.path.exists(ref_exec._part(gpu.RECORDING, 1))
    if ref_exec.may_skip():
        return
    live = batch.run()
    for i, (want, got) in enumerate(zip(live, recorded)):
        assert sorted(want) == sorted(got) == ["x"], (i, want.get("error"), got.get("error"))
        ref_exec.assert_bits(got["x"], want["x"], f"case {i}")


# ---- the C ABI without a device --------------------------------------------------------------------------------------
def gemm(gk, m, n, k, a=8, a_stride=None, b=8, b_stride=None, c=8, c_stride=None, alpha=None, beta=None, mode=1, ws=None,
         ws_bytes=0):
    return gk.dense_gemm_f64(None, m, n, k, a, k if a_stride is None else a_stride, b, n if b_stride is None else b_stride, c,
                             n if c_stride is None else c_stride, alpha, beta, mode, ws, ws_bytes)


def test_abi_rejects_bad_arguments_before_any_launch(gk, geo):
    import gkomi
    bad = [dict(m=-1, n=1, k=1), dict(m=1, n=-1, k=1), dict(m=1, n=1, k=-1), dict(m=2, n=3, k=4, a_stride=3),
           dict(m=2, n=3, k=4, b_stride=2), dict(m=2, n=3, k=4, c_stride=2), dict(m=2, n=3, k=4, alpha=8),
           dict(m=2, n=3, k=4, beta=8), dict(m=2, n=3, k=4, mode=3), dict(m=2, n=3, k=4, mode=-1),
           dict(m=2, n=3, k=4, c=None), dict(m=2, n=3, k=4, a=None), dict(m=2, n=3, k=4, b=None)]
    for kw in bad:
        with pytest.raises(gkomi.GkomiError) as e:
            gemm(gk, **kw)
        assert e.value.code == -1, kw
    for kw in (dict(nrows=-1, ncols=2, in_stride=2, out_stride=0), dict(nrows=2, ncols=3, in_stride=2, out_stride=2),
               dict(nrows=2, ncols=3, in_stride=3, out_stride=1)):
        with pytest.raises(gkomi.GkomiError) as e:
            gk.dense_transpose_f64(None, kw["nrows"], kw["ncols"], 8, kw["in_stride"], 8, kw["out_stride"])
        assert e.value.code == -1, kw
    with pytest.raises(gkomi.GkomiError) as e:
        gk.dense_matrix_apply_cb(None, None, 1, None, 8, 1, None, 8, 1)
    assert e.value.code == -1


def test_abi_empty_shapes_return_without_a_launch(gk):
    assert gemm(gk, 0, 5, 3, a=None, b=None, c=None) == 0
    assert gemm(gk, 5, 0, 3, a=None, b=None, c=None) == 0
    assert gemm(gk, 0, 0, 0, a=None, b=None, c=None, mode=2) == 0
    assert gk.dense_transpose_f64(None, 0, 5, None, 5, None, 0) == 0
    assert gk.dense_transpose_f64(None, 5, 0, None, 0, None, 5) == 0


def test_abi_workspace(gk, geo):
    import gkomi
    big = geo["L"]
    assert gk.dense_gemm_workspace_bytes(3, 2, 5 * big + 3, 1) == 0
    assert gk.dense_gemm_workspace_bytes(3, 2, 5 * big + 3, 2) == 8 * 6 * 3 * 2
    assert gk.dense_gemm_workspace_bytes(3, 2, big, 2) == 8 * 3 * 2
    assert gk.dense_gemm_workspace_bytes(0, 2, big, 2) == 0
    for ws, nbytes in ((None, 0), (8, 8 * 6 * 3 * 2 - 1), (None, 1 << 20)):
        with pytest.raises(gkomi.GkomiError) as e:
            gemm(gk, 3, 2, 5 * big + 3, mode=2, ws=ws, ws_bytes=nbytes)
        assert e.value.code == -4, (ws, nbytes)


def test_plan_is_a_pure_function_with_the_fixed_conditions(gk, geo):
    big, wide = geo["L"], geo["narrow_n"]
    assert big > 0 and big & (big - 1) == 0
    shapes = [(m, n, k) for m in (1, 3, 16, 64, 65, 1000, 8192, 1 << 20) for n in (1, 2, 16, 17, 64, 1000, 8192)
              for k in (0, 1, big - 1, big, big + 1, 4 * big, 1000000)]
    plans = {}
    for m, n, k in shapes:
        ordered = 2 if n <= wide else 1
        assert gk.dense_gemm_plan(m, n, k, 1) == ordered
        assert gk.dense_gemm_plan(m, n, k, 2) == 3
        auto = gk.dense_gemm_plan(m, n, k, 0)
        assert auto in (ordered, 3)
        if k <= big:
            assert auto != 3
        if auto == 3:
            assert gk.dense_gemm_workspace_bytes(m, n, k, 0) == 8 * -(-k // big) * m * n
        else:
            assert gk.dense_gemm_workspace_bytes(m, n, k, 0) == 0
        plans[(m, n, k)] = auto
    assert plans[(8192, 8192, 1000000)] != 3          # m n alone fills the device
    assert all(gk.dense_gemm_plan(m, n, k, 0) == p for (m, n, k), p in plans.items())
    assert gk.dense_gemm_plan(-1, 1, 1, 0) < 0 and gk.dense_gemm_plan(1, 1, 1, 5) < 0


# ---- the layers above ------------------------------------------------------------------------------------------------
def test_mirror_example_compiles():
    src = open(os.path.join(PKG, "examples", "dense_operator_mirror.cpp")).read()
    for needle in ("->transpose()", "gko::solver::Cg<double>", "gko::solver::Bicg<double>", "gko::lend(alpha)"):
        assert needle in src
    r = subprocess.run(["make", "-C", os.path.join(PKG, "examples"), "bin/dense_operator_mirror"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def build_dense_shim_smoke(tmp_path):
    """shims/hip/matrix/dense_kernels.hip.cpp against the mirror, linked with shims/test/shim_smoke11.cpp"""
    obj, exe = tmp_path / "dense_kernels.o", tmp_path / "shim_smoke11"
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Wno-unused-parameter", f"-I{ROOT}/include", f"-I{PKG}/include", "-include",
                        os.path.join(ROOT, "shims", "test", "prelude_mirror.hpp"), "-c",
                        os.path.join(ROOT, "shims", "hip", "matrix", "dense_kernels.hip.cpp"), "-o", str(obj)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(["g++", "-std=c++14", f"-I{ROOT}/include", f"-I{PKG}/include", f"-I{ROOT}/shims/test",
                        os.path.join(ROOT, "shims", "test", "shim_smoke11.cpp"), str(obj), "-o", str(exe), f"-L{PKG}/lib", "-lgkomi",
                        f"-Wl,-rpath,{PKG}/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_dense_gemm_shims_compile_against_the_mirror(tmp_path):
    assert os.path.exists(build_dense_shim_smoke(tmp_path))
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("dense::simple_apply", "dense::apply", "dense::transpose", "dense::conj_transpose", "shim_smoke11.cpp"):
        assert name in text, name


def test_formats_dense_checks_its_arguments(gk):
    import torch
    from gkomi import formats
    a = torch.zeros((4, 3), dtype=torch.float64)
    d = formats.Dense(gk, a)
    assert (d.nrows, d.ncols, d.stride, d.storage_bytes()) == (4, 3, 3, 96)
    assert formats.Dense(gk, torch.zeros((4, 5), dtype=torch.float64)[:, :3]).stride == 5
    for bad in (torch.zeros((4, 3), dtype=torch.float32), torch.zeros(4, dtype=torch.float64), np.zeros((4, 3))):
        with pytest.raises(TypeError):
            formats.Dense(gk, bad)
    with pytest.raises(ValueError):
        formats.Dense(gk, torch.zeros((3, 4), dtype=torch.float64).t())
    b, x = torch.zeros((3, 2), dtype=torch.float64), torch.zeros((4, 2), dtype=torch.float64)
    for args, kw, err in (((torch.zeros((2, 2), dtype=torch.float64), x), {}, ValueError),
                          ((b, torch.zeros((3, 2), dtype=torch.float64)), {}, ValueError),
                          ((b, torch.zeros((4, 1), dtype=torch.float64)), {}, ValueError),
                          ((b, x), {"alpha": 1.0}, ValueError), ((b, x), {"beta": 1.0}, ValueError),
                          ((b, x), {"mode": 3}, ValueError), ((b.float(), x), {}, TypeError),
                          ((b, torch.zeros(4, dtype=torch.float64)), {}, TypeError)):
        with pytest.raises(err):
            d.apply(*args, **kw)
    cb = d.callback()
    assert (cb.ctx.nrows, cb.ctx.ncols, cb.ctx.stride, cb.ctx.mode) == (4, 3, 3, 1) and cb.fn
