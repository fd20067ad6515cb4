"""Dense::apply (gkomi_dense_gemm_f64) and Dense::transpose on the device.

Ordered kernels: bit for bit the reference executor's Dense::apply on the whole c buffer, padding included.  The
expected values come from oracle/_ref/ref_driver where it exists (`spmv`, fmt = DENSE), else from its recorded output
tests/golden/ref_parity_dense_gpu.bin (`python tests/test_dense_gemm_gpu.py record` writes it; keyed by the input hash;
tests/test_dense_gemm_reference.py checks it against the driver).  Split: bit for bit the chunked restatement, and
within (k + 2) 2^-52 S of the reference.  The shapes sit on the edges of the kernels' geometry, which is read from the
library (gkomi_dense_gemm_geometry, gkomi_dense_gemm_split_chunk)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch   # before the library is loaded below (the case list needs its geometry): both then share torch's HIP runtime

import dense_gemm_util as du
import ref_exec

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "repo-8852-ginkgo_amd")
RECORDING = os.path.join(HERE, "golden", "ref_parity_dense_gpu.bin")
G = json.load(open(os.path.join(HERE, "golden", "dense_apply.json")))

pytestmark = pytest.mark.gpu


def library():
    if PKG not in sys.path:     # run as a script (record): no conftest has put the package on the path
        sys.path.insert(0, PKG)
    import gkomi
    return gkomi.lib()


@functools.lru_cache(maxsize=None)
def case_list():
    return du.cases(du.geometry(library()))


@functools.lru_cache(maxsize=None)
def reference():
    """id -> the reference's whole c buffer, computed (or read) once for the module"""
    batch, idx = du.batch_of(case_list())
    results = batch.run(RECORDING)
    out = {}
    for c, i in zip(case_list(), idx):
        assert "error" not in results[i], results[i]
        out[c.id] = results[i]["x"].reshape(c.m, c.n + du.C_PAD)
    return out


def ids(group):
    return [c.id for c in case_list() if c.group in group]


def case(cid):
    return next(c for c in case_list() if c.id == cid)


def padded(a, pad, fill=du.FILL):
    """a device buffer with `pad` more columns than the 2-d array `a`, and the view of `a` in it"""
    from gpu_util import dev
    buf = torch.full((a.shape[0], a.shape[1] + pad), fill, dtype=torch.float64, device="cuda:0")
    view = buf[:, :a.shape[1]]
    if a.size:
        view.copy_(dev(a))
    return buf, view


def run(gk, c, mode):
    """the whole c buffer after formats.Dense.apply on strided operands"""
    from gkomi import formats
    from gpu_util import dev, host
    a, b, _ = c.data
    _, av = padded(a, du.A_PAD)
    _, bv = padded(b, du.B_PAD)
    cbuf = dev(c.c_buffer())
    cv = cbuf[:, :c.n]
    formats.Dense(gk, av).apply(bv, cv, alpha=c.alpha, beta=c.beta, mode=mode)
    torch.cuda.synchronize()
    return host(cbuf)


def check_split(gk, c, got):
    geo = du.geometry(gk)
    want = split_restated(c.id, geo["L"])
    ref_exec.assert_bits(got, want, c.id + " against the chunked restatement")
    a, b, c0 = c.data
    bound = du.split_bound(a, b, c0, c.alpha, c.beta)
    ref = reference()[c.id][:, :c.n]
    finite = np.isfinite(bound)
    with np.errstate(invalid="ignore"):
        err = np.abs(got[:, :c.n] - ref)
    worst = float(np.max(err[finite] / np.where(bound[finite] > 0, bound[finite], 1.0))) if finite.any() else 0.0
    print(f"{c.id}: max |got - ref| / bound = {worst:.3g}")
    assert np.all(err[finite] <= bound[finite]), (c.id, worst)
    ref_exec.assert_bits(np.isnan(got), np.isnan(reference()[c.id]), c.id + " NaN pattern")


@functools.lru_cache(maxsize=None)
def split_restated(cid, chunk):
    return case(cid).restated(du.split, chunk=chunk)


# ---- ordered: the reference's bits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ids(("tile", "narrow")))
def test_ordered_equals_the_reference(gk, cid):
    c = case(cid)
    geo = du.geometry(gk)
    assert gk.dense_gemm_plan(c.m, c.n, c.k, 1) == (2 if c.n <= geo["narrow_n"] else 1)
    got = run(gk, c, 1)
    ref_exec.assert_bits(got, reference()[cid], cid)
    if c.signed_zero:
        assert np.all(np.signbit(got[:, :c.n])) and np.all(got[:, :c.n] == 0.0)


@pytest.mark.parametrize("shape", [(130, 70, 33), (67, 17, 35), (300, 16, 37), (259, 5, 19)], ids=str)
def test_ordered_with_every_row_its_own_equals_the_restatement(gk, shape):
    """the recorded cases repeat their rows with period 5 (dense_gemm_util.operands); here no two rows are alike, and the
    expectation is the restatement that tests/test_dense_gemm_reference.py pins to the reference bit for bit"""
    from gkomi import formats
    from gpu_util import dev, host
    m, n, k = shape
    a, b, c0 = du.operands(m, n, k, [m, n, k, 1], period=None)
    for _, alpha, beta in du.VARIANTS:
        _, av = padded(a, du.A_PAD)
        _, bv = padded(b, du.B_PAD)
        cbuf, cv = padded(c0 if alpha is not None else np.full((m, n), np.nan), du.C_PAD)
        formats.Dense(gk, av).apply(bv, cv, alpha=alpha, beta=beta, mode=1)
        ref_exec.assert_bits(host(cv), du.ordered(a, b, c0, alpha, beta), f"{shape} {alpha} {beta}")
        assert np.all(host(cbuf[:, n:]) == du.FILL)


# ---- automatic: whatever the plan says, that kernel's check -----------------------------------------------------------
@pytest.mark.parametrize("cid", ids(("tile", "narrow", "split")))
def test_automatic_mode_passes_the_check_of_the_kernel_it_plans(gk, cid):
    c = case(cid)
    plan = gk.dense_gemm_plan(c.m, c.n, c.k, 0)
    assert plan in (1, 2, 3) and plan == gk.dense_gemm_plan(c.m, c.n, c.k, 0)
    if c.k <= du.geometry(gk)["L"]:
        assert plan != 3
    got = run(gk, c, 0)
    if plan == 3:
        check_split(gk, c, got)
    else:
        ref_exec.assert_bits(got, reference()[cid], cid)


# ---- split ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ids(("split",)))
def test_split_equals_its_restatement_and_stays_within_the_bound(gk, cid):
    c = case(cid)
    assert gk.dense_gemm_plan(c.m, c.n, c.k, 2) == 3
    got = run(gk, c, 2)
    check_split(gk, c, got)
    ref_exec.assert_bits(run(gk, c, 2), got, cid + ": two runs")


# ---- transpose -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (63, 65), (64, 64), (65, 63), (1, 300), (300, 1), (0, 5)], ids=str)
def test_transpose(gk, shape):
    from gpu_util import host
    rows, cols = shape
    a = np.random.default_rng(rows * 1000 + cols).standard_normal((rows, cols))
    if a.size:
        a.flat[0] = -0.0
    _, av = padded(a, 3)
    out = torch.full((cols, rows + 2), du.FILL, dtype=torch.float64, device="cuda:0")
    gk.dense_transpose_f64(torch.cuda.current_stream().cuda_stream, rows, cols, av, a.shape[1] + 3, out, rows + 2)
    got = host(out)
    ref_exec.assert_bits(got[:, :rows], np.ascontiguousarray(a.T), str(shape))
    ref_exec.assert_bits(got[:, :rows], du.transpose(a), str(shape))
    assert np.all(got[:, rows:] == du.FILL), "padding of out written"
    if rows and cols:
        from gkomi import formats
        t = formats.Dense(gk, av).transpose()
        assert (t.nrows, t.ncols) == (cols, rows)
        ref_exec.assert_bits(host(t.values), np.ascontiguousarray(a.T), str(shape))


def test_golden_cases(gk):
    from gkomi import formats
    from gpu_util import dev, host
    for key in ("applies_to_dense", "applies_linear_combination_to_dense"):
        g = G[key]
        b, c = np.array(g["b"]), np.array(g["c"])
        _, bv = padded(b, g["b_stride"] - b.shape[1])
        cbuf, cv = padded(c, g["c_stride"] - c.shape[1], g["stride_slot"])
        formats.Dense.from_host(gk, np.array(g["a"])).apply(bv, cv, alpha=g.get("alpha"), beta=g.get("beta"))
        ref_exec.assert_bits(host(cv), np.array(g["expect"]), key)
        assert np.all(host(cbuf[:, c.shape[1]:]) == g["stride_slot"])
    for key in ("square_matrix_is_transposable", "non_square_matrix_is_transposable"):
        g = G[key]
        a = np.array(g["in"])
        _, av = padded(a, g.get("in_stride", a.shape[1]) - a.shape[1])
        ref_exec.assert_bits(host(formats.Dense(gk, av).transpose().values), np.array(g["expect"]), key)


# ---- solvers through the callback ------------------------------------------------------------------------------------
def spd_system(n=48):
    rng = np.random.default_rng(48)
    m = rng.standard_normal((n, n))
    a = m.T @ m / n + 2.0 * np.eye(n)
    return a, np.sin(0.1 * np.arange(n))


def as_full_csr(gk, a):
    from gkomi import formats
    n = a.shape[0]
    return formats.Csr.from_host(gk, n, a.shape[1], np.arange(n + 1) * a.shape[1], np.tile(np.arange(a.shape[1]), n),
                                 a.reshape(-1), strategy=1, split=False)    # GKOMI_CSR_STREAM: a row's terms in order


def test_cg_on_dense_equals_cg_on_the_fully_stored_csr(gk):
    """the reference kernel sequence (gkomi_cg_solve_op_f64); the two applies are the same chains"""
    from gkomi import formats, solvers
    from gpu_util import dev, host
    a, b = spd_system()
    d = solvers.solve_op(gk, "cg", formats.Dense.from_host(gk, a), dev(b), max_iters=200, reduction=1e-12)
    s = solvers.solve_op(gk, "cg", as_full_csr(gk, a), dev(b), max_iters=200, reduction=1e-12)
    assert d["converged"] and s["converged"] and 0 < d["iterations"] == s["iterations"] < 200
    ref_exec.assert_bits(host(d["x"]), host(s["x"]), "x")
    assert np.linalg.norm(a @ host(d["x"]).reshape(-1) - b) <= 1e-10 * np.linalg.norm(b)


def test_bicg_on_dense_through_transpose_equals_bicg_on_csr(gk):
    from gkomi import formats, solvers
    from gpu_util import dev, host
    a, b = spd_system()
    a = a + np.triu(np.random.default_rng(3).standard_normal(a.shape), 1) * 0.05      # not symmetric: A^T matters
    dense = formats.Dense.from_host(gk, a)
    d = solvers.bicg_solve_op(gk, dense, dense.transpose(), dev(b), max_iters=200, reduction=1e-12)
    s = solvers.bicg_solve_op(gk, as_full_csr(gk, a), as_full_csr(gk, np.ascontiguousarray(a.T)), dev(b), max_iters=200,
                              reduction=1e-12)
    assert d["converged"] and s["converged"] and 0 < d["iterations"] == s["iterations"] < 200
    ref_exec.assert_bits(host(d["x"]), host(s["x"]), "x")
    assert np.linalg.norm(a @ host(d["x"]).reshape(-1) - b) <= 1e-10 * np.linalg.norm(b)


# ---- mirror and shims ------------------------------------------------------------------------------------------------
def test_mirror_example_prints_its_ok_lines():
    ex = os.path.join(PKG, "examples")
    r = subprocess.run(["make", "-C", ex, "bin/dense_operator_mirror"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(ex, "bin", "dense_operator_mirror")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split(":", 1)[1].strip() for ln in r.stdout.splitlines() if ln.startswith("dense_operator_mirror:")]
    assert lines == ["apply ok", "advanced_apply ok", "transpose ok", "cg ok", "bicg ok"], r.stdout


def test_dense_gemm_shims_run_on_the_device(tmp_path):
    from test_dense_gemm_reference import build_dense_shim_smoke
    run_ = subprocess.run([build_dense_shim_smoke(tmp_path)], capture_output=True, text=True)
    ran = {t[1]: t[2] for t in (ln.split() for ln in run_.stdout.splitlines()) if len(t) == 3 and t[0] == "ran"}
    assert run_.returncode == 0, run_.stdout + run_.stderr
    assert ran == {k: "ok" for k in ("dense::simple_apply", "dense::apply", "dense::transpose", "dense::conj_transpose")}, ran


if __name__ == "__main__" and sys.argv[1:] == ["record"]:
    du.batch_of(case_list())[0].record(RECORDING)
    print(f"{RECORDING}: {os.path.getsize(RECORDING)} bytes")
