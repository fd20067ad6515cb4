"""GPU tests of the mixed-precision path (csrc/mixed.hip): convert_precision<double <-> float> bit-exact against
numpy's static_cast (round to nearest even, overflow to inf, subnormals kept), the fused Cg<float> against the oracle's
Cg<float> (oracle/f32.c), and Ir<double> over that Cg<float> against the reference Ir loop composed here from the
oracle's double SpMV and its Cg<float>."""
import json
import os

import numpy as np
import pytest
import torch

import matgen
from gpu_util import dev, host, stream_ptr

pytestmark = pytest.mark.gpu
F = np.float32
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _same_bits(got, expect):
    """bit-identical, NaN matching any NaN"""
    got, expect = np.asarray(got), np.asarray(expect)
    nan = np.isnan(expect)
    assert np.array_equal(np.isnan(got), nan)
    ui = np.uint32 if got.dtype == np.float32 else np.uint64
    assert np.array_equal(got[~nan].view(ui), expect[~nan].view(ui))


def _special_doubles(rng):
    f = rng.standard_normal(2000).astype(F)
    up = np.nextafter(f, np.float32(np.inf))
    ties = (f.astype(np.float64) + up.astype(np.float64)) / 2  # exactly halfway between two floats
    fmax = float(np.finfo(F).max)
    tiny = float(np.finfo(F).tiny)
    specials = [0.0, -0.0, np.inf, -np.inf, np.nan, fmax, -fmax, fmax * 1.0000001, -fmax * 1.0000001, 1e300, -1e300,
                fmax + 2.0 ** 103, np.nextafter(fmax + 2.0 ** 103, 0.0), tiny, tiny / 2, tiny / 3, -tiny / 7, 1e-40, -3e-42,
                1.4e-45, 7e-46, 6e-46, 1e-300, -1e-320]
    sub = rng.uniform(-tiny, tiny, 500)
    return np.concatenate([rng.standard_normal(3000) * 10.0 ** rng.integers(-30, 30, 3000), ties, np.array(specials), sub])


@pytest.mark.parametrize("shape", ["flat", "cols1_stride4", "cols3", "cols3_stride7", "empty"])
def test_convert_bit_exact_both_directions(gk, shape):
    rng = np.random.default_rng(7)
    vals = _special_doubles(rng)
    ncols, in_stride, out_stride = {"flat": (1, 1, 1), "cols1_stride4": (1, 4, 3), "cols3": (3, 3, 3),
                                    "cols3_stride7": (3, 7, 5), "empty": (3, 5, 4)}[shape]
    nrows = 0 if shape == "empty" else len(vals) // ncols
    vals = vals[:nrows * ncols].reshape(nrows, ncols)
    src = np.full((nrows, in_stride), 12345.0)
    src[:, :ncols] = vals
    # f64 -> f32
    sentinel = F(-777.25)
    out = torch.full((max(nrows, 1), out_stride), float(sentinel), dtype=torch.float32, device="cuda:0")
    gk.dense_convert_f64_to_f32(stream_ptr(), nrows, ncols, dev(src), in_stride, out, out_stride)
    got = host(out)
    with np.errstate(over="ignore"):
        expect = vals.astype(F)
    _same_bits(got[:nrows, :ncols], expect)
    assert np.all(got[:, ncols:] == sentinel), "padding between rows written"
    if nrows == 0:
        assert np.all(got == sentinel)
    # f32 -> f64: exact
    srcf = np.full((nrows, in_stride), F(3.5), F)
    srcf[:, :ncols] = expect
    out64 = torch.full((max(nrows, 1), out_stride), -777.25, dtype=torch.float64, device="cuda:0")
    gk.dense_convert_f32_to_f64(stream_ptr(), nrows, ncols, dev(srcf), in_stride, out64, out_stride)
    got64 = host(out64)
    _same_bits(got64[:nrows, :ncols], expect.astype(np.float64))
    assert np.all(got64[:, ncols:] == -777.25)


@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 7, 8, 1023, 4097, 1 << 20])
@pytest.mark.parametrize("offset", [0, 1])
def test_convert_vector_lengths_and_alignment(gk, count, offset):
    """the 16-B path (contiguous, aligned) and its tail, and an unaligned view that takes the strided path"""
    rng = np.random.default_rng(count)
    v = rng.standard_normal(count + offset) * 1e3
    src = dev(v)[offset:]
    out = torch.full((count + 4,), -1.0, dtype=torch.float32, device="cuda:0")
    gk.dense_convert_f64_to_f32(stream_ptr(), count, 1, src, 1, out[offset:], 1)
    got = host(out)
    _same_bits(got[offset:offset + count], v[offset:].astype(F))
    assert np.all(got[offset + count:] == -1.0) and np.all(got[:offset] == -1.0)
    back = torch.full((count + 4,), -1.0, dtype=torch.float64, device="cuda:0")
    gk.dense_convert_f32_to_f64(stream_ptr(), count, 1, out[offset:], 1, back[offset:], 1)
    gb = host(back)
    _same_bits(gb[offset:offset + count], v[offset:].astype(F).astype(np.float64))
    assert np.all(gb[offset + count:] == -1.0)


def test_convert_rejects_bad_arguments(gk):
    from gkomi._lib import GkomiError
    x = torch.zeros(8, dtype=torch.float64, device="cuda:0")
    y = torch.zeros(8, dtype=torch.float32, device="cuda:0")
    for args in [(-1, 1, x, 1, y, 1), (2, 3, x, 2, y, 3), (2, 3, x, 3, y, 2), (2, -1, x, 1, y, 1)]:
        with pytest.raises(GkomiError) as e:
            gk.dense_convert_f64_to_f32(stream_ptr(), *args)
        assert e.value.code == -1


# ---- fused Cg<float> -------------------------------------------------------------------------------------------------

def fused_cg(gk, n, rp, ci, v, b, x0, max_iters, reduction, baseline):
    x = dev(np.asarray(x0, F))
    nb = gk.cg_fused_workspace_bytes_f32(n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda:0")
    info = np.zeros(4)
    gk.cg_solve_fused_f32_i32(stream_ptr(), n, len(v), dev(rp.astype(np.int32)), dev(ci.astype(np.int32)), dev(v.astype(F)),
                              dev(np.asarray(b, F)), x, max_iters, reduction, baseline, ws, nb, info)
    return host(x), int(info[0]), bool(info[1]), info[2], info[3]


def _systems():
    g = json.load(open(os.path.join(G, "cg.json")))["solve_cases"]
    out = []
    for c in g:
        rp, ci, v = matgen.dense_to_csr(c["A"])
        out.append((c["name"], len(c["b"]), rp, ci, v, np.array(c["b"], np.float64), np.array(c["x0"], np.float64)))
    rng = np.random.default_rng(3)
    n, rp, ci, v = matgen.poisson_2d_5pt(71, 53)
    out.append(("poisson2d", n, rp, ci, v, rng.standard_normal(n), 0.1 * rng.standard_normal(n)))
    n, rp, ci, v = matgen.poisson_3d_7pt(17, 19, 21)
    out.append(("poisson3d", n, rp, ci, v, rng.standard_normal(n), 0.1 * rng.standard_normal(n)))
    return out


SYSTEMS = _systems()


@pytest.mark.parametrize("system", SYSTEMS, ids=lambda s: s[0])
@pytest.mark.parametrize("guess", ["zero", "x0"])
@pytest.mark.parametrize("baseline", [0, 1, 2], ids=["rhs_norm", "initial_resnorm", "absolute"])
def test_fused_f32_cg_against_oracle(gk, oracle, system, guess, baseline):
    name, n, rp, ci, v, b, x0 = system
    if guess == "zero":
        x0 = np.zeros(n)
    reduction = 1e-5
    if baseline == 2:  # the same goal as an absolute norm
        reduction = 1e-5 * float(np.linalg.norm(b))
    x, iters, conv, res, base = fused_cg(gk, n, rp, ci, v, b, x0, 1000, reduction, baseline)
    xe = np.asarray(x0, F).copy()
    ite = oracle.ref_cg_solve_f32(n, rp.astype(np.int32), ci.astype(np.int32), v.astype(F), b.astype(F), xe, 1000,
                                  F(reduction), baseline)
    assert ite < 1000, "oracle did not converge"
    assert conv and abs(iters - ite) <= max(2, int(0.05 * ite)), (iters, ite)
    assert res < reduction * base
    assert matgen.rel_err(x.astype(np.float64), xe.astype(np.float64)) <= 1e-3


def test_fused_f32_cg_iteration_cap(gk, oracle):
    n, rp, ci, v = matgen.poisson_2d_5pt(40)
    b = np.random.default_rng(1).standard_normal(n)
    x, iters, conv, _, _ = fused_cg(gk, n, rp, ci, v, b, np.zeros(n), 5, 1e-7, 0)
    xe = np.zeros(n, F)
    oracle.ref_cg_solve_f32(n, rp.astype(np.int32), ci.astype(np.int32), v.astype(F), b.astype(F), xe, 5, F(1e-7), 0)
    assert iters == 5 and not conv
    assert matgen.rel_err(x.astype(np.float64), xe.astype(np.float64)) <= 1e-4
    x, iters, conv, _, _ = fused_cg(gk, n, rp, ci, v, b, np.zeros(n), 0, 1e-7, 0)
    assert iters == 0 and not conv and np.all(x == 0)


# ---- Ir<double> over Cg<float> ---------------------------------------------------------------------------------------

def ref_ir_mixed(oracle, n, rp, ci, v, b, x, max_iters, reduction, inner_max_iters, inner_reduction, relaxation):
    """core/solver/ir.cpp:188-277 with Cg<float> inner solver behind precision_dispatch, baselines rhs_norm"""
    rp32, ci32, vf = rp.astype(np.int32), ci.astype(np.int32), v.astype(F)

    def residual(x):
        ax = np.zeros((n, 1))
        oracle.ref_csr_spmv(n, 1, rp32, ci32, v, x.reshape(n, 1), 1, ax, 1)
        return b - ax[:, 0]

    x = x.copy()
    r = residual(x)
    goal = reduction * np.linalg.norm(b)
    it = -1
    inner_total = 0
    while True:
        it += 1
        if it >= max_iters:
            return x, it, False, inner_total
        if np.linalg.norm(r) < goal:
            return x, it, True, inner_total
        rf = r.astype(F)
        d = rf.copy()
        inner_total += oracle.ref_cg_solve_f32(n, rp32, ci32, vf, rf, d, inner_max_iters, F(inner_reduction), 0)
        x = x + relaxation * d.astype(np.float64)
        r = residual(x)


def _mtx(name):
    kind, n, m, rows, cols, vals = matgen.read_mtx(os.path.join(G, name))
    rp, ci, v = matgen.coo_to_csr(n, rows, cols, vals)
    return n, rp, ci, v


def _ir_matrix(name):
    if name == "poisson2d_100":
        return matgen.poisson_2d_5pt(100)
    if name == "poisson3d_30":
        return matgen.poisson_3d_7pt(30)
    return _mtx(name)


def ir_raw(gk, n, rp, ci, v, b, x0, max_iters, reduction, inner_max_iters, inner_reduction, relaxation):
    vd = dev(v)
    vf = torch.empty(len(v), dtype=torch.float32, device="cuda:0")
    gk.dense_convert_f64_to_f32(stream_ptr(), len(v), 1, vd, 1, vf, 1)
    x = dev(np.asarray(x0, np.float64))
    nb = gk.ir_mixed_workspace_bytes(n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda:0")
    info = np.zeros(6)
    gk.ir_mixed_solve_f64_i32(stream_ptr(), n, 1, len(v), dev(rp.astype(np.int32)), dev(ci.astype(np.int32)), vd, vf, 0, -1,
                              dev(b), x, max_iters, reduction, 0, inner_max_iters, inner_reduction, 0, relaxation, ws, nb,
                              info)
    return host(x), info


@pytest.mark.parametrize("name", ["poisson2d_100", "poisson3d_30", "ani4.mtx"])
@pytest.mark.parametrize("relaxation", [1.0, 0.8])
def test_ir_mixed_against_reference_loop(gk, oracle, name, relaxation):
    n, rp, ci, v = _ir_matrix(name)
    rng = np.random.default_rng(11)
    b = rng.standard_normal(n)
    x0 = np.zeros(n)
    x, info = ir_raw(gk, n, rp, ci, v, b, x0, 100, 1e-12, 200, 1e-2, relaxation)
    xe, ite, conv_e, inner_e = ref_ir_mixed(oracle, n, rp, ci, v, b, x0, 100, 1e-12, 200, 1e-2, relaxation)
    assert conv_e
    assert bool(info[1]) and abs(int(info[0]) - ite) <= 1, (info, ite)
    ax = np.zeros((n, 1))
    oracle.ref_csr_spmv(n, 1, rp.astype(np.int32), ci.astype(np.int32), v, x.reshape(n, 1), 1, ax, 1)
    true_res = np.linalg.norm(b - ax[:, 0])
    assert true_res <= 1e-12 * np.linalg.norm(b)
    assert abs(info[2] - true_res) <= 1e-3 * true_res
    assert info[3] == pytest.approx(np.linalg.norm(b), rel=1e-12)
    assert info[4] >= int(info[0]) and info[5] == 0
    assert abs(info[4] - inner_e) <= max(2 * int(info[0]), int(0.1 * inner_e))


def test_ir_mixed_ill_conditioned_report_is_consistent(gk, oracle):
    """1138_bus (kappa ~ 1e7): near the limit of float CG; whatever happens, the report says what happened"""
    n, rp, ci, v = _mtx("1138_bus.mtx")
    b = np.random.default_rng(2).standard_normal(n)
    x, info = ir_raw(gk, n, rp, ci, v, b, np.zeros(n), 30, 1e-12, 500, 1e-2, 1.0)
    ax = np.zeros((n, 1))
    oracle.ref_csr_spmv(n, 1, rp.astype(np.int32), ci.astype(np.int32), v, x.reshape(n, 1), 1, ax, 1)
    true_res = np.linalg.norm(b - ax[:, 0])
    if info[1]:
        assert true_res <= 1e-12 * np.linalg.norm(b) and info[0] < 30
    else:
        assert int(info[0]) == 30
    assert 0 <= info[5] <= info[0]


def test_ir_mixed_outer_cap_and_unsupported(gk):
    from gkomi._lib import GkomiError
    n, rp, ci, v = matgen.poisson_2d_5pt(50)
    b = np.random.default_rng(4).standard_normal(n)
    x, info = ir_raw(gk, n, rp, ci, v, b, np.zeros(n), 2, 1e-12, 100, 1e-2, 1.0)
    assert int(info[0]) == 2 and not info[1] and info[2] > 1e-12 * info[3]
    # inner cap: 3 iterations per inner solve, each of them stopped by the cap
    x, info = ir_raw(gk, n, rp, ci, v, b, np.zeros(n), 4, 1e-12, 3, 1e-6, 1.0)
    assert int(info[0]) == 4 and info[4] == 12 and info[5] == 4
    with pytest.raises(GkomiError) as e:
        gk.ir_mixed_solve_f64_i32(stream_ptr(), n, 2, len(v), None, None, None, None, 0, -1, None, None, 10, 1e-12, 0, 10,
                                  1e-2, 0, 1.0, None, 0, None)
    assert e.value.code == -2


def test_python_ir_mixed_matches_raw_entry(gk):
    import gkomi.solvers as solvers
    n, rp, ci, v = matgen.poisson_2d_5pt(60)
    rng = np.random.default_rng(9)
    b = rng.standard_normal(n)
    x0 = 0.01 * rng.standard_normal(n)
    x_raw, info = ir_raw(gk, n, rp, ci, v, b, x0, 50, 1e-12, 100, 1e-2, 0.9)
    got = solvers.ir_mixed(gk, n, dev(rp.astype(np.int32)), dev(ci.astype(np.int32)), dev(v), dev(b), x=dev(x0), max_iters=50,
                           reduction=1e-12, inner_max_iters=100, inner_reduction=1e-2, relaxation_factor=0.9)
    assert np.array_equal(host(got["x"]), x_raw)
    assert got["iterations"] == int(info[0]) and got["converged"] == bool(info[1]) and got["converged"]
    assert got["residual_norm"] == info[2] and got["baseline_norm"] == info[3]
    assert got["inner_iterations"] == int(info[4]) and got["inner_capped"] == int(info[5])
