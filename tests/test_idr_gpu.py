"""GPU parity of IDR(s) through the C ABI: the step kernels against the numpy restatement of the reference's loops
(idr_util.py; bit for bit where the kernel is elementwise, within the error budget of a re-ordered sum elsewhere), the
two drivers against the reference's known answers and the restatement's iteration counts."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import gkomi
import idr_util
import matgen
import oracle_lib
from gkomi import solvers
from gpu_util import dev, host, stream_ptr
from krylov_util import dense_to_csr

pytestmark = pytest.mark.gpu
G = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "idr.json")))
EPS = np.finfo(np.float64).eps
LD = np.longdouble


def budget(n, err64):
    """what a device sum in another order may be off by: 4 eps sqrt(n), or 4 x what the float64 restatement itself is
    off by against extended precision"""
    return max(4 * EPS * np.sqrt(n), 4 * err64)


def ld_err(a, exact):
    return matgen.rel_err(np.asarray(a, np.float64), np.asarray(exact.astype(np.float64)))


def orthonormal_rows(rng, s, n):
    p = rng.standard_normal((s, n))
    if n >= s:
        p = np.linalg.qr(p.T)[0].T.copy()
    else:
        p /= np.linalg.norm(p, axis=1, keepdims=True)
    return np.ascontiguousarray(p)


def step_data(n, nrhs, pad, s, seed):
    rng = np.random.default_rng(seed)
    wide = s * nrhs
    d = {"p": orthonormal_rows(rng, s, n), "m": rng.standard_normal((s, wide)), "f": rng.standard_normal((s, nrhs)),
         "c": rng.standard_normal((s, nrhs)), "g": rng.standard_normal((n, wide + pad)),
         "u": rng.standard_normal((n, wide + pad))}
    for k in ("residual", "v", "x", "g_k", "pv"):
        d[k] = rng.standard_normal((n, nrhs + pad))
    for j in range(s):                                        # |m_jj| >= 1
        for i in range(nrhs):
            d["m"][j, j * nrhs + i] = np.copysign(1.0 + abs(d["m"][j, j * nrhs + i]), d["m"][j, j * nrhs + i])
    for k in ("omega", "tht", "residual_norm"):
        d[k] = rng.standard_normal(nrhs)
    d["tht"], d["residual_norm"] = np.abs(d["tht"]) + 0.1, np.abs(d["residual_norm"]) + 0.1
    stop = np.zeros(nrhs, np.uint8)
    if nrhs > 2:
        stop[1] = 1                                           # a stopped column
    return d, stop


SHAPES = [(1, 1, 0), (777, 3, 2), (100003, 2, 0)]


@pytest.mark.parametrize("s", [1, 4])
@pytest.mark.parametrize("n,nrhs,pad", SHAPES)
def test_elementwise_kernels_bitexact(gk, n, nrhs, pad, s):
    wide = s * nrhs
    for k in sorted({0, s - 1}):
        data, stop = step_data(n, nrhs, pad, s, 100 * s + n % 97 + k)
        e = {key: val.copy() for key, val in data.items()}
        idr_util.step_1(nrhs, k, e["m"], e["f"], e["residual"][:, :nrhs], e["g"][:, :wide], e["c"], e["v"][:, :nrhs], stop)
        idr_util.step_2(nrhs, k, e["omega"], e["pv"][:, :nrhs], e["c"], e["u"][:, :wide], stop)
        idr_util.compute_omega(nrhs, 0.7, e["tht"], e["residual_norm"], e["omega"], stop)
        d = {key: dev(val) for key, val in data.items()}
        ds = dev(stop)
        gk.idr_step_1_f64(stream_ptr(), n, nrhs, s, k, d["m"], wide, d["f"], nrhs, d["residual"], nrhs + pad, d["g"],
                          wide + pad, d["c"], nrhs, d["v"], nrhs + pad, ds)
        gk.idr_step_2_f64(stream_ptr(), n, nrhs, s, k, d["omega"], d["pv"], nrhs + pad, d["c"], nrhs, d["u"], wide + pad, ds)
        gk.idr_compute_omega_f64(stream_ptr(), nrhs, 0.7, d["tht"], d["residual_norm"], d["omega"], ds)
        for key in ("c", "v", "u", "omega"):
            assert host(d[key]).tobytes() == e[key].tobytes(), (key, k)
        assert host(ds).tobytes() == stop.tobytes()


@pytest.mark.parametrize("s", [1, 4])
@pytest.mark.parametrize("n,nrhs,pad", SHAPES)
def test_initialize(gk, n, nrhs, pad, s):
    rng = np.random.default_rng(n + s)
    p = rng.standard_normal((s, n))
    m = dev(np.full((s, s * nrhs + pad), 7.0))
    st = dev(np.ones(nrhs, np.uint8))
    dp = dev(p)
    if s > n:
        with pytest.raises(gkomi.GkomiError) as err:
            gk.idr_initialize_f64(stream_ptr(), n, nrhs, s, m, s * nrhs + pad, dp, n, st)
        assert err.value.code == -1
        return
    gk.idr_initialize_f64(stream_ptr(), n, nrhs, s, m, s * nrhs + pad, dp, n, st)
    em = np.full((s, s * nrhs + pad), 7.0)
    p64, pld, est = p.copy(), p.astype(LD), np.ones(nrhs, np.uint8)
    idr_util.initialize(nrhs, em[:, :s * nrhs], p64, est)
    idr_util.initialize(nrhs, np.zeros((s, s * nrhs), LD), pld, est.copy())
    assert host(m).tobytes() == em.tobytes() and not host(st).any()
    err64, errdev = ld_err(p64, pld), ld_err(host(dp), pld)
    print(f"initialize n={n} s={s}: P error device {errdev:.3e}, float64 restatement {err64:.3e}")
    assert errdev <= budget(n, err64)


STEP_3_OUT = ("g", "u", "m", "f", "residual", "x")


@pytest.mark.parametrize("s", [1, 4])
@pytest.mark.parametrize("n,nrhs,pad", SHAPES)
def test_step_3_within_the_error_of_a_reordered_sum(gk, n, nrhs, pad, s):
    wide = s * nrhs
    for k in sorted({0, s - 1}):
        data, stop = step_data(n, nrhs, pad, s, 7 * s + n % 89 + k)

        def restate(dt):
            e = {key: val.astype(dt) for key, val in data.items()}
            idr_util.step_3(nrhs, k, e["p"], e["g"][:, :wide], e["g_k"][:, :nrhs], e["u"][:, :wide], e["m"], e["f"],
                            e["residual"][:, :nrhs], e["x"][:, :nrhs], stop)
            return e
        e64, eld = restate(np.float64), restate(LD)
        d = {key: dev(val) for key, val in data.items()}
        alpha = dev(np.zeros(nrhs))
        nbytes = gk.idr_step_3_workspace_bytes(nrhs, s)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
        gk.idr_step_3_f64(stream_ptr(), n, nrhs, s, k, d["p"], n, d["g"], wide + pad, d["g_k"], nrhs + pad, d["u"],
                          wide + pad, d["m"], wide, d["f"], nrhs, alpha, d["residual"], nrhs + pad, d["x"], nrhs + pad,
                          dev(stop), ws, nbytes)
        for key in STEP_3_OUT:
            got = host(d[key])
            err64, errdev = ld_err(e64[key], eld[key]), ld_err(got, eld[key])
            print(f"step_3 n={n} nrhs={nrhs} s={s} k={k} {key}: device {errdev:.3e}, float64 restatement {err64:.3e}")
            assert errdev <= budget(n, err64), (key, k)
            if nrhs > 2:                                      # the stopped column and the padding are untouched
                width = wide if key in ("g", "u", "m") else nrhs
                cols = [j * nrhs + 1 for j in range(s)] if key in ("g", "u", "m") else [1]
                assert np.array_equal(got[:, cols], data[key][:, cols]), key
                assert np.array_equal(got[:, width:], data[key][:, width:]), key


@pytest.mark.parametrize("s", [1, 4])
@pytest.mark.parametrize("n", [777, 100003])
def test_fused_projection_within_the_error_of_a_reordered_sum(gk, n, s):
    """Step 3 of the fused driver on its own: one multi-dot sweep, the triangular solve with the stored m, one update
    sweep -- against the reference order in extended precision, on data where m_ji = p_j . g_i holds as in a solve."""
    ld = n + (n & 1)
    for k in sorted({0, s - 1}):
        rng = np.random.default_rng(31 * s + k + n % 83)
        p = orthonormal_rows(rng, s, n)
        g, u = rng.standard_normal((n, s)), rng.standard_normal((n, s))
        for j in range(s):                                    # p_j . g_j = m_jj with |m_jj| >= 1
            pl = p[j].astype(LD)
            want = np.copysign(1.0 + abs(rng.standard_normal()), rng.standard_normal())
            g[:, j] = (g[:, j].astype(LD) + (want - pl @ g[:, j].astype(LD)) * pl).astype(np.float64)
        m = (p.astype(LD) @ g.astype(LD)).astype(np.float64)
        m[:, k:] = rng.standard_normal((s, s - k))             # column k onwards is what the step defines
        f, r, x = rng.standard_normal((s, 1)), rng.standard_normal((n, 1)), rng.standard_normal((n, 1))
        stop = np.zeros(1, np.uint8)

        def restate(dt):
            e = {"g": g.astype(dt), "u": u.astype(dt), "m": m.astype(dt), "f": f.astype(dt), "residual": r.astype(dt),
                 "x": x.astype(dt)}
            g_k = e["g"][:, k:k + 1].copy()
            idr_util.step_3(1, k, p.astype(dt), e["g"], g_k, e["u"], e["m"], e["f"], e["residual"], e["x"], stop)
            return e
        e64, eld = restate(np.float64), restate(LD)

        def colmajor(a):                                      # n x s -> s columns of ld
            out = np.zeros((a.shape[1], ld))
            out[:, :n] = a.T
            return dev(out)
        dp, dg, du, dm = colmajor(p.T), colmajor(g), colmajor(u), dev(m)
        df, dfo, dr, dx = dev(f[:, 0].copy()), dev(np.zeros(s)), dev(r[:, 0].copy()), dev(x[:, 0].copy())
        nbytes = gk.idr_fused_step_3_workspace_bytes(s)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
        gk.idr_fused_step_3_f64(stream_ptr(), n, s, k, dp, dg, du, ld, dm, df, dfo, dr, dx, ws, nbytes)
        got = {"g": host(dg)[:, :n].T, "u": host(du)[:, :n].T, "m": host(dm), "f": host(dfo).reshape(s, 1),
               "residual": host(dr).reshape(n, 1), "x": host(dx).reshape(n, 1)}
        for key in STEP_3_OUT:
            err64, errdev = ld_err(e64[key], eld[key]), ld_err(got[key], eld[key])
            print(f"fused step 3 n={n} s={s} k={k} {key}: device {errdev:.3e}, float64 restatement {err64:.3e}")
            assert errdev <= budget(n, err64), (key, k)


@pytest.mark.parametrize("fused", [False, True], ids=["sequence", "fused"])
@pytest.mark.parametrize("case", G["solves"], ids=lambda c: c["name"])
def test_known_answers(gk, case, fused):
    n, rp, ci, v = dense_to_csr(case["A"])
    b = np.array(case["b"])
    args = (gk, n, dev(rp), dev(ci), dev(v), dev(b))
    kw = dict(subspace_dim=G["subspace_dim"], kappa=G["kappa"], max_iters=case["max_iters"], reduction=case["reduction"])
    if fused and b.shape[1] != 1:
        with pytest.raises(gkomi.GkomiError) as err:           # one right-hand side only
            solvers.idr_solve(*args, fused=True, **kw)
        assert err.value.code == solvers.GKOMI_ENOTSUPPORTED
        return
    res = solvers.idr_solve(*args, fused=fused, **kw)
    err = matgen.rel_err(host(res["x"]), np.array(case["expect_x"]))
    print(case["name"], "fused" if fused else "sequence", "iterations", res["iterations"], "rel err", err)
    # the reference's tolerance holds for its sequential dots; the device sums in another order: allow 4x
    assert err <= 4 * case["tol"], res


def convection(n3=12):
    n, rp, ci, v = matgen.poisson_3d_7pt(n3)
    v = v.copy()
    rows = np.repeat(np.arange(n), np.diff(rp))
    v[ci == rows - 1] -= 0.5
    v[ci == rows] += 0.5
    return n, rp, ci, v


@functools.lru_cache(maxsize=None)
def problem(name):
    n, rp, ci, v = {"poisson": lambda: matgen.poisson_2d_5pt(40), "convection": convection,
                    "poisson317": lambda: matgen.poisson_2d_5pt(317)}[name]()
    xs = np.sin(0.3 * np.arange(n))
    b = np.zeros((n, 1))
    oracle_lib.load().ref_csr_spmv(n, 1, rp, ci, v, xs.reshape(n, 1), 1, b, 1)
    return n, rp, ci, v, xs, b


@functools.lru_cache(maxsize=None)
def restated(name, s):
    """outer iterations of the restatement on `name` with the P the device gets too (computed once, shared)"""
    n, rp, ci, v, xs, b = problem(name)
    res = idr_util.solve(idr_util.csr_apply(oracle_lib.load(), n, rp, ci, v), b.copy(), idr_util.subspace(s, n, 15),
                         subspace_dim=s, max_iters=4000, reduction=1e-10)
    assert res["converged"]
    return res["iterations"]


def check_solve(gk, name, s, fused):
    n, rp, ci, v, xs, b = problem(name)
    rpd, cid, vd = dev(rp), dev(ci), dev(v)
    run = lambda **kw: solvers.idr_solve(gk, n, rpd, cid, vd, dev(b[:, 0].copy()), subspace_dim=s,
                                         subspace=dev(idr_util.subspace(s, n, 15)), max_iters=4000, reduction=1e-10,
                                         fused=fused, **kw)
    res = run()
    x = host(res["x"])
    r = b[:, 0] - np.add.reduceat(v * x[ci], rp[:-1])
    true_rel = np.linalg.norm(r) / np.linalg.norm(b)
    ite = restated(name, s)
    print(f"{name} s={s} {'fused' if fused else 'sequence'}: {res['iterations']} outer iterations (restatement {ite}), "
          f"true relative residual {true_rel:.3e}, reported {res['rel_residual']:.3e}")
    assert res["converged"]
    assert true_rel <= 1e-10
    assert abs(res["iterations"] - ite) <= max(2, ite // 10), (res["iterations"], ite)
    return run, res


@pytest.mark.parametrize("fused", [False, True], ids=["sequence", "fused"])
@pytest.mark.parametrize("s", [1, 2, 4, 8])
@pytest.mark.parametrize("name", ["poisson", "convection"])
def test_solves_like_the_restatement(gk, name, s, fused):
    run, res = check_solve(gk, name, s, fused)
    if fused:  # the criterion lives on the device: how often the host looks changes nothing
        for every in (1, 3, 50):
            again = run(check_every=every)
            assert again["iterations"] == res["iterations"] and again["converged"]
            assert host(again["x"]).tobytes() == host(res["x"]).tobytes()
            assert again["residual_norm"][0] == res["residual_norm"][0]


def test_fused_odd_tail_and_many_partials(gk):
    """n = 100 489: an odd tail element, and more workgroups in a sweep than one block of partials holds lanes"""
    check_solve(gk, "poisson317", 4, True)


def test_limits(gk):
    n, rp, ci, v, xs, b = problem("poisson")
    rpd, cid, vd = dev(rp), dev(ci), dev(v)
    for fused in (False, True):
        capped = solvers.idr_solve(gk, n, rpd, cid, vd, dev(b[:, 0].copy()), subspace_dim=4, max_iters=3, fused=fused)
        assert capped["iterations"] == 3 and not capped["converged"]
        r = b[:, 0] - np.add.reduceat(v * host(capped["x"])[ci], rp[:-1])
        # recurrence and true residual differ by the rounding of 3 x 5 updates, ~1e-14 |b|; a norm taken before the
        # last omega step would be off by a tenth of |r| or more
        assert abs(np.linalg.norm(r) - capped["residual_norm"][0]) <= 1e-12 * np.linalg.norm(b)
    # s = 9 on the fused entry, s > 32, s = 0; and s > n on the reference's 3 x 3 system
    n3, rp3, ci3, v3 = dense_to_csr(G["solves"][0]["A"])
    small = (n3, dev(rp3), dev(ci3), dev(v3), np.array(G["solves"][0]["b"]))
    big = (n, rpd, cid, vd, b)
    for system, fused, s, code in ((big, True, 9, solvers.GKOMI_ENOTSUPPORTED), (big, False, 33, -1), (big, True, 0, -1),
                                   (small, False, 4, -1), (small, True, 4, -1)):
        nn, rps, cis, vs, bs = system
        ws = torch.empty(gk.idr_workspace_bytes(nn, 1, 8) + (1 << 20), dtype=torch.uint8, device="cuda:0")
        p = torch.zeros((max(s, 1), nn), dtype=torch.float64, device="cuda:0")
        entry = gk.idr_solve_fused_f64_i32 if fused else gk.idr_solve_f64_i32
        with pytest.raises(gkomi.GkomiError) as err:
            entry(stream_ptr(), nn, 1, int(vs.numel()), rps, cis, vs, 0, -1, None, None, s, 0.7, p, dev(bs), dev(bs * 0), 10,
                  1e-10, 0, 8, ws, ws.numel(), np.zeros(4))
        assert err.value.code == code, (fused, s)


def test_jacobi_three_right_hand_sides_one_converging_early(gk):
    n, rp, ci, v = matgen.poisson_2d_5pt(32)
    rpd, cid, vd = dev(rp), dev(ci), dev(v)
    rng = np.random.default_rng(4)
    xs = rng.standard_normal((n, 3))
    b = np.zeros((n, 3))
    oracle_lib.load().ref_csr_spmv(n, 3, rp, ci, v, xs, 3, b, 3)
    x0 = np.zeros((n, 3))
    x0[:, 1] = xs[:, 1] * (1 + 1e-8)                           # this column needs a few iterations only
    pc = solvers.jacobi_generate(gk, n, rpd, cid, vd, max_block_size=4, nrhs=3)
    alone = solvers.idr_solve(gk, n, rpd, cid, vd, dev(b[:, 1].copy()), x=dev(x0[:, 1].copy()), subspace_dim=4,
                              max_iters=2000, reduction=1e-11,
                              precond=solvers.jacobi_generate(gk, n, rpd, cid, vd, max_block_size=4))
    res = solvers.idr_solve(gk, n, rpd, cid, vd, dev(b), x=dev(x0), subspace_dim=4, max_iters=2000, reduction=1e-11,
                            precond=pc)
    assert res["converged"] and alone["converged"] and alone["iterations"] < res["iterations"]
    assert matgen.rel_err(host(res["x"]), xs) < 1e-8
    r = b - np.stack([np.add.reduceat(v * host(res["x"])[ci, j], rp[:-1]) for j in range(3)], axis=1)
    # a stopped column is left alone: what is reported for it is the norm of its residual
    assert np.all(np.abs(np.linalg.norm(r, axis=0) - res["residual_norm"]) <= 1e-6 * np.linalg.norm(b, axis=0))
    # the criterion bounds the recurrence residual by 1e-11 |b|; the true one may differ from it by the rounding of
    # ~100 updates, ~1e-13 |b|: 10 % on top
    assert np.all(np.linalg.norm(r, axis=0) <= 1.1e-11 * np.linalg.norm(b, axis=0))


def test_fused_with_jacobi_and_on_every_format(gk):
    """the fused driver with a preconditioner (step 1 - apply - step 2) and behind solve_op: ELL carries the dot
    epilogue, COO takes apply + a partials kernel"""
    from gkomi import formats
    n, rp, ci, v, xs, b = problem("convection")
    A = formats.Csr.from_host(gk, n, n, rp, ci, v, split=False)
    pc = solvers.jacobi_generate(gk, n, A.row_ptrs, A.col_idxs, A.vals, max_block_size=4)
    bd = dev(b[:, 0].copy())
    for precond in (None, pc):
        kw = dict(subspace_dim=4, max_iters=2000, reduction=1e-10, precond=precond, fused=True)
        base = solvers.idr_solve(gk, n, A.row_ptrs, A.col_idxs, A.vals, bd, **kw)
        assert base["converged"] and matgen.rel_err(host(base["x"]), xs) < 1e-7
        for fmt in ("csr", "ell", "coo"):
            M = A if fmt == "csr" else A.to(fmt)
            res = solvers.solve_op(gk, "idr", M, bd, **kw)
            assert res["converged"] and matgen.rel_err(host(res["x"]), xs) < 1e-7, fmt
            if fmt in ("csr", "ell"):
                assert res["iterations"] == base["iterations"] and host(res["x"]).tobytes() == host(base["x"]).tobytes()


@pytest.mark.parametrize("precond", ["none", "jacobi"])
def test_mirror_idr_solves_the_simple_solver_system(tmp_path, precond):
    """gko::solver::Idr<double> of the C++ mirror (deterministic subspace, s = 4) through examples/solve_mtx.cpp"""
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    ex = os.path.join(os.path.dirname(here), "repo-8852-ginkgo_amd", "examples")
    r = subprocess.run(["make", "-C", ex, "bin/solve_mtx"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    (tmp_path / "data").mkdir()
    for name in ("A", "b", "x0"):
        shutil.copy(os.path.join(here, "golden", f"simple_solver_{name}.mtx"), tmp_path / "data" / f"{name}.mtx")
    r = subprocess.run([os.path.join(ex, "bin", "solve_mtx"), "--executor", "hip", "--solver", "idr", "--precond", precond,
                        "--max-iters", "200", "--reduction", "1e-10", "--quiet"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    kv = {ln.split(":")[0]: ln.split(":", 1)[1].strip() for ln in r.stdout.splitlines() if ":" in ln}
    assert kv["solver"] == "idr" and 0 < int(kv["iterations"]) < 200 and float(kv["true residual norm"]) < 1e-8


def test_idr_shims_run_on_the_device(tmp_path):
    """the five kernels of core/solver/idr_kernels.hpp through their shim: one "ran idr::<kernel> ok" line each"""
    import subprocess
    from test_idr_reference import build_idr_shim_smoke
    run = subprocess.run([build_idr_shim_smoke(tmp_path)], capture_output=True, text=True)
    ran = {t[1]: t[2] for t in (ln.split() for ln in run.stdout.splitlines()) if len(t) == 3 and t[0] == "ran"}
    assert run.returncode == 0, run.stdout + run.stderr
    assert ran == {f"idr::{k}": "ok" for k in ("initialize", "step_1", "step_2", "step_3", "compute_omega")}, ran


def test_mirror_idr_with_a_random_subspace():
    """with_deterministic(false): P seeded from std::random_device, s = 3, kappa = 0.6, on a 500-row system"""
    import subprocess
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "repo-8852-ginkgo_amd", "examples")
    r = subprocess.run(["make", "-C", ex, "bin/idr_mirror"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(ex, "bin", "idr_mirror"), "solve"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    kv = {ln.split(":")[0]: ln.split(":", 1)[1].strip() for ln in r.stdout.splitlines() if ":" in ln}
    assert kv["converged"] == "yes" and 0 < int(kv["iterations"]) < 300 and float(kv["relative residual"]) <= 1.1e-10
