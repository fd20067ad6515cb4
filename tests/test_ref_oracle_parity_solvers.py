"""Second half of test_ref_oracle_parity.py: Csr x Csr, the factorizations,
triangular solves, Direct, Jacobi and the solvers -- the C oracle and the
Python restatements against the reference's own ReferenceExecutor, bit for bit
(iteration counts exactly)."""
import ctypes
import math

import numpy as np
import pytest

import exact_systems as exs
import idr_util
import ilu_exact_util as xu
import ilu_util
import lu_util
import matgen
import ref_exec
import spgemm_util
from ref_cases import Registry, golden_csr, grid_5pt_reversed, jacobi_written, ok, padded, rhs, rows_csr, run_case
from ref_exec import assert_bits

REG = Registry()
SCALARS = [0.0, 1.0, -1.0, 2.5]


@pytest.fixture(scope="module")
def prepared(oracle):
    if ref_exec.may_skip():
        pytest.skip("neither the reference nor oracle/_ref/ is on this machine")
    return REG.prepare(oracle)


def assert_csr(want, res, pre, what):
    for k, w in zip(("rp", "ci", "v"), want):
        assert_bits(np.asarray(w), res[pre + k], f"{what} {pre}{k}")


# ---- spgemm, advanced_spgemm, spgeam

def spgemm_case(name, a, b, c, ka, kb):
    """(rp, ci, v) triples: a is m x ka, b is ka x kb, c is m x kb"""
    m = len(a[0]) - 1

    def build(oracle, batch):
        arrays = {}
        params = {}
        for pre, mat, shape in (("a_", a, (m, ka)), ("b_", b, (ka, kb)), ("c_", c, (m, kb))):
            ar, pa = ref_exec.csr_arrays(shape[0], shape[1], *mat, pre=pre)
            arrays.update(ar)
            params.update(pa)
        plain = batch.add("spgemm", arrays, mode=0, **params)
        adv = {(al, be): batch.add("spgemm", arrays, mode=1, alpha=al, beta=be, **params)
               for al in SCALARS for be in SCALARS}
        geam = {}
        if ka == kb:    # alpha A I + beta C
            geam = {(al, be): batch.add("spgemm", arrays, mode=2, alpha=al, beta=be, **params)
                    for al in SCALARS for be in SCALARS}

        def check(results):
            assert_csr(spgemm_util.spgemm(a, b), ok(results[plain]), "c_", name + " spgemm")
            for (al, be), i in adv.items():
                assert_csr(spgemm_util.spgemm(a, b, al, be, c), ok(results[i]), "c_", f"{name} advanced[{al},{be}]")
            for (al, be), i in geam.items():
                assert_csr(spgemm_util.spgeam(al, a, be, c), ok(results[i]), "c_", f"{name} spgeam[{al},{be}]")
        return check
    return build


def _register_spgemm():
    rng = np.random.default_rng(5)
    tri = lambda t: (t[2], t[3], t[4])
    cnt = rng.integers(0, 7, 60)
    cnt[7:15] = 0
    cnt[40] = 60                                        # one dense row
    a = tri(rows_csr(60, 60, cnt, 1))
    b = tri(rows_csr(60, 60, rng.integers(0, 6, 60), 2))
    c = tri(rows_csr(60, 60, rng.integers(0, 6, 60), 3))
    REG.case("spgemm-square")(spgemm_case("square", a, b, c, 60, 60))
    a2 = tri(rows_csr(33, 17, rng.integers(0, 5, 33), 4, sort=False))
    b2 = tri(rows_csr(17, 29, rng.integers(0, 9, 17), 5, sort=False))
    c2 = tri(rows_csr(33, 29, rng.integers(0, 4, 33), 6))
    REG.case("spgemm-rectangular-unsorted")(spgemm_case("rect", a2, b2, c2, 17, 29))
    # cancellation to +0.0, explicit zeros, -0.0, inf and nan; repeated columns in A
    a3 = (np.array([0, 2, 4, 4, 6], np.int32), np.array([0, 1, 0, 1, 2, 2], np.int32),
          np.array([1.0, -1.0, 0.0, -0.0, np.inf, 2.0]))
    b3 = (np.array([0, 2, 4, 5, 5], np.int32), np.array([0, 3, 0, 3, 1], np.int32), np.array([2.0, 1.0, 2.0, np.nan, 0.0]))
    c3 = (np.array([0, 1, 2, 3, 4], np.int32), np.array([0, 1, 2, 3], np.int32), np.array([-0.0, 1.0, np.inf, 3.0]))
    REG.case("spgemm-special-values")(spgemm_case("special", a3, b3, c3, 4, 4))
    e = (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    REG.case("spgemm-empty")(spgemm_case("empty", e, e, e, 0, 0))


_register_spgemm()


# ---- factorizations, triangular solves, Direct

def factor_matrices():
    mats = {}
    mats["ani1"] = golden_csr("ani1")
    mats["ani4"] = golden_csr("ani4")
    mats["1138_bus"] = golden_csr("1138_bus")
    mats["grid20_reversed"] = grid_5pt_reversed(20)
    m = xu.random_dominant(150, 2, 9, 3)
    mats["random_dominant"] = (150,) + tuple(m)
    mats["unsymmetric_values"] = (200,) + tuple(lu_util.unsymmetric_values())
    mats["lu_zero_pivot"] = (4,) + tuple(lu_util.with_zero_pivot())
    # a zero and a tiny pivot: the diagonal is missing in one row, tiny in another
    n, rp, ci, v = matgen.poisson_2d_5pt(6)
    v = v.copy()
    rows = np.repeat(np.arange(n), np.diff(rp))
    v[(rows == 9) & (ci == 9)] = 0.0
    v[(rows == 20) & (ci == 20)] = 1e-300
    mats["zero_and_tiny_pivot"] = (n, rp, ci, v)
    keep = ~((rows == 13) & (ci == 13))
    rp2 = np.zeros(n + 1, np.int32)
    np.add.at(rp2, rows[keep] + 1, 1)
    mats["missing_diagonal"] = (n, np.cumsum(rp2).astype(np.int32), ci[keep], matgen.poisson_2d_5pt(6)[3][keep])
    return mats


FMATS = factor_matrices()
# Lu with symmetric_sparsity needs a symmetric pattern that holds the diagonal
LU_MATS = {"ani1", "1138_bus", "grid20_reversed", "zero_and_tiny_pivot", "unsymmetric_values", "lu_zero_pivot"}


def sorted_csr(oracle, n, rp, ci, v):
    ci, v = ci.copy(), v.copy()
    oracle.ref_csr_sort_by_column_index(n, rp, ci, v)
    return rp, ci, v


def factor_case(mname):
    n, rp, ci, v = FMATS[mname]

    def build(oracle, batch):
        arrays, params = ref_exec.csr_arrays(n, n, rp, ci, v)
        idx = {("parilu", it): batch.add("factor", arrays, kind=0, iterations=it, **params) for it in (0, 1, 3)}
        idx["paric"] = batch.add("factor", arrays, kind=1, iterations=1, **params)
        idx["ilu"] = batch.add("factor", arrays, kind=2, **params)
        idx["ic"] = batch.add("factor", arrays, kind=3, **params)
        b = rhs(n, 3, 8)
        if mname in LU_MATS:
            idx["lu"] = batch.add("factor", arrays, kind=4, symmetric=1, **params)
            da, dp = ref_exec.dense_arrays("b", b, 4)
            xa, xp = ref_exec.dense_arrays("x", np.zeros((n, 3)), 5)
            idx["direct"] = batch.add("direct", {**arrays, **da, **xa}, symmetric=1, **params, **dp, **xp)

        def check(results):
            srp, sci, sv = sorted_csr(oracle, n, rp, ci, v)       # generate() sorts first (skip_sorting = false)
            for it in (0, 1, 3):
                f = ilu_util.oracle_par_ilu(oracle, n, srp, sci, sv, it)
                r = ok(results[idx[("parilu", it)]])
                assert_csr(f["L"], r, "l_", f"{mname} ParIlu({it})")
                assert_csr(f["U"], r, "u_", f"{mname} ParIlu({it})")
            f = ilu_util.oracle_par_ic(oracle, n, srp, sci, sv)
            r = ok(results[idx["paric"]])
            assert_csr(f["L"], r, "l_", mname + " ParIc")
            assert_csr(f["Lt"], r, "u_", mname + " ParIc")
            L, U = xu.ilu_generate((rp, ci, v))
            r = ok(results[idx["ilu"]])
            assert_csr(L, r, "l_", mname + " Ilu")
            assert_csr(U, r, "u_", mname + " Ilu")
            L, Lt = xu.ic_generate((rp, ci, v))
            r = ok(results[idx["ic"]])
            assert_csr(L, r, "l_", mname + " Ic")
            assert_csr(Lt, r, "u_", mname + " Ic")
            if mname in LU_MATS:
                s = xu.sort_by_column_index((rp, ci, v))
                combined, _ = lu_util.lu_generate(s)
                r = ok(results[idx["lu"]])
                assert_csr(combined, r, "lu_", mname + " Lu")
                # symbolic Cholesky's row counts are the lower triangle of the reference's pattern, diagonal included
                rows_of = np.repeat(np.arange(n), np.diff(r["lu_rp"]))
                lower = np.bincount(rows_of[r["lu_ci"] <= rows_of], minlength=n).astype(np.int32)
                assert_bits(lu_util.cholesky_symbolic_count(s, lu_util.elimination_forest(s)), lower, mname + " row counts")
                x = lu_util.direct_apply(combined, b)
                got = ok(results[idx["direct"]])["x"].reshape(n, 5)
                assert_bits(x, got[:, :3], mname + " Direct")
                assert_bits(np.full((n, 2), -77.0), got[:, 3:], mname + " Direct padding")
        return check
    return build


for _m in FMATS:
    REG.case(f"factor-{_m}")(factor_case(_m))


def trs_case(mname, nrhs):
    n, rp, ci, v = FMATS[mname]

    def build(oracle, batch):
        srp, sci, sv = sorted_csr(oracle, n, rp, ci, v)
        f = ilu_util.oracle_par_ilu(oracle, n, srp, sci, sv, 1)
        b = rhs(n, nrhs, 12, special=mname == "ani1" and nrhs == 3)
        bs, xs = nrhs + 1, nrhs + 2
        idx = {}
        for upper, key in ((0, "L"), (1, "U")):
            frp, fci, fv = f[key]
            for unit in (0, 1):
                arrays, params = ref_exec.csr_arrays(n, n, frp, fci, fv)
                arrays.update(b=padded(b, bs).reshape(-1), x=padded(np.zeros((n, nrhs)), xs).reshape(-1))
                params.update(b_rows=n, b_cols=nrhs, b_stride=bs, x_rows=n, x_cols=nrhs, x_stride=xs)
                idx[(upper, unit)] = batch.add("trs", arrays, upper=upper, unit_diagonal=unit, **params)

        def check(results):
            for (upper, unit), i in idx.items():
                frp, fci, fv = f["U" if upper else "L"]
                x = padded(np.zeros((n, nrhs)), xs)
                fn = oracle.ref_upper_trs_solve if upper else oracle.ref_lower_trs_solve
                fn(n, nrhs, frp, fci, fv, unit, padded(b, bs), bs, x, xs)
                assert_bits(x.reshape(-1), ok(results[i])["x"], f"{mname} trs upper={upper} unit={unit} nrhs={nrhs}")
                # and the Python restatement that Direct's check is built from
                px = (lu_util.upper_trs if upper else lu_util.lower_trs)((frp, fci, fv), b, bool(unit))
                assert_bits(px, results[i]["x"].reshape(n, xs)[:, :nrhs], f"{mname} lu_util trs upper={upper} unit={unit}")
        return check
    return build


for _m in FMATS:
    for _nrhs in (1, 3, 17):
        REG.case(f"trs-{_m}-{_nrhs}")(trs_case(_m, _nrhs))


# ---- Jacobi

def jacobi_oracle(oracle, n, rp, ci, v, max_bs, adaptive, accuracy=0.1):
    ptrs = np.zeros(n + 1, np.int32)
    nb = int(oracle.ref_jacobi_find_blocks(n, rp, ci, max_bs, ptrs))
    scheme = np.zeros(3, np.int64)
    oracle.ref_jacobi_storage_scheme(max_bs, 32, scheme)       # the reference executor's max_block_stride is 32
    blocks = np.zeros(int(oracle.ref_jacobi_storage_space(scheme, nb)))
    cond = np.zeros(max(nb, 1))
    prec = np.full(max(nb, 1), 0xff, np.uint8)                  # 0xff asks for autodetection
    if adaptive:
        oracle.ref_jacobi_generate_adaptive(n, rp, ci, v, nb, scheme, ptrs, accuracy, cond, prec, blocks)
    else:
        oracle.ref_jacobi_generate(n, rp, ci, v, nb, scheme, ptrs, cond, blocks)
    return nb, ptrs[:nb + 1], scheme, blocks, cond[:nb], prec[:nb]


def jacobi_matrices():
    mats = {}
    n, rp, ci, v = golden_csr("ani1")
    mats["ani1"] = (n, rp, ci, v)
    mats["ani4"] = golden_csr("ani4")
    # natural blocks of mixed sizes, values over several magnitudes so that adaptive picks several precisions
    rng = np.random.default_rng(9)
    sizes = rng.integers(1, 14, 40)
    n = int(sizes.sum())
    a = np.zeros((n, n))
    at = 0
    for k, s in enumerate(sizes):
        blk = rng.uniform(-1, 1, (s, s)) + np.eye(s) * (s + 1)
        if k % 3 == 0:
            blk = np.round(blk * 4) / 4 + np.eye(s) * 8       # exactly representable in half: reduces far
        if k % 5 == 4:
            blk = blk * 10.0 ** rng.integers(-3, 4)
        a[at:at + s, at:at + s] = blk
        at += s
    n2, rp, ci, v = (n,) + tuple(xu.dense_to_csr(a))
    mats["natural_blocks"] = (n2, rp, ci, v)
    n, rp, ci, v = matgen.poisson_2d_5pt(9)
    v = v.copy()
    v[0] = 0.0        # a singular 1 x 1 block at max_block_size 1, and a zero on a block diagonal otherwise
    mats["grid9_zero_diagonal"] = (n, rp, ci, v)
    return mats


JMATS = jacobi_matrices()


def jacobi_case(mname, max_bs, adaptive):
    n, rp, ci, v = JMATS[mname]

    def build(oracle, batch):
        arrays, params = ref_exec.csr_arrays(n, n, rp, ci, v)
        nrhs = 3
        b = rhs(n, nrhs, 15)
        x0 = rhs(n, nrhs, 16)
        bs, xs = nrhs + 1, nrhs + 2
        arrays.update(b=padded(b, bs).reshape(-1), x=padded(x0, xs).reshape(-1))
        params.update(b_rows=n, b_cols=nrhs, b_stride=bs, x_rows=n, x_cols=nrhs, x_stride=xs,
                      max_block_size=max_bs, adaptive=int(adaptive), accuracy=0.1)
        simple = batch.add("jacobi", arrays, op=0, **params)
        adv = batch.add("jacobi", arrays, op=1, alpha=2.5, beta=-1.0, **params)
        tr = batch.add("jacobi", arrays, op=2, **params)

        def check_scalar(results):
            """max_block_size 1: the inverted diagonal, scalar applies; transpose copies it"""
            what = f"scalar jacobi {mname}"
            diag = np.zeros(n)
            oracle.ref_csr_extract_diagonal(n, rp, ci, v, diag)
            inv = np.zeros(n)
            oracle.ref_jacobi_invert_diagonal(n, diag, inv)
            pb = padded(b, bs)
            for i in (simple, adv, tr):
                assert_bits(inv, ok(results[i])["blocks"], what + " inverted diagonal")
            x = padded(x0, xs)
            oracle.ref_jacobi_simple_scalar_apply(n, nrhs, inv, pb, bs, x, xs)
            assert_bits(x.reshape(-1), results[simple]["x"], what + " apply")
            assert_bits(x.reshape(-1), results[tr]["x"], what + " transposed apply")
            x = padded(x0, xs)
            oracle.ref_jacobi_scalar_apply(n, nrhs, inv, 2.5, pb, bs, -1.0, x, xs)
            assert_bits(x.reshape(-1), results[adv]["x"], what + " advanced apply")

        def check(results):
            if max_bs == 1:
                return check_scalar(results)
            nb, ptrs, scheme, blocks, cond, prec = jacobi_oracle(oracle, n, rp, ci, v, max_bs, adaptive)
            r = ok(results[simple])
            what = f"jacobi {mname} max_bs={max_bs} adaptive={adaptive}"
            assert int(r["num_blocks"][0]) == nb, what
            assert_bits(ptrs, r["block_pointers"], what + " block pointers")
            assert_bits(scheme, r["scheme"], what + " storage scheme")
            if adaptive:
                assert_bits(prec, r["precisions"][:nb], what + " precisions")
            assert r["blocks"].size == blocks.size, what
            live = jacobi_written(scheme, ptrs, prec if adaptive else [], blocks.size * 8)
            assert_bits(blocks.view(np.uint8)[live], r["blocks"].view(np.uint8)[live], what + " block storage")
            if "conditioning" in r and adaptive:
                assert_bits(cond, r["conditioning"], what + " conditioning")
            x = padded(x0, xs)
            pb = padded(b, bs)
            if adaptive:
                oracle.ref_jacobi_apply_adaptive(nb, scheme, ptrs, prec, blocks, nrhs, 1.0, pb, bs, 0.0, x, xs)
            else:
                oracle.ref_jacobi_simple_apply(nb, scheme, ptrs, blocks, nrhs, pb, bs, x, xs)
            assert_bits(x.reshape(-1), r["x"], what + " apply")
            x = padded(x0, xs)
            if adaptive:
                oracle.ref_jacobi_apply_adaptive(nb, scheme, ptrs, prec, blocks, nrhs, 2.5, pb, bs, -1.0, x, xs)
            else:
                oracle.ref_jacobi_apply(nb, scheme, ptrs, blocks, nrhs, 2.5, pb, bs, -1.0, x, xs)
            assert_bits(x.reshape(-1), ok(results[adv])["x"], what + " advanced apply")
            tb = np.zeros_like(blocks)
            oracle.ref_jacobi_transpose(nb, scheme, ptrs, prec if adaptive else None, blocks, tb)
            x = padded(x0, xs)
            if adaptive:
                oracle.ref_jacobi_apply_adaptive(nb, scheme, ptrs, prec, tb, nrhs, 1.0, pb, bs, 0.0, x, xs)
            else:
                oracle.ref_jacobi_simple_apply(nb, scheme, ptrs, tb, nrhs, pb, bs, x, xs)
            assert_bits(x.reshape(-1), ok(results[tr])["x"], what + " transposed apply")
        return check
    return build


for _m in JMATS:
    for _bs in (1, 4, 13, 32):
        for _ad in (False, True):
            REG.case(f"jacobi-{_m}-{_bs}-{'adaptive' if _ad else 'plain'}")(jacobi_case(_m, _bs, _ad))


# ---- solvers

def systems():
    """The two systems of test_krylov_gpu.py."""
    out = {}
    n, rp, ci, v = matgen.poisson_2d_5pt(40)
    out["poisson40"] = (n, rp, ci, v)
    n, rp, ci, v = matgen.poisson_3d_7pt(12)
    v = v.copy()
    rows = np.repeat(np.arange(n), np.diff(rp))
    v[ci == rows - 1] -= 0.5
    v[ci == rows] += 0.5
    out["convection12"] = (n, rp, ci, v)
    return out


SYS = systems()
SOLVERS = {"cg": 0, "fcg": 1, "bicgstab": 2, "cgs": 3, "bicg": 4, "gmres": 5, "ir": 6, "idr": 7}


def deterministic_subspace(s, n):
    """Idr's deterministic subspace (core/solver/idr.cpp:159-164): matrix_data(size,
    std::normal_distribution<>(0, 1), std::default_random_engine(15)), row-major.  libstdc++:
    default_random_engine is minstd_rand0, generate_canonical<double, 53> takes two draws, normal_distribution is
    the polar method and hands out y * mult first, then the saved x * mult."""
    state = [15]
    R = 2147483646.0

    def draw():
        state[0] = state[0] * 16807 % 2147483647
        return state[0]

    def canonical():
        total = float(draw() - 1)
        total += float(draw() - 1) * R
        ret = total / (R * R)
        return math.nextafter(1.0, 0.0) if ret >= 1.0 else ret

    out = np.zeros(s * n)
    saved = None
    for i in range(s * n):
        if saved is not None:
            out[i], saved = saved, None
            continue
        while True:
            x = 2.0 * canonical() - 1.0
            y = 2.0 * canonical() - 1.0
            r2 = x * x + y * y
            if not (r2 > 1.0 or r2 == 0.0):
                break
        mult = math.sqrt(-2.0 * math.log(r2) / r2)
        saved = x * mult
        out[i] = y * mult
    return out.reshape(s, n)


def solver_case(solver, sysname, x0_kind, precond=0, **extra):
    n, rp, ci, v = SYS[sysname]

    def build(oracle, batch):
        xs = np.sin(0.3 * np.arange(n))
        b = np.zeros((n, 1))
        oracle.ref_csr_spmv(n, 1, rp, ci, v, xs.reshape(n, 1), 1, b, 1)
        x0 = np.zeros(n) if x0_kind == "zero" else np.cos(0.07 * np.arange(n))
        max_iters, reduction = extra.get("max_iters", 2000), 1e-10
        arrays, params = ref_exec.csr_arrays(n, n, rp, ci, v)
        arrays.update(b=b.reshape(-1), x=x0.copy())
        params.update(b_rows=n, b_cols=1, x_rows=n, x_cols=1, solver=SOLVERS[solver], precond=precond,
                      max_iters=max_iters, reduction=reduction)
        params.update({k: val for k, val in extra.items() if k != "max_iters"})
        if precond == 1:
            params.update(max_block_size=extra.get("max_block_size", 4))
        idx = batch.add("solve", arrays, **params)

        def precond_fn():
            if precond == 0:
                return None
            if precond == 1:
                nb, ptrs, scheme, blocks, _, _ = jacobi_oracle(oracle, n, rp, ci, v, params["max_block_size"], False)

                def app(w):
                    out = np.zeros_like(w)
                    oracle.ref_jacobi_simple_apply(nb, scheme, ptrs, blocks, w.shape[1], np.ascontiguousarray(w),
                                                   w.shape[1], out, w.shape[1])
                    return out
                return app
            f = ilu_util.oracle_par_ilu(oracle, n, rp, ci, v, 5) if precond == 2 else None
            L, U = (f["L"], f["U"]) if f else xu.ilu_generate((rp, ci, v))

            def app(w):
                w = np.ascontiguousarray(w)
                mid, out = np.zeros_like(w), np.zeros_like(w)
                oracle.ref_lower_trs_solve(n, w.shape[1], *L, 0, w, w.shape[1], mid, w.shape[1])
                oracle.ref_upper_trs_solve(n, w.shape[1], *U, 0, mid, w.shape[1], out, w.shape[1])
                return out
            return app

        def check(results):
            r = ok(results[idx])
            x = x0.copy()
            what = f"{solver} {sysname} x0={x0_kind} precond={precond}"
            app = precond_fn()
            if solver == "cg":
                it = oracle.ref_cg_solve(n, rp, ci, v, b[:, 0].copy(), x, max_iters, reduction, 0, None, 0)
            elif solver in ("fcg", "bicgstab", "cgs", "bicg"):
                it = getattr(oracle, f"ref_{solver}_solve")(n, rp, ci, v, b[:, 0].copy(), x, max_iters, reduction, 0)
            elif solver == "ir":
                it = oracle.ref_ir_solve(n, rp, ci, v, extra["relaxation_factor"], b[:, 0].copy(), x, max_iters,
                                         reduction, 0)
            elif solver == "gmres":
                keep, fnptr = None, None
                if app:
                    FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double),
                                          ctypes.POINTER(ctypes.c_double))

                    def cb(_, pin, pout):
                        np.ctypeslib.as_array(pout, shape=(n, 1))[:] = app(np.ctypeslib.as_array(pin, shape=(n, 1)).copy())
                        return 0
                    keep = FN(cb)
                    fnptr = ctypes.cast(keep, ctypes.c_void_p).value
                fr = np.zeros(1)
                # krylov_dim 0 asks the reference for its default of 100 (solver/gmres.hpp:144-151)
                it = oracle.ref_gmres_solve(n, rp, ci, v, fnptr, None, b[:, 0].copy(), x, extra["krylov_dim"] or 100,
                                            max_iters, reduction, 0, fr)
                assert_bits(fr, r["resnorm"], what + " final residual norm")
            else:
                s = extra.get("subspace_dim", 2)
                res = idr_util.solve(idr_util.csr_apply(oracle, n, rp, ci, v), b.copy(), deterministic_subspace(s, n),
                                     subspace_dim=s, kappa=extra.get("kappa", 0.7), max_iters=max_iters,
                                     reduction=reduction, precond=app, x=x.reshape(n, 1), literal=True)
                it, x = res["iterations"], res["x"][:, 0]
            assert int(r["iterations"][0]) == int(it), f"{what}: {int(it)} iterations, the reference {int(r['iterations'][0])}"
            assert_bits(x, r["x"], what + " x")
        return check
    return build


def _register_solvers():
    for sysname in SYS:
        for x0 in ("zero", "guess"):
            for solver in ("cg", "fcg", "bicgstab", "cgs", "bicg"):
                REG.case(f"solve-{solver}-{sysname}-{x0}")(solver_case(solver, sysname, x0))
            for kd in (0, 5, 30):
                REG.case(f"solve-gmres{kd}-{sysname}-{x0}")(solver_case("gmres", sysname, x0, krylov_dim=kd))
            REG.case(f"solve-ir-{sysname}-{x0}")(
                solver_case("ir", sysname, x0, relaxation_factor=0.24 if sysname == "poisson40" else 0.15, max_iters=300))
            for s, kappa in ((2, 0.7), (4, 0.5), (1, 0.7)):
                REG.case(f"solve-idr{s}-{sysname}-{x0}")(solver_case("idr", sysname, x0, subspace_dim=s, kappa=kappa,
                                                                    deterministic=1, max_iters=400))
        # the restatements that take a preconditioner: Gmres (a callback) and Idr
        for pc, pname in ((1, "jacobi"), (2, "parilu"), (3, "ilu")):
            REG.case(f"solve-gmres30-{sysname}-{pname}")(solver_case("gmres", sysname, "zero", pc, krylov_dim=30))
            REG.case(f"solve-idr2-{sysname}-{pname}")(solver_case("idr", sysname, "guess", pc, subspace_dim=2,
                                                                 deterministic=1, max_iters=400))


_register_solvers()


def cg_f32_case(sysname, x0_kind):
    n, rp, ci, v = SYS[sysname]

    def build(oracle, batch):
        v32 = v.astype(np.float32)
        b = np.sin(0.1 * np.arange(n)).astype(np.float32)
        x0 = np.zeros(n, np.float32) if x0_kind == "zero" else np.cos(0.07 * np.arange(n)).astype(np.float32)
        arrays, params = ref_exec.csr_arrays(n, n, rp, ci, v32, vdt=np.float32)
        arrays.update(b=b, x=x0.copy())
        idx = batch.add("solve", arrays, vt=1, solver=0, b_rows=n, b_cols=1, x_rows=n, x_cols=1, max_iters=500,
                        reduction=1e-5, **params)

        def check(results):
            x = x0.copy()
            it = oracle.ref_cg_solve_f32(n, rp, ci, v32, b, x, 500, 1e-5, 0)
            r = ok(results[idx])
            assert int(r["iterations"][0]) == int(it)
            assert_bits(x, r["x"], f"cg f32 {sysname} {x0_kind}")
        return check
    return build


for _x0 in ("zero", "guess"):
    REG.case(f"solve-cg-f32-poisson40-{_x0}")(cg_f32_case("poisson40", _x0))


# ---- the exact systems of tests/exact_systems.py: breakdown guards, zero right-hand sides, one-step convergence

def exact_case(solver, case):
    """One kept (solver, case) pair at the small size: iterations exactly, x and the residual norm the oracle reports
    as bits -- the all-NaN x of Gmres on a zero right-hand side included."""
    c = exs.CASES[case]
    n = c.sizes()[0]

    def build(oracle, batch):
        (_, rp, ci, v), b, x0 = c.build(n)
        f32, jacobi = solver == "cg_f32", solver == "cg_jacobi"
        dt = np.float32 if f32 else np.float64
        arrays, params = ref_exec.csr_arrays(n, n, rp, ci, v.astype(dt), vdt=dt)
        arrays.update(b=b.astype(dt), x=x0.astype(dt))
        params.update(b_rows=n, b_cols=1, x_rows=n, x_cols=1, solver=SOLVERS["cg" if f32 or jacobi else solver],
                      max_iters=c.max_iters, reduction=exs.REDUCTION, baseline=exs.BASELINES[c.baseline])
        if f32:
            params.update(vt=1)
        if jacobi:
            params.update(precond=1, max_block_size=1)
        if solver == "gmres":
            params.update(krylov_dim=c.krylov_dim)
        if solver == "ir":
            params.update(relaxation_factor=exs.IR_RELAXATION)
        idx = batch.add("solve", arrays, **params)

        def check(results):
            r = ok(results[idx])
            it, x, res = exs.run(oracle, solver, case, n)
            what = f"{solver} on {case}"
            assert int(r["iterations"][0]) == it, f"{what}: {it} iterations, the reference {int(r['iterations'][0])}"
            # the oracle reports no `converged`: on every one of these cases the limit is what ends an unconverged solve
            assert bool(r["converged"][0]) == (it < c.max_iters), what
            assert_bits(x, r["x"], what + " x")
            # the oracle's norm where it reports one, else the exact known |b - A x| (exs.run); the reference's Ir logs none
            if res is not None and solver != "ir":
                assert_bits(np.array([res], r["resnorm"].dtype), r["resnorm"], what + " final residual norm")
        return check
    return build


def exact_columns_case(solver, names):
    """Three different columns in one solve (exs.column_sets): iterations, x and, for Gmres, the residual norms of
    exs.solve_columns against the reference executor.  For Cg, Fcg, Bicgstab, Cgs, Bicg and Ir every column is its own
    single-column solve and the count is the largest.  Not for Gmres: there the column that stopped first receives its
    correction again at every later restart (exs.gmres_columns says why); the reference's result is the expectation."""
    n = exs.SMALL

    def build(oracle, batch):
        built = [exs.CASES[c].build(n) for c in names]
        _, rp, ci, v = built[0][0]
        b = np.stack([t[1] for t in built], 1)
        x0 = np.stack([t[2] for t in built], 1)
        arrays, params = ref_exec.csr_arrays(n, n, rp, ci, v)
        arrays.update(b=b.reshape(-1).copy(), x=x0.reshape(-1).copy())
        params.update(b_rows=n, b_cols=3, x_rows=n, x_cols=3, solver=SOLVERS[solver], max_iters=exs.MAX_ITERS,
                      reduction=exs.REDUCTION)
        if solver == "gmres":
            params.update(krylov_dim=5)
        if solver == "ir":
            params.update(relaxation_factor=exs.IR_RELAXATION)
        idx = batch.add("solve", arrays, **params)

        def check(results):
            r = ok(results[idx])
            it, x, res = exs.solve_columns(oracle, solver, names, n)
            what = f"{solver} on the columns {names}"
            assert int(r["iterations"][0]) == it, what
            assert_bits(x.reshape(-1), r["x"], what + " x")
            if res is not None:
                assert_bits(res, r["resnorm"].reshape(-1), what + " residual norms")
        return check
    return build


def exact_idr_case(case):
    """Idr on a case where every vector stays zero (b = 0, or an exact guess): the literal restatement with the
    reference's deterministic subspace.  On b = 0 the reference divides 0 by m_kk = 0 and returns NaN."""
    c = exs.CASES[case]
    n = c.sizes()[0]

    def build(oracle, batch):
        (_, rp, ci, v), b, x0 = c.build(n)
        arrays, params = ref_exec.csr_arrays(n, n, rp, ci, v)
        arrays.update(b=b.copy(), x=x0.copy())
        idx = batch.add("solve", arrays, b_rows=n, b_cols=1, x_rows=n, x_cols=1, solver=SOLVERS["idr"],
                        max_iters=c.max_iters, reduction=exs.REDUCTION, subspace_dim=exs.IDR_SUBSPACE_DIM,
                        kappa=exs.IDR_KAPPA, deterministic=1, **params)

        def check(results):
            r = ok(results[idx])
            with np.errstate(invalid="ignore"):
                res = idr_util.solve(idr_util.csr_apply(oracle, n, rp, ci, v), b.reshape(n, 1).copy(),
                                     deterministic_subspace(exs.IDR_SUBSPACE_DIM, n), subspace_dim=exs.IDR_SUBSPACE_DIM,
                                     kappa=exs.IDR_KAPPA, max_iters=c.max_iters, reduction=exs.REDUCTION,
                                     x=x0.reshape(n, 1).copy(), literal=True)
            assert int(r["iterations"][0]) == res["iterations"], case
            assert_bits(res["x"][:, 0].copy(), r["x"], f"idr on {case} x")
            # what the library's drivers do instead (literal=False, the subspace the GPU tests use) gives the same
            it, x, _ = exs.run(oracle, "idr", case, n)
            assert it == res["iterations"]
            assert_bits(x, r["x"], f"idr on {case}: the drivers' variant")
        return check
    return build


def _register_exact():
    for case in ("Z0", "E"):
        REG.case(f"exact-idr-{case}")(exact_idr_case(case))
    for solver, case in exs.pairs(exs.ALL7 + ("cg_f32", "cg_jacobi")):
        REG.case(f"exact-{solver}-{case}")(exact_case(solver, case))
    for solver in exs.ALL7:
        for names in exs.column_sets(solver):
            REG.case(f"exact-{solver}-columns-{'-'.join(names)}")(exact_columns_case(solver, names))


_register_exact()


@pytest.mark.parametrize("name", REG.names())
def test_ref_parity(prepared, name):
    run_case(prepared, name)
