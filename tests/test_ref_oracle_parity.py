"""The C oracle and the Python restatements against the reference library's own
ReferenceExecutor (oracle/_ref/ref_driver, see ref_exec.py), bit for bit:
SpMV in every format, Dense BLAS-1, the conversions, the Csr operations and
matrix-data clean-up.  Factorizations, triangular solves, Jacobi and the
solvers are in test_ref_oracle_parity_solvers.py; the completeness table in
test_ref_oracle_table.py.

Comparison rule: every output is compared as integers; a NaN matches a NaN of
any sign and payload (ref_exec.assert_bits).  No case may skip where the
reference or oracle/_ref/ exists: a missing driver is a failure there."""
import itertools

import numpy as np
import pytest

import fbcsr_util
import formats_util
import ilu_exact_util as xu
import lu_util
import spgemm_util
import ref_exec
from ref_cases import Registry, ok, padded, rhs, run_case, spmv_matrices
from ref_exec import CSR, ELL, SELLP, HYBRID, COO, FBCSR, DENSE, assert_bits

REG = Registry()
FMT = {"csr": CSR, "ell": ELL, "sellp": SELLP, "hybrid": HYBRID, "coo": COO}
SCALARS = [0.0, 1.0, -1.0, 2.5]
MATS = spmv_matrices()


@pytest.fixture(scope="module")
def prepared(oracle):
    if ref_exec.may_skip():
        pytest.skip("neither the reference nor oracle/_ref/ is on this machine")
    return REG.prepare(oracle)


# ---- SpMV

def oracle_spmv(oracle, fmt, mat, nrhs, b, bs, c, cs, alpha=None, beta=None, apply2=False):
    """c (rows x cs buffer) <- the oracle's apply of `mat` held in format `fmt`."""
    m, n, rp, ci, v = mat
    adv = alpha is not None
    nnz = int(rp[-1])
    if fmt == "csr":
        if adv:
            oracle.ref_csr_advanced_spmv(m, nrhs, alpha, rp, ci, v, b, bs, beta, c, cs)
        else:
            oracle.ref_csr_spmv(m, nrhs, rp, ci, v, b, bs, c, cs)
    elif fmt == "ell":
        k, stride, cols, vals = formats_util.oracle_to_ell(oracle, m, rp, ci, v)
        if adv:
            oracle.ref_ell_advanced_spmv(m, nrhs, alpha, k, stride, cols, vals, b, bs, beta, c, cs)
        else:
            oracle.ref_ell_spmv(m, nrhs, k, stride, cols, vals, b, bs, c, cs)
    elif fmt == "sellp":
        sets, lens, cols, vals = formats_util.oracle_to_sellp(oracle, m, rp, ci, v)
        if adv:
            oracle.ref_sellp_advanced_spmv(m, nrhs, alpha, 64, sets, lens, cols, vals, b, bs, beta, c, cs)
        else:
            oracle.ref_sellp_spmv(m, nrhs, 64, sets, lens, cols, vals, b, bs, c, cs)
    elif fmt == "hybrid":
        # Hybrid::apply_impl: the Ell part's apply, then the Coo part's apply2
        h = formats_util.oracle_to_hybrid(oracle, m, n, rp, ci, v)
        if adv:
            oracle.ref_ell_advanced_spmv(m, nrhs, alpha, h["ell_lim"], h["ell_stride"], h["ell_cols"], h["ell_vals"],
                                         b, bs, beta, c, cs)
            oracle.ref_coo_advanced_spmv2(h["coo_nnz"], nrhs, alpha, h["coo_rows"], h["coo_cols"], h["coo_vals"],
                                          b, bs, c, cs)
        else:
            oracle.ref_ell_spmv(m, nrhs, h["ell_lim"], h["ell_stride"], h["ell_cols"], h["ell_vals"], b, bs, c, cs)
            oracle.ref_coo_spmv2(h["coo_nnz"], nrhs, h["coo_rows"], h["coo_cols"], h["coo_vals"], b, bs, c, cs)
    elif fmt == "coo":
        rows = np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))
        if apply2:
            if adv:
                oracle.ref_coo_advanced_spmv2(nnz, nrhs, alpha, rows, ci, v, b, bs, c, cs)
            else:
                oracle.ref_coo_spmv2(nnz, nrhs, rows, ci, v, b, bs, c, cs)
        elif adv:
            oracle.ref_coo_advanced_spmv(m, nnz, nrhs, alpha, rows, ci, v, b, bs, beta, c, cs)
        else:
            oracle.ref_coo_spmv(m, nnz, nrhs, rows, ci, v, b, bs, c, cs)
    else:
        raise KeyError(fmt)


def spmv_case(fmt, mname, nrhs, mode, alpha=None, beta=None, special_c=False):
    mat = MATS[mname]
    m, n, rp, ci, v = mat

    def build(oracle, batch):
        seed = len(mname) * 131 + nrhs
        bs, cs = nrhs + 2, nrhs + 3
        b = padded(rhs(n, nrhs, seed, special=mname == "special_values"), bs)
        c0 = padded(rhs(m, nrhs, seed + 1), cs)
        if special_c and m:
            c0[0, 0], c0[m // 2, nrhs - 1], c0[m - 1, 0] = np.nan, np.inf, -np.inf
        arrays, params = ref_exec.csr_arrays(m, n, rp, ci, v)
        arrays.update(b=b.reshape(-1), x=c0.reshape(-1))
        params.update(b_rows=n, b_cols=nrhs, b_stride=bs, x_rows=m, x_cols=nrhs, x_stride=cs,
                      fmt=FMT[fmt], mode=mode)
        if alpha is not None:
            params.update(alpha=alpha, beta=0.0 if beta is None else beta)
        idx = batch.add("spmv", arrays, **params)
        want = c0.copy()
        oracle_spmv(oracle, fmt, mat, nrhs, b, bs, want, cs, alpha, beta, apply2=mode >= 2)

        def check(results):
            assert_bits(want.reshape(-1), ok(results[idx])["x"], f"{fmt} {mname} nrhs={nrhs} mode={mode}")
            if fmt == "csr" and mode == 0 and m == n and 0 < m <= 200:
                with np.errstate(invalid="ignore"):
                    mine = lu_util.spmv((rp, ci, v), b[:, :nrhs])
                assert_bits(mine, results[idx]["x"].reshape(m, cs)[:, :nrhs], "lu_util.spmv")
        return check
    return build


def _register_spmv():
    rot = itertools.cycle(list(itertools.product(SCALARS, SCALARS)))
    for fmt in FMT:
        for mname in MATS:
            for nrhs in (1, 3, 17):
                REG.case(f"spmv-{fmt}-{mname}-{nrhs}-apply")(spmv_case(fmt, mname, nrhs, 0))
                a, be = next(rot)
                REG.case(f"spmv-{fmt}-{mname}-{nrhs}-advanced[{a},{be}]")(spmv_case(fmt, mname, nrhs, 1, a, be))
                if fmt == "coo":
                    REG.case(f"spmv-coo-{mname}-{nrhs}-apply2")(spmv_case(fmt, mname, nrhs, 2))
                    REG.case(f"spmv-coo-{mname}-{nrhs}-advanced_apply2[{a}]")(spmv_case(fmt, mname, nrhs, 3, a))
            # beta = 0 over a non-finite c: the reference multiplies (NaN stays) or overwrites?
            REG.case(f"spmv-{fmt}-{mname}-3-beta0-nonfinite-c")(spmv_case(fmt, mname, 3, 1, 2.5, 0.0, special_c=True))
        for a, be in itertools.product(SCALARS, SCALARS):
            REG.case(f"spmv-{fmt}-irregular-3-all[{a},{be}]")(spmv_case(fmt, "irregular", 3, 1, a, be, special_c=be == 0.0))


_register_spmv()


def csr_typed_case(mname, nrhs, vt, it, adv):
    """Csr<double,int64> and Csr<float,int32>."""
    m, n, rp, ci, v = MATS[mname]

    def build(oracle, batch):
        vdt = np.float32 if vt else np.float64
        idt = np.int64 if it else np.int32
        bs, cs = nrhs + 1, nrhs + 2
        b = padded(rhs(n, nrhs, 5, special=mname == "special_values").astype(vdt), bs)
        c0 = padded(rhs(m, nrhs, 6).astype(vdt), cs)
        vv = v.astype(vdt)
        arrays, params = ref_exec.csr_arrays(m, n, rp, ci, vv, vdt=vdt, idt=idt)
        arrays.update(b=b.reshape(-1), x=c0.reshape(-1))
        params.update(b_rows=n, b_cols=nrhs, b_stride=bs, x_rows=m, x_cols=nrhs, x_stride=cs, fmt=CSR,
                      mode=int(adv), vt=vt, it=it, alpha=-1.0, beta=2.5)
        idx = batch.add("spmv", arrays, **params)
        want = c0.copy()
        sfx = "_f32" if vt else ""
        if adv:
            getattr(oracle, "ref_csr_advanced_spmv" + sfx)(m, nrhs, -1.0, rp, ci, vv, b, bs, 2.5, want, cs)
        else:
            getattr(oracle, "ref_csr_spmv" + sfx)(m, nrhs, rp, ci, vv, b, bs, want, cs)

        def check(results):
            assert_bits(want.reshape(-1), ok(results[idx])["x"], f"csr vt={vt} it={it} {mname}")
        return check
    return build


for _m in MATS:
    for _vt, _it in ((0, 1), (1, 0)):
        for _nrhs in (1, 3):
            for _adv in (False, True):
                REG.case(f"spmv-csr-typed-{_m}-vt{_vt}-it{_it}-{_nrhs}-{'advanced' if _adv else 'apply'}")(
                    csr_typed_case(_m, _nrhs, _vt, _it, _adv))


# ---- Fbcsr: the Python restatement

def fbcsr_case(bs, nrhs, adv, sorted_rows):
    def build(oracle, batch):
        m, n, rp, ci, v = fbcsr_util.random_block_csr(9, 11, bs, [0, 3, 1, 0, 0, 11, 2, 5, 1], 40 + bs, sorted=sorted_rows)
        if bs == 3:
            v[0], v[5], v[9] = -0.0, np.inf, np.nan
        frp, fci, fv = fbcsr_util.csr_to_fbcsr(m, n, bs, rp, ci, v)
        b = rhs(n, nrhs, 9)
        c0 = rhs(m, nrhs, 10)
        a1, p1 = ref_exec.csr_arrays(m, n, rp, ci, v)
        conv = batch.add("convert", a1, fmt=FBCSR, bs=bs, **p1)
        bstr, cstr = nrhs + 1, nrhs + 2
        a2, p2 = ref_exec.csr_arrays(m, n, rp, ci, v)
        a2.update(b=padded(b, bstr).reshape(-1), x=padded(c0, cstr).reshape(-1))
        p2.update(b_rows=n, b_cols=nrhs, b_stride=bstr, x_rows=m, x_cols=nrhs, x_stride=cstr, fmt=FBCSR, bs=bs,
                  mode=int(adv), alpha=2.5, beta=-1.0)
        ap = batch.add("spmv", a2, **p2)
        want = fbcsr_util.spmv(bs, frp, fci, fv, b, c0 if adv else None, 2.5 if adv else None, -1.0 if adv else None)
        ops = {}
        fb = dict(rp=frp, ci=fci, v=fv)
        for op in range(6):
            ops[op] = batch.add("fbcsr_op", fb, m=m, n=n, bs=bs, op=op)

        def check(results):
            r = ok(results[conv])
            assert_bits(frp, r["fb_rp"], "convert_to_fbcsr row_ptrs")
            assert_bits(fci, r["fb_ci"], "convert_to_fbcsr col_idxs")
            assert_bits(fv, r["fb_v"], "convert_to_fbcsr values")
            back = fbcsr_util.to_csr(bs, frp, fci, fv)
            for k, w in zip(("back_rp", "back_ci", "back_v"), back):
                assert_bits(w, r[k], "fbcsr convert_to_csr " + k)
            assert_bits(padded(want, cstr)[:, :nrhs], ok(results[ap])["x"].reshape(m, cstr)[:, :nrhs], "fbcsr spmv")
            assert_bits(padded(c0, cstr)[:, nrhs:], results[ap]["x"].reshape(m, cstr)[:, nrhs:], "fbcsr spmv padding")
            t = ok(results[ops[0]])
            for k, w in zip(("fb_rp", "fb_ci", "fb_v"), fbcsr_util.transpose(n // bs, bs, frp, fci, fv)):
                assert_bits(w, t[k], "fbcsr transpose " + k)
            if bs == 1:     # the reference compiles its block sort for the sizes 2, 3, 4 and 7 only
                assert "unable to find an eligible kernel" in results[ops[1]]["error"]
            else:
                s = ok(results[ops[1]])
                sc, sv = fbcsr_util.sort(bs, frp, fci, fv)
                assert_bits(sc, s["fb_ci"], "fbcsr sort col_idxs")
                assert_bits(sv, s["fb_v"], "fbcsr sort values")
            assert bool(ok(results[ops[2]])["sorted"][0]) == fbcsr_util.is_sorted(frp, fci)
            assert_bits(fbcsr_util.extract_diagonal(n // bs, bs, frp, fci, fv), ok(results[ops[3]])["diag"], "fbcsr diag")
            for k, w in zip(("back_rp", "back_ci", "back_v"), back):
                assert_bits(w, ok(results[ops[4]])[k], "fbcsr to csr " + k)
            assert_bits(fbcsr_util.fill_in_dense(n // bs, bs, frp, fci, fv).reshape(-1), ok(results[ops[5]])["dense_v"],
                        "fbcsr fill_in_dense")
        return check
    return build


for _bs in (1, 2, 3, 4, 7):
    for _nrhs in (1, 3, 17):
        REG.case(f"fbcsr-bs{_bs}-nrhs{_nrhs}")(fbcsr_case(_bs, _nrhs, _nrhs != 1, _nrhs != 3))


def fbcsr_unsorted_blocks(oracle, batch):
    """block rows whose block columns are out of order and repeat: transpose, sort, is_sorted, diagonal"""
    bs = 2
    frp = np.array([0, 3, 3, 7, 8], np.int32)
    fci = np.array([2, 0, 2, 3, 1, 2, 0, 3], np.int32)
    fv = np.random.default_rng(3).uniform(-1, 1, 8 * bs * bs)
    fb = dict(rp=frp, ci=fci, v=fv)
    ops = {op: batch.add("fbcsr_op", fb, m=8, n=8, bs=bs, op=op) for op in range(4)}

    def check(results):
        for k, w in zip(("fb_rp", "fb_ci", "fb_v"), fbcsr_util.transpose(4, bs, frp, fci, fv)):
            assert_bits(w, ok(results[ops[0]])[k], "transpose " + k)
        sc, sv = fbcsr_util.sort(bs, frp, fci, fv)
        assert_bits(sc, ok(results[ops[1]])["fb_ci"], "sort col_idxs")
        assert_bits(sv, results[ops[1]]["fb_v"], "sort values")
        assert bool(ok(results[ops[2]])["sorted"][0]) == fbcsr_util.is_sorted(frp, fci)
        assert_bits(fbcsr_util.extract_diagonal(4, bs, frp, fci, fv), ok(results[ops[3]])["diag"], "diag")
    return check


REG.case("fbcsr-unsorted-blocks")(fbcsr_unsorted_blocks)


# ---- Dense BLAS-1

def dense_case(op, rows, cols, vt, per_column, special):
    def build(oracle, batch):
        dt = np.float32 if vt else np.float64
        sfx = "_f32" if vt else ""
        xs, ys = cols + 2, cols + 1
        x = padded(rhs(rows, cols, 20 + op, special).astype(dt), xs)
        y = padded(rhs(rows, cols, 30 + op, False).astype(dt), ys)
        if special and rows >= 8:
            y[2, 0], y[6, 0] = np.inf, 1.0
        acols = cols if per_column else 1
        alpha = np.array([SCALARS[(i + op) % 4] if not special else [2.5, -0.0, np.inf, np.nan][(i + op) % 4]
                          for i in range(acols)], dt).reshape(1, acols)
        if op == 1:
            alpha[alpha == 0] = 0.5 if not special else alpha[alpha == 0]
        arrays = dict(x=x.reshape(-1), y=y.reshape(-1), alpha=alpha.reshape(-1))
        params = dict(x_rows=rows, x_cols=cols, x_stride=xs, y_rows=rows, y_cols=cols, y_stride=ys,
                      alpha_rows=1, alpha_cols=acols, op=op, vt=vt)
        idx = batch.add("dense", arrays, **params)
        want = x.copy()
        res = np.full(cols, -5.0, dt)
        name = ["scale", "inv_scale", "add_scaled", "sub_scaled", "compute_dot", "compute_norm2", "compute_norm1"][op]
        fn = getattr(oracle, f"ref_dense_{name}{sfx}")
        if op <= 1:
            fn(rows, cols, alpha, acols, want, xs)
        elif op <= 3:     # the oracle's argument order is (source, destination)
            fn(rows, cols, alpha, acols, y, ys, want, xs)
        elif op == 4:
            fn(rows, cols, want, xs, y, ys, res)
        else:
            fn(rows, cols, want, xs, res)

        def check(results):
            r = ok(results[idx])
            if op <= 3:
                assert_bits(want.reshape(-1), r["x"], f"dense {name} {rows}x{cols} vt={vt}")
            else:
                assert_bits(res, r["r"], f"dense {name} {rows}x{cols} vt={vt}")
        return check
    return build


for _op in range(7):
    for _vt in (0, 1):
        if _op == 6 and _vt == 1:
            continue   # the oracle has no float norm1
        for _rows, _cols in ((0, 3), (1, 1), (257, 17), (1000, 3), (3001, 1)):
            for _pc in (False, True):
                REG.case(f"dense-op{_op}-vt{_vt}-{_rows}x{_cols}-{'percol' if _pc else 'scalar'}")(
                    dense_case(_op, _rows, _cols, _vt, _pc, False))
        REG.case(f"dense-op{_op}-vt{_vt}-special")(dense_case(_op, 64, 3, _vt, True, True))


# ---- conversions, Csr operations, matrix data

def convert_case(mname):
    m, n, rp, ci, v = MATS[mname]

    def build(oracle, batch):
        arrays, params = ref_exec.csr_arrays(m, n, rp, ci, v)
        idx = {f: batch.add("convert", arrays, fmt=code, **params) for f, code in FMT.items() if f != "csr"}
        idx["dense"] = batch.add("convert", arrays, fmt=DENSE, **params) if m * n <= 500000 else None
        idx["hybrid_cols"] = batch.add("convert", arrays, fmt=HYBRID, hyb_strategy=1, hyb_columns=3, **params)
        idx["hybrid_imb"] = batch.add("convert", arrays, fmt=HYBRID, hyb_strategy=2, hyb_percent=0.8, **params)
        idx["sellp_8_4"] = batch.add("convert", arrays, fmt=SELLP, slice_size=8, stride_factor=4, **params)
        ops = {op: batch.add("csr_op", arrays, op=op, **params) for op in range(4)}
        nnz = int(rp[-1])

        def check(results):
            k, stride, ecols, evals = formats_util.oracle_to_ell(oracle, m, rp, ci, v)
            r = ok(results[idx["ell"]])
            assert list(r["ell_meta"]) == [k, stride]
            assert_bits(ecols[:k * stride], r["ell_ci"], "ell col_idxs")
            assert_bits(evals[:k * stride], r["ell_v"], "ell values")
            for key, (ss, sf) in (("sellp", (64, 1)), ("sellp_8_4", (8, 4))):
                sets, lens, scols, svals = formats_util.oracle_to_sellp(oracle, m, rp, ci, v, ss, sf)
                nsl = (m + ss - 1) // ss
                total = int(sets[nsl]) * ss
                r = ok(results[idx[key]])
                assert_bits(sets.astype(np.int64), r["sellp_set"], key + " slice_sets")
                assert_bits(lens[:nsl].astype(np.int64), r["sellp_len"], key + " slice_lengths")
                # the rows that pad the last slice are never written: the reference leaves them uninitialised
                pos = np.arange(total)
                slice_of = np.searchsorted(sets[1:nsl + 1].astype(np.int64), pos // ss, side="right")
                live = slice_of * ss + pos % ss < m
                assert_bits(scols[:total][live], r["sellp_ci"][live], key + " col_idxs")
                assert_bits(svals[:total][live], r["sellp_v"][live], key + " values")
            rows = np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))
            r = ok(results[idx["coo"]])
            assert_bits(rows, r["coo_ri"], "coo row_idxs")
            assert_bits(ci, r["coo_ci"], "coo col_idxs")
            assert_bits(v, r["coo_v"], "coo values")
            for key, kw in (("hybrid", dict(kind=4)), ("hybrid_cols", dict(kind=0, num_columns=3)),
                            ("hybrid_imb", dict(kind=1, percent=0.8))):
                h = formats_util.oracle_to_hybrid(oracle, m, n, rp, ci, v, **kw)
                r = ok(results[idx[key]])
                assert list(r["ell_meta"]) == [h["ell_lim"], h["ell_stride"]], key
                sz = h["ell_lim"] * h["ell_stride"]
                assert_bits(h["ell_cols"][:sz], r["ell_ci"], key + " ell col_idxs")
                assert_bits(h["ell_vals"][:sz], r["ell_v"], key + " ell values")
                cn = h["coo_nnz"]
                assert_bits(h["coo_rows"][:cn], r["coo_ri"], key + " coo row_idxs")
                assert_bits(h["coo_cols"][:cn], r["coo_ci"], key + " coo col_idxs")
                assert_bits(h["coo_vals"][:cn], r["coo_v"], key + " coo values")
            if idx["dense"] is not None:
                d = np.zeros((m, n))
                for row in range(m):        # csr::fill_in_dense: the last of repeated columns stays
                    for z in range(rp[row], rp[row + 1]):
                        d[row, ci[z]] = v[z]
                assert_bits(d.reshape(-1), ok(results[idx["dense"]])["dense_v"], "dense values")
            # the way back: every format's convert_to(Csr)
            for key in ("ell", "sellp", "coo", "hybrid", "dense"):
                if idx.get(key) is None:
                    continue
                r = results[idx[key]]
                assert list(r["back_size"]) == [m, n]
                brp, bci, bv = r["back_rp"], r["back_ci"], r["back_v"]
                if key == "coo":
                    ptrs = np.zeros(m + 1, np.int32)
                    oracle.ref_convert_idxs_to_ptrs(rows, nnz, m, ptrs)
                    assert_bits(ptrs, brp, "coo->csr row_ptrs (convert_idxs_to_ptrs)")
                    assert_bits(rp, brp, "coo->csr row_ptrs")
                    assert_bits(ci, bci, "coo->csr col_idxs")
                    assert_bits(v, bv, "coo->csr values")
                else:
                    want = _back_from(key, m, n, rp, ci, v)
                    assert_bits(want[0], brp, key + "->csr row_ptrs")
                    assert_bits(want[1], bci, key + "->csr col_idxs")
                    assert_bits(want[2], bv, key + "->csr values")
            # csr operations
            trp, tci, tv = np.zeros(n + 1, np.int32), np.zeros(nnz, np.int32), np.zeros(nnz)
            oracle.ref_csr_transpose(m, n, rp, ci, v, trp, tci, tv)
            r = ok(results[ops[0]])
            assert_bits(trp, r["rp"], "transpose row_ptrs")
            assert_bits(tci, r["ci"], "transpose col_idxs")
            assert_bits(tv, r["v"], "transpose values")
            for k, w in zip(("rp", "ci", "v"), spgemm_util.transpose(m, n, (rp, ci, v))):
                assert_bits(w, r[k], "spgemm_util.transpose " + k)
            if m == n and m:
                for k, w in zip(("rp", "ci", "v"), xu.transpose((rp, ci, v))):
                    assert_bits(w, r[k], "ilu_exact_util.transpose " + k)
            sci, sv = ci.copy(), v.copy()
            oracle.ref_csr_sort_by_column_index(m, rp, sci, sv)
            r = ok(results[ops[1]])
            assert_bits(sci, r["ci"], "sort col_idxs")
            if len(np.unique(ci)) and not _has_repeats(rp, ci):
                assert_bits(sv, r["v"], "sort values")
            else:   # std::sort is not stable: equal columns may swap; the multiset per (row, col) must agree
                assert _sorted_groups(rp, sci, sv) == _sorted_groups(rp, r["ci"], r["v"])
            assert int(ok(results[ops[2]])["sorted"][0]) == int(oracle.ref_csr_is_sorted_by_column_index(m, rp, ci))
            diag = np.full(min(m, n), 0.0)
            oracle.ref_csr_extract_diagonal(min(m, n), rp, ci, v, diag)
            assert_bits(diag, ok(results[ops[3]])["diag"], "extract_diagonal")
        return check
    return build


def _has_repeats(rp, ci):
    return any(len(set(ci[rp[r]:rp[r + 1]].tolist())) != rp[r + 1] - rp[r] for r in range(len(rp) - 1))


def _sorted_groups(rp, ci, v):
    out = []
    for r in range(len(rp) - 1):
        out.append(sorted((int(c), float(x).hex()) for c, x in zip(ci[rp[r]:rp[r + 1]], v[rp[r]:rp[r + 1]])))
    return out


def _back_from(key, m, n, rp, ci, v):
    """What format -> Csr gives for a matrix that came from this Csr: ell,
    sellp and hybrid keep every entry with a valid column (stored zeros too)
    in the order of storage; dense keeps the last value of a repeated column,
    sorted by column, zeros dropped."""
    orp, oci, ov = [0], [], []
    for r in range(m):
        if key == "dense":
            row = {}
            for z in range(rp[r], rp[r + 1]):
                row[int(ci[z])] = v[z]
            items = sorted(row.items())
        else:
            items = [(int(ci[z]), v[z]) for z in range(rp[r], rp[r + 1])]
        for c, x in items:
            if key != "dense" or x != 0.0:      # is_nonzero: NaN counts as nonzero
                oci.append(c)
                ov.append(x)
        orp.append(len(oci))
    return np.array(orp, np.int32), np.array(oci, np.int32), np.array(ov, np.float64)


for _m in MATS:
    REG.case(f"convert-{_m}")(convert_case(_m))


def mdata_case(name, m, n, ri, ci, v):
    def build(oracle, batch):
        arrays = dict(ri=ri, ci=ci, v=v)
        idx = {op: batch.add("mdata", arrays, m=m, n=n, op=op) for op in range(3)}
        cnt = len(v)

        def check(results):
            orr, oc, ov = np.zeros(cnt, np.int32), np.zeros(cnt, np.int32), np.zeros(cnt)
            # device_matrix_data::sum_duplicates sorts (sort_row_major) before its kernel sums each run
            sr, sc, sv = ri.copy(), ci.copy(), v.copy()
            oracle.ref_matrix_data_sort_row_major(cnt, sr, sc, sv)
            k = int(oracle.ref_matrix_data_sum_duplicates(cnt, sr, sc, sv, orr, oc, ov))
            r = ok(results[idx[0]])
            assert_bits(orr[:k], r["ri"], name + " sum_duplicates rows")
            assert_bits(oc[:k], r["ci"], name + " sum_duplicates cols")
            assert_bits(ov[:k], r["v"], name + " sum_duplicates values")
            k = int(oracle.ref_matrix_data_remove_zeros(cnt, ri, ci, v, orr, oc, ov))
            r = ok(results[idx[1]])
            assert_bits(orr[:k], r["ri"], name + " remove_zeros rows")
            assert_bits(oc[:k], r["ci"], name + " remove_zeros cols")
            assert_bits(ov[:k], r["v"], name + " remove_zeros values")
            sr, sc, sv = ri.copy(), ci.copy(), v.copy()
            oracle.ref_matrix_data_sort_row_major(cnt, sr, sc, sv)
            r = ok(results[idx[2]])
            assert_bits(sr, r["ri"], name + " sort rows")
            assert_bits(sc, r["ci"], name + " sort cols")
            # equal (row, col) pairs may come out in any order of an unstable sort
            key = lambda a, b, c: sorted(zip(a.tolist(), b.tolist(), [float(x).hex() for x in c]))
            assert key(sr, sc, sv) == key(r["ri"], r["ci"], r["v"]), name + " sort values"
        return check
    return build


def _register_mdata():
    """The reference sorts with std::sort, which leaves entries of equal (row, column) in an unspecified order, and
    sum_duplicates adds each run in that order.  So the sums are compared where the order cannot matter: values that
    add exactly (multiples of 1/8), keys that repeat at most twice (0 + a + b == 0 + b + a), and 16 entries (below
    that size std::sort of libstdc++ is an insertion sort, which is stable)."""
    rng = np.random.default_rng(77)
    cnt = 3000
    ri = rng.integers(0, 40, cnt).astype(np.int32)
    ci = rng.integers(0, 30, cnt).astype(np.int32)
    v = rng.integers(-32, 33, cnt) / 8.0
    v[5], v[11], v[13], v[17] = -0.0, np.inf, np.nan, -np.inf
    REG.case("mdata-exact-sums-unsorted")(mdata_case("unsorted", 40, 30, ri, ci, v))
    order = np.lexsort((ci, ri))
    REG.case("mdata-exact-sums-sorted")(mdata_case("sorted", 40, 30, ri[order], ci[order], v[order]))
    keys = rng.permutation(np.repeat(rng.choice(40 * 30, 900, replace=False), 2))[:1500]
    v2 = rng.uniform(-1, 1, 1500)
    v2[::9] = 0.0
    REG.case("mdata-pairs")(mdata_case("pairs", 40, 30, (keys // 30).astype(np.int32), (keys % 30).astype(np.int32), v2))
    r16 = np.array([3, 1, 3, 0, 3, 1, 2, 3, 1, 0, 3, 2, 1, 3, 0, 1], np.int32)
    c16 = np.array([1, 2, 1, 0, 1, 2, 2, 0, 2, 0, 1, 2, 2, 0, 0, 2], np.int32)
    REG.case("mdata-16-runs")(mdata_case("16", 4, 4, r16, c16, rng.uniform(-1, 1, 16) * 10.0 ** rng.integers(-8, 8, 16)))
    REG.case("mdata-empty")(mdata_case("empty", 4, 4, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)))
    one = np.array([2], np.int32)
    REG.case("mdata-one")(mdata_case("one", 4, 4, one, one, np.array([0.0])))


_register_mdata()


def dense_fill_copy_gather(vt):
    def build(oracle, batch):
        dt = np.float32 if vt else np.float64
        sfx = "_f32" if vt else ""
        rows, cols, xs, ys = 37, 5, 8, 6
        x = padded(rhs(rows, cols, 50).astype(dt), xs)
        y = padded(rhs(rows, cols, 51, special=True).astype(dt), ys)
        base = dict(x_rows=rows, x_cols=cols, x_stride=xs, vt=vt)
        fill = batch.add("dense", dict(x=x.reshape(-1)), op=7, value=-0.0, **base)
        copy = batch.add("dense", dict(x=x.reshape(-1), y=y.reshape(-1)), op=8, y_rows=rows, y_cols=cols, y_stride=ys, **base)
        gather = None
        if not vt:
            pick = np.array([5, 0, 36, 5, 17], np.int32)
            g0 = padded(np.zeros((5, cols)), xs)
            gather = batch.add("dense", dict(x=g0.reshape(-1), y=y.reshape(-1), rows=pick), op=9, x_rows=5, x_cols=cols,
                               x_stride=xs, y_rows=rows, y_cols=cols, y_stride=ys)

        def check(results):
            want = x.copy()
            getattr(oracle, "ref_dense_fill" + sfx)(rows, cols, want, xs, -0.0)
            assert_bits(want.reshape(-1), ok(results[fill])["x"], "dense fill")
            want = x.copy()
            getattr(oracle, "ref_dense_copy" + sfx)(rows, cols, y, ys, want, xs)
            assert_bits(want.reshape(-1), ok(results[copy])["x"], "dense copy")
            if gather is not None:
                want = g0.copy()
                oracle.ref_dense_row_gather(5, cols, pick, y, ys, want, xs)
                assert_bits(want.reshape(-1), ok(results[gather])["x"], "dense row_gather")
        return check
    return build


REG.case("dense-fill-copy-gather-f64")(dense_fill_copy_gather(0))
REG.case("dense-fill-copy-f32")(dense_fill_copy_gather(1))


# ---- stopping criteria: one check() on given statuses

def criterion_case(kind, vt, set_finalized):
    def build(oracle, batch):
        dt = np.float32 if vt else np.float64
        nrhs = 9
        orig = np.array([1.0, 2.0, 0.5, 3.0, 1.0, 1.0, 7.0, 1e-3, 1.0], dt)
        red = dt(0.25)
        # below, exactly at and above the goal; a NaN; columns that already stopped or converged
        tau = np.array([0.2, 0.5, 0.2, 0.75, np.nan, 0.0, 1.75, 1e-5, np.inf], dt)
        if kind == 1:
            tau = (tau * tau).astype(dt)
            tau[3] = -tau[3]        # the implicit norm takes sqrt(abs(tau))
        status = np.array([0, 0, 0x03, 0, 0, 0x82, 0, 0, 0xc1], np.uint8)
        arrays = dict(b=orig.reshape(-1), tau=tau.reshape(-1), stop_status=status)
        idx = batch.add("criterion", arrays, kind=kind, vt=vt, reduction=float(red), b_rows=1, b_cols=nrhs,
                        tau_rows=1, tau_cols=nrhs, stopping_id=5, set_finalized=int(set_finalized), max_iters=4,
                        iteration=4)
        low = batch.add("criterion", arrays, kind=2, vt=vt, reduction=float(red), b_rows=1, b_cols=nrhs,
                        stopping_id=5, set_finalized=int(set_finalized), max_iters=4, iteration=3) if kind == 2 else None

        def check(results):
            st, flags = status.copy(), np.zeros(2, np.uint8)
            if kind == 0:
                getattr(oracle, "ref_residual_norm" + ("_f32" if vt else ""))(nrhs, tau, orig, red, 5, int(set_finalized), st, flags)
            elif kind == 1:
                oracle.ref_implicit_residual_norm(nrhs, tau, orig, red, 5, int(set_finalized), st, flags)
            else:       # Iteration::check_impl: at max_iters every column stops
                oracle.ref_set_all_statuses(nrhs, 5, int(set_finalized), st)
                flags[:] = 1
            r = ok(results[idx])
            assert_bits(st, r["stop_status"], f"criterion {kind} statuses")
            assert_bits(flags, r["flags"], f"criterion {kind} flags")
            if low is not None:
                r = ok(results[low])
                assert_bits(status, r["stop_status"], "Iteration below max_iters leaves the statuses")
                assert list(r["flags"]) == [0, 0]
        return check
    return build


for _fin in (False, True):
    REG.case(f"criterion-residual-norm-f64-fin{int(_fin)}")(criterion_case(0, 0, _fin))
    REG.case(f"criterion-residual-norm-f32-fin{int(_fin)}")(criterion_case(0, 1, _fin))
    REG.case(f"criterion-implicit-residual-norm-fin{int(_fin)}")(criterion_case(1, 0, _fin))
    REG.case(f"criterion-iteration-fin{int(_fin)}")(criterion_case(2, 0, _fin))


@pytest.mark.parametrize("name", REG.names())
def test_ref_parity(prepared, name):
    run_case(prepared, name)
