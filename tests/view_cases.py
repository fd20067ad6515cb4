"""The cases of the layout sweep (tests/test_views_gpu.py) and its registry -- TEST INFRASTRUCTURE.

A case is one call of one C-ABI entry point on fixed data; the sweep runs it under every layout
of view_util.LAYOUTS that the case lists.  Importing this module needs neither a GPU nor torch:
tests/test_views_inventory.py checks on the CPU that the registry, together with the entry points
other tests cover, is every function of include/gkomi.h that takes a stride.

Per case:
  fn       the entry point without its gkomi_ prefix
  build    oracle -> {parameter name: value}; Mat / Vec / Work for pointers (view_util), plain
           numbers otherwise.  `*stride` parameters are left out: the layout supplies them.
  ref      oracle -> kernel(named) that computes the same call on the host twin with the same
           strides (the oracle, or the suite's Python restatement)
  tol      {operand: bound} for the entry points the suite holds to a tolerance: a number bounds
           matgen.rel_err, a function gives elementwise bounds (one with .pair set: error and bound).  "_order": the paths may sum in
           different orders, so no bit comparison with L0; "_twice": two runs must agree bit
           for bit; "_skip": operands the host reference does not compute
  state    (gk, args) -> {parameter name: value} built once on the device (plans, handles,
           callback contexts); may hold "_post": a check to run after every call
  targets  the dispatch predicate the case is there for
"""
import collections
import functools

import numpy as np

import formats_util as fu
import matgen
from krylov_util import KERNEL_ARGS
from view_util import LAYOUTS, Mat, Vec, Work, oracle_kernel

Case = collections.namedtuple("Case", "id fn build ref layouts tol state targets")
CASES = collections.OrderedDict()

ALL = [k for k in LAYOUTS if k != "L4" and not k.startswith("L6")]
ROTATE = [k for k in LAYOUTS if k.startswith("L6")]
F64, F32 = np.float64, np.float32


def add(fn, tag, build, ref=None, layouts=None, tol=None, state=None, targets="", column=False, vec_offset=False, rotate=False):
    """column: every Mat has one column, so the L4 layout applies.  vec_offset: also run the
    layouts with the Vec(offset=True) arrays of the case one element off ("+v"; a number: that
    many such arrays, also offset one at a time, "+v0", "+v1", ...).  rotate: more
    than two Mats, so the layouts that offset one operand at a time apply."""
    layouts = list(layouts or ALL) + (ROTATE if rotate else []) + (["L4"] if column else [])
    if vec_offset:
        layouts += ["L0+v", "L1a+v", "L2+v"] + ([f"L0+v{i}" for i in range(int(vec_offset))] if int(vec_offset) > 1 else [])
    cid = f"{fn}-{tag}"
    assert cid not in CASES, cid
    CASES[cid] = Case(cid, fn, functools.lru_cache(maxsize=None)(build), ref, layouts, tol or {}, state, targets)


def registry():
    return {"gkomi_" + c.fn for c in CASES.values()}


def _seed(*key):
    # hash() of a str changes from run to run: spell the key out
    return np.random.default_rng([sum(ord(ch) * (i + 1) for i, ch in enumerate(str(k))) for k in key])


STEP_SHAPES = [(n, k) for n in (1, 2, 513, 1030) for k in (1, 3)]


def _stop(nrhs):
    stop = np.zeros(nrhs, np.uint8)
    if nrhs > 2:
        stop[1] = 1          # a stopped column
    return stop


def _by_name(ref_name, alias=None):
    return lambda orc: oracle_kernel(orc, ref_name, alias)


# ---- dense elementwise, f64 and f32 ---------------------------------------------------------------------------------
def _dense_ew(sfx, dtype):
    o = "" if sfx == "_f64" else "_f32"
    flat = "dense.hip:92-95 (f32.hip twin)" if o else "dense.hip:92-95"
    for nr, nc in STEP_SHAPES:
        col = nc == 1
        for op in ("scale", "inv_scale", "add_scaled", "sub_scaled"):
            for acols in sorted({1, nc}):
                def build(orc, nr=nr, nc=nc, op=op, acols=acols):
                    rng = _seed("ew", op, nr, nc, acols)
                    args = collections.OrderedDict(nrows=nr, ncols=nc, alpha=Vec((rng.standard_normal(acols) + 2.5).astype(dtype)),
                                                   alpha_ncols=acols, x=Mat(rng.standard_normal((nr, nc)).astype(dtype)))
                    if op in ("add_scaled", "sub_scaled"):
                        args["y"] = Mat(rng.standard_normal((nr, nc)).astype(dtype))
                    return args
                add(f"dense_{op}{sfx}", f"{nr}x{nc}-a{acols}", build, _by_name(f"ref_dense_{op}{o}"), column=col,
                    targets=f"{flat}: contiguous && aligned(y) && aligned(x) && alpha_ncols == 1")
        add(f"dense_fill{sfx}", f"{nr}x{nc}", lambda orc, nr=nr, nc=nc: collections.OrderedDict(
            nrows=nr, ncols=nc, x=Mat(_seed("fill", nr, nc).standard_normal((nr, nc)).astype(dtype)), value=0.25),
            _by_name(f"ref_dense_fill{o}"), column=col, targets="dense.hip:334: stride == ncols && aligned(x)")
        add(f"dense_copy{sfx}", f"{nr}x{nc}", lambda orc, nr=nr, nc=nc: collections.OrderedDict(
            nrows=nr, ncols=nc, **{"in": Mat(_seed("copy", nr, nc).standard_normal((nr, nc)).astype(dtype)),
                                   "out": Mat(np.full((nr, nc), -3.0, dtype))}),
            _by_name(f"ref_dense_copy{o}"), column=col, targets="dense.hip:354-356: both contiguous && both aligned")


_dense_ew("_f64", F64)
_dense_ew("_f32", F32)

for nr, nc in STEP_SHAPES:
    add("dense_compute_sqrt_f64", f"{nr}x{nc}", lambda orc, nr=nr, nc=nc: collections.OrderedDict(
        nrows=nr, ncols=nc, x=Mat(np.abs(_seed("sqrt", nr, nc).standard_normal((nr, nc))))),
        _by_name("ref_dense_compute_sqrt"), column=nc == 1, targets="one kernel, strided")

    def _gather(orc, nr=nr, nc=nc):
        rng = _seed("gather", nr, nc)
        nin = nr + 4                      # at least four rows: the integer poison (3) stays a valid row
        return collections.OrderedDict(nout=nr, ncols=nc, rows=Vec(rng.integers(0, nin, size=nr).astype(np.int32)),
                                       **{"in": Mat(rng.standard_normal((nin, nc))), "out": Mat(np.zeros((nr, nc)))})
    add("dense_row_gather_f64_i32", f"{nr}x{nc}", _gather, _by_name("ref_dense_row_gather"), column=nc == 1,
        targets="one kernel, strided")

    for src, dst, fn in ((F64, F32, "dense_convert_f64_to_f32"), (F32, F64, "dense_convert_f32_to_f64")):
        def _conv(orc, nr=nr, nc=nc, src=src, dst=dst):
            a = (_seed("conv", nr, nc).standard_normal((nr, nc)) * 1e3).astype(src)
            return collections.OrderedDict(nrows=nr, ncols=nc, **{"in": Mat(a), "out": Mat(np.full((nr, nc), -777.25, dst))})

        def _conv_ref(orc):
            def kernel(a):
                nr, nc = a["nrows"], a["ncols"]
                src = a["in"][:nr * a["in_stride"]].reshape(nr, a["in_stride"])[:, :nc]
                with np.errstate(over="ignore"):
                    a["out"][:nr * a["out_stride"]].reshape(nr, a["out_stride"])[:, :nc] = src.astype(a["out"].dtype)
            return kernel
        add(fn, f"{nr}x{nc}", _conv, _conv_ref, column=nc == 1, targets="mixed.hip:73-75: contiguous && aligned(in) && aligned(out)")


# ---- CG and the other Krylov step kernels ---------------------------------------------------------------------------------
def _step_case(fn, ref, vecs, scalars, n, nrhs, dtype=F64, targets="krylov.hip: one kernel, strided", init=False, finalize=False):
    def build(orc):
        rng = _seed(fn, n, nrhs)
        args = collections.OrderedDict(n=n, nrows=n, nrhs=nrhs)
        for k in vecs:
            args[k] = Mat(rng.standard_normal((n, nrhs)).astype(dtype))
        for k in scalars:
            a = rng.standard_normal(nrhs).astype(dtype)
            if nrhs > 1 and not init:
                a[nrhs - 1] = 0.0          # zero denominators in the last column; the first one stays live
            args[k] = Vec(a)
        stop = np.ones(nrhs, np.uint8) if init else _stop(nrhs)
        if finalize:
            stop = np.array(([1, 65, 0] * nrhs)[:nrhs], np.uint8)
        args["stop_status"] = Vec(stop)
        return args

    def build_named(orc):
        # the header says n or nrows; keep only the one it has
        from view_util import header_params
        names = {p[2] for p in header_params(fn)}
        return collections.OrderedDict((k, v) for k, v in build(orc).items() if k in names)
    add(fn, f"{n}x{nrhs}", build_named, _by_name(ref, {"s": "s_vec"}), column=nrhs == 1, targets=targets, rotate=len(vecs) > 2)


CG_VEC = "cg.hip:181 / :206 (f32.hip twins): nrhs == 1 && every stride == 1 && every operand aligned"
for n, nrhs in STEP_SHAPES:
    for sfx, o, dt in (("_f64", "", F64), ("_f32", "_f32", F32)):
        _step_case(f"cg_initialize{sfx}", f"ref_cg_initialize{o}", ["b", "r", "z", "p", "q"], ["prev_rho", "rho"], n, nrhs, dt,
                   "one kernel, strided", init=True)
        _step_case(f"cg_step_1{sfx}", f"ref_cg_step_1{o}", ["p", "z"], ["rho", "prev_rho"], n, nrhs, dt, CG_VEC)
        _step_case(f"cg_step_2{sfx}", f"ref_cg_step_2{o}", ["x", "r", "p", "q"], ["beta", "rho"], n, nrhs, dt, CG_VEC)
    for (solver, op), (vecs, scalars) in sorted(KERNEL_ARGS.items()):
        hv = ["s_vec" if v == "s" else v for v in vecs]
        _step_case(f"{solver}_{op}_f64", f"ref_{solver}_{op}", hv, scalars, n, nrhs, targets="krylov.hip step kernels: strided",
                   finalize=op == "finalize")
    _step_case("bicgstab_initialize_f64", "ref_bicgstab_initialize", ["b", "r", "rr", "y", "s_vec", "t", "z", "v", "p"],
               ["prev_rho", "rho", "alpha", "beta", "gamma", "omega"], n, nrhs, init=True)
    _step_case("fcg_initialize_f64", "ref_fcg_initialize", ["b", "r", "z", "p", "q", "t"], ["prev_rho", "rho", "rho_t"], n, nrhs,
               init=True)
    _step_case("cgs_initialize_f64", "ref_cgs_initialize", ["b", "r", "r_tld", "p", "q", "u", "u_hat", "v_hat", "t"],
               ["alpha", "beta", "gamma", "prev_rho", "rho"], n, nrhs, init=True)
    _step_case("bicg_initialize_f64", "ref_bicg_initialize", ["b", "r", "z", "p", "q", "r2", "z2", "p2", "q2"],
               ["prev_rho", "rho"], n, nrhs, init=True)


# ---- SpMV of every format --------------------------------------------------------------------------------------------
MATS = {   # the two of tests/test_formats_gpu.py's MATS that the sweep uses
    "rand532x231": lambda: (532, 231) + matgen.random_csr(532, 231, 0, 40, seed=42),
    "empty_rows": lambda: (64 * 3 + 5, 50) + matgen.random_csr(64 * 3 + 5, 50, 0, 2, seed=8),
}
SPMV_NRHS = (1, 2, 3, 8, 15)
ALPHA, BETA = 2.0, -1.0
STREAM, SPMM = 1, 1 | (20 << 8)


@functools.lru_cache(maxsize=None)
def _mat(name):
    return MATS[name]()


def _bc(name, nrhs, adv, dtype=F64):
    n, nc = _mat(name)[:2]
    rng = _seed("spmv", name, nrhs)
    b = rng.standard_normal((nc, nrhs)).astype(dtype)
    c = rng.standard_normal((n, nrhs)).astype(dtype) if adv else np.full((n, nrhs), np.nan, dtype)
    sc = collections.OrderedDict(alpha=Vec(np.array([ALPHA], dtype)) if adv else None, beta=Vec(np.array([BETA], dtype)) if adv else None)
    return Mat(b), Mat(c), sc


def _csr_ref(adv, o=""):
    def ref(orc):
        def kernel(a):
            if adv:
                getattr(orc, "ref_csr_advanced_spmv" + o)(a["nrows"], a["nrhs"], float(a["alpha"][0]), a["row_ptrs"], a["col_idxs"], a["vals"],
                                                          a["b"], a["b_stride"], float(a["beta"][0]), a["c"], a["c_stride"])
            else:
                getattr(orc, "ref_csr_spmv" + o)(a["nrows"], a["nrhs"], a["row_ptrs"], a["col_idxs"], a["vals"], a["b"], a["b_stride"],
                                                 a["c"], a["c_stride"])
        return kernel
    return ref


def _spmv_ref(fmt, adv):
    """ref_<fmt>_spmv / ref_<fmt>_advanced_spmv, their parameters found by name"""
    def ref(orc):
        name = f"ref_{fmt}_advanced_spmv" if adv else f"ref_{fmt}_spmv"
        params = [p[2] for p in orc.protos[name][1]]

        def kernel(a):
            vals = []
            for p in params:
                v = a[p]
                vals.append(float(v[0]) if p in ("alpha", "beta") else v)
            getattr(orc, name)(*vals)
        return kernel
    return ref


def _csr64_ref(adv):
    def ref(orc):
        inner = _csr_ref(adv)(orc)
        return lambda a: inner(dict(a, row_ptrs=a["row_ptrs"].astype(np.int32), col_idxs=a["col_idxs"].astype(np.int32)))
    return ref


SPMM_VEC = "aligned(b) && aligned(c) && b_stride % 2 == 0 && c_stride % 2 == 0"
for mat in sorted(MATS):
    for adv in (False, True):
        for nrhs in SPMV_NRHS:
            tag = f"{mat}-{'advanced' if adv else 'simple'}-{nrhs}"
            col = nrhs == 1

            def _ell(orc, mat=mat, adv=adv, nrhs=nrhs):
                n, nc, rp, ci, v = _mat(mat)
                k, st, cols, vals = fu.oracle_to_ell(orc, n, rp, ci, v)
                b, c, sc = _bc(mat, nrhs, adv)
                return collections.OrderedDict(nrows=n, ncols=nc, nrhs=nrhs, num_stored_per_row=k, stride=st, col_idxs=Vec(cols),
                                               vals=Vec(vals), b=b, c=c, **sc)
            add("ell_spmv_f64_i32", tag, _ell, _spmv_ref("ell", adv), column=col, targets="formats.hip:281-282: " + SPMM_VEC)

            def _sellp(orc, mat=mat, adv=adv, nrhs=nrhs):
                n, nc, rp, ci, v = _mat(mat)
                sets, lens, cols, vals = fu.oracle_to_sellp(orc, n, rp, ci, v, 64, 1)
                b, c, sc = _bc(mat, nrhs, adv)
                return collections.OrderedDict(nrows=n, ncols=nc, nrhs=nrhs, slice_size=64, slice_sets=Vec(sets), slice_lengths=Vec(lens),
                                               col_idxs=Vec(cols), vals=Vec(vals), b=b, c=c, **sc)
            add("sellp_spmv_f64_i32", tag, _sellp, _spmv_ref("sellp", adv), column=col, targets="formats.hip:281-282: " + SPMM_VEC)

            def _coo(orc, mat=mat, adv=adv, nrhs=nrhs):
                n, nc, rp, ci, v = _mat(mat)
                nnz = int(rp[-1])
                rows = np.zeros(max(nnz, 1), np.int32)
                orc.ref_convert_ptrs_to_idxs(rp, n, rows)
                b, c, sc = _bc(mat, nrhs, adv)
                return collections.OrderedDict(nrows=n, ncols=nc, nrhs=nrhs, nnz=nnz, row_idxs=Vec(rows, True), col_idxs=Vec(ci, True),
                                               vals=Vec(v, True), b=b, c=c, **sc)
            # COO sums row segments with atomics: the bound of test_spmv_all_formats_vs_oracle
            add("coo_spmv_f64_i32", tag, _coo, _spmv_ref("coo", adv), column=col, tol={"c": 1e-14, "_order": True}, vec_offset=3,
                targets="formats.hip:476: aligned(vals, 16) && aligned(rows, 8) && aligned(cols, 8); coo_spmv.hip:536: aligned(b) && "
                        "b_stride % 2 == 0; coo_spmv.hip:564 -> fallback")

            def _hyb(orc, mat=mat, adv=adv, nrhs=nrhs):
                n, nc, rp, ci, v = _mat(mat)
                h = fu.oracle_to_hybrid(orc, n, nc, rp, ci, v, kind=0, num_columns=1)
                b, c, sc = _bc(mat, nrhs, adv)
                return collections.OrderedDict(
                    nrows=n, ncols=nc, nrhs=nrhs, ell_num_stored_per_row=h["ell_lim"], ell_stride=h["ell_stride"],
                    ell_col_idxs=Vec(h["ell_cols"]), ell_vals=Vec(h["ell_vals"]), coo_nnz=h["coo_nnz"], coo_row_idxs=Vec(h["coo_rows"], True),
                    coo_col_idxs=Vec(h["coo_cols"], True), coo_vals=Vec(h["coo_vals"], True), b=b, c=c, **sc)

            def _hyb_ref(orc, mat=mat, adv=adv):
                _, _, rp, ci, v = _mat(mat)
                inner = _csr_ref(adv)(orc)
                return lambda a: inner(dict(a, row_ptrs=rp, col_idxs=ci, vals=v))
            add("hybrid_spmv_f64_i32", tag, _hyb, _hyb_ref, column=col, tol={"c": 1e-14, "_order": True}, vec_offset=3,
                targets="formats.hip:281-282 (ELL part) and formats.hip:476 / coo_spmv.hip:564 (COO part)")

            # CSR: what test_several_right_hand_sides_read_the_matrix_once lacks -- offset bases of b and c
            def _csr(orc, mat=mat, adv=adv, nrhs=nrhs, idx=np.int32, dtype=F64, strategy=True):
                n, nc, rp, ci, v = _mat(mat)
                b, c, sc = _bc(mat, nrhs, adv, dtype)
                args = collections.OrderedDict(nrows=n, ncols=nc, nrhs=nrhs, nnz=int(rp[-1]), row_ptrs=Vec(rp.astype(idx)),
                                               col_idxs=Vec(ci.astype(idx)), vals=Vec(v.astype(dtype)), b=b, c=c, **sc)
                if strategy:
                    args.update(strategy=STREAM if nrhs == 1 else SPMM, max_row_nnz_hint=int(np.max(np.diff(rp))) if nrhs == 1 else 0)
                return args
            csr_layouts = ALL
            add("csr_spmv_f64_i32", tag, _csr, _csr_ref(adv), layouts=csr_layouts, column=col, targets="csr_spmv.hip:1123-1125: " + SPMM_VEC)
            if nrhs in (1, 3):
                add("csr_spmv_f64_i64", tag, functools.partial(_csr, idx=np.int64), _csr64_ref(adv), layouts=csr_layouts, column=col,
                    targets="csr_spmv.hip:1123-1125 (i64)")
                add("csr_spmv_f32_i32", tag, functools.partial(_csr, dtype=F32, strategy=False), _csr_ref(adv, "_f32"),
                    layouts=csr_layouts, column=col, targets="f32.hip: one kernel, strided")


# ---- dense reductions: tolerance against the exactly rounded sum of the rounded terms ---------------------------------------
RED_SHAPES = [(1, 1), (1, 3), (2051, 1), (2051, 3), (300001, 1)]   # 2051: three first-stage partials; 300001: 293, a second
                                                                  # trip of reduce_final_kernel's loop


def live2d(a, name, nr, nc, stride=None):
    st = a[name + "_stride"] if stride is None else stride
    return a[name][:nr * st].reshape(nr, st)[:, :nc]


def _red_terms(op, a):
    nr, nc = a["nrows"], a["ncols"]
    x = live2d(a, "x", nr, nc)
    if op == "dot":
        return x * live2d(a, "y", nr, nc)       # rounded in the working precision: numpy keeps the dtype
    return np.abs(x) if op == "norm1" else x * x


def _red_ref(op):
    def ref(orc):
        def kernel(a):
            from view_util import fsum_columns
            s = fsum_columns(_red_terms(op, a).astype(np.float64))
            a["result"][:a["ncols"]] = np.sqrt(s) if op == "norm2" else s
        return kernel
    return ref


def _red_bound(op):
    def bound(a, want):
        """4 eps max(1, sqrt(n)) sum|terms| (test_dense_reductions_vs_oracle; norm2: times the norm, as there)"""
        eps = np.finfo(a["x"].dtype).eps
        scale = np.abs(want.astype(np.float64)).reshape(-1) if op == "norm2" else \
            np.sum(np.abs(_red_terms(op, a).astype(np.float64)), axis=0)
        return (4 * eps * max(1.0, np.sqrt(a["nrows"])) * scale).reshape(want.shape)
    return bound


for sfx, dtype, ops in (("_f64", F64, ("dot", "norm2", "squared_norm2", "norm1")), ("_f32", F32, ("dot", "norm2"))):
    for op in ops:
        for nr, nc in RED_SHAPES:
            def _red(orc, op=op, nr=nr, nc=nc, dtype=dtype, sfx=sfx):
                rng = _seed("red", nr, nc)
                args = collections.OrderedDict(nrows=nr, ncols=nc, x=Mat(rng.standard_normal((nr, nc)).astype(dtype)))
                if op == "dot":
                    args["y"] = Mat(rng.standard_normal((nr, nc)).astype(dtype))
                args["result"] = Vec(np.full(nc, np.nan, dtype))
                wsfn = "dense_reduction_workspace_bytes" + ("" if sfx == "_f64" else "_f32")
                args["workspace"] = Work(lambda gk: getattr(gk, wsfn)(nr, nc))
                return args
            name = {"squared_norm2": "compute_squared_norm2"}.get(op, "compute_" + op)
            add(f"dense_{name}{sfx}", f"{nr}x{nc}", _red, _red_ref({"squared_norm2": "sqnorm"}.get(op, op)), column=nc == 1,
                tol={"result": _red_bound({"squared_norm2": "sqnorm"}.get(op, op)), "_twice": True, "_order": True},
                targets="dense.hip:295-299 (f32.hip twin): ncols == 1 && x_stride == 1 && y_stride == 1 && aligned(x) && aligned(y)")


# ---- COO: apply2 and the sorted kernels --------------------------------------------------------------------------------
def _coo_args(orc, mat, nrhs, adv, offset):
    n, nc, rp, ci, v = _mat(mat)
    nnz = int(rp[-1])
    rows = np.zeros(max(nnz, 1), np.int32)
    orc.ref_convert_ptrs_to_idxs(rp, n, rows)
    b, _, sc = _bc(mat, nrhs, adv)
    c = Mat(_seed("coo2", mat, nrhs).standard_normal((n, nrhs)))
    return collections.OrderedDict(nrows=n, ncols=nc, nrhs=nrhs, nnz=nnz, row_idxs=Vec(rows, offset), col_idxs=Vec(ci, offset),
                                   vals=Vec(v, offset), b=b, c=c), sc


def _spmv2_ref(adv):
    def ref(orc):
        def kernel(a):
            if adv:
                orc.ref_coo_advanced_spmv2(a["nnz"], a["nrhs"], float(a["alpha"][0]), a["row_idxs"], a["col_idxs"], a["vals"], a["b"],
                                           a["b_stride"], a["c"], a["c_stride"])
            else:
                orc.ref_coo_spmv2(a["nnz"], a["nrhs"], a["row_idxs"], a["col_idxs"], a["vals"], a["b"], a["b_stride"], a["c"],
                                  a["c_stride"])
        return kernel
    return ref


COO_TARGETS = ("formats.hip:476: aligned(vals, 16) && aligned(rows, 8) && aligned(cols, 8); coo_spmv.hip:536: aligned(b) && "
               "b_stride % 2 == 0; coo_spmv.hip:564 -> fallback")
for mat in sorted(MATS):
    for adv in (False, True):
        for nrhs in SPMV_NRHS:
            tag = f"{mat}-{'advanced' if adv else 'simple'}-{nrhs}"

            def _coo2(orc, mat=mat, adv=adv, nrhs=nrhs):
                args, sc = _coo_args(orc, mat, nrhs, adv, True)
                args["alpha"] = sc["alpha"]
                return args
            add("coo_spmv2_f64_i32", tag, _coo2, _spmv2_ref(adv), column=nrhs == 1, tol={"c": 1e-14, "_order": True}, vec_offset=3,
                targets=COO_TARGETS)

            def _sorted(orc, mat=mat, adv=adv, nrhs=nrhs, two=False):
                args, sc = _coo_args(orc, mat, nrhs, adv, False)
                if not two and not adv:
                    args["c"] = Mat(np.full(args["c"].a.shape, np.nan))
                args["alpha"] = sc["alpha"]
                if not two:
                    args["beta"] = sc["beta"]
                nnz = args["nnz"]
                args.update(max_row_nnz_hint=-1, workspace=Work(lambda gk: gk.coo_sorted_workspace_bytes(nnz, nrhs)))
                return args
            # the sorted kernels add partial sums per tile: the bound of test_sorted_against_the_oracle; no atomics
            tol = {"c": 1e-14, "_order": True, "_twice": True}
            add("coo_spmv_sorted_f64_i32", tag, _sorted, _spmv_ref("coo", adv), column=nrhs == 1, tol=tol,
                targets="coo_spmv.hip:536: aligned(b) && b_stride % 2 == 0 (the 8/4/2/1 column passes)")
            add("coo_spmv2_sorted_f64_i32", tag, functools.partial(_sorted, two=True), _spmv2_ref(adv), column=nrhs == 1, tol=tol,
                targets="coo_spmv.hip:536: aligned(b) && b_stride % 2 == 0 (the 8/4/2/1 column passes)")


# ---- Jacobi -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _jacobi(orc, max_bs, adaptive):
    from test_jacobi_gpu import block_structured_matrix     # the generator of the existing Jacobi tests
    n, rp, ci, v, _ = block_structured_matrix(67, max_bs, seed=max_bs)
    ptrs = np.zeros(n + 1, np.int32)
    nb = int(orc.ref_jacobi_find_blocks(n, rp, ci, max_bs, ptrs))
    scheme = np.zeros(3, np.int64)
    orc.ref_jacobi_storage_scheme(max_bs, 64, scheme)
    blocks = np.zeros(int(orc.ref_jacobi_storage_space(scheme, nb)))
    cond = np.zeros(max(nb, 1))
    prec = np.resize(np.array([0x01, 0x00, 0x02, 0x10, 0x11, 0x20, 0xff], np.uint8), max(nb, 1)).copy()
    if adaptive:
        orc.ref_jacobi_generate_adaptive(n, rp, ci, v, nb, scheme, ptrs, 1e-1, cond, prec, blocks)
    else:
        orc.ref_jacobi_generate(n, rp, ci, v, nb, scheme, ptrs, cond, blocks)
    return n, nb, scheme, ptrs, prec, blocks


def _ab(adv):
    return collections.OrderedDict(alpha=Vec(np.array([ALPHA])) if adv else None, beta=Vec(np.array([BETA])) if adv else None)


for max_bs in (4, 32):
    for nrhs in (1, 3):
        for adv in (False, True):
            tag = f"bs{max_bs}-{'advanced' if adv else 'simple'}-{nrhs}"
            for adaptive in (False, True):
                def _jac(orc, max_bs=max_bs, nrhs=nrhs, adv=adv, adaptive=adaptive):
                    n, nb, scheme, ptrs, prec, blocks = _jacobi(orc, max_bs, adaptive)
                    rng = _seed("jacobi", max_bs, nrhs)
                    args = collections.OrderedDict(num_blocks=nb, max_block_size=max_bs, block_ptrs=Vec(ptrs))
                    if adaptive:
                        args["block_precisions"] = Vec(prec)
                    args.update(blocks=Vec(blocks), nrhs=nrhs, b=Mat(rng.standard_normal((n, nrhs))), x=Mat(rng.standard_normal((n, nrhs))),
                                **_ab(adv))
                    return args

                def _jac_ref(orc, max_bs=max_bs, adv=adv, adaptive=adaptive):
                    scheme = _jacobi(orc, max_bs, adaptive)[2]

                    def kernel(a):
                        al, be = (float(a["alpha"][0]), float(a["beta"][0])) if adv else (1.0, 0.0)
                        tail = (a["nrhs"], al, a["b"], a["b_stride"], be, a["x"], a["x_stride"])
                        if adaptive:
                            orc.ref_jacobi_apply_adaptive(a["num_blocks"], scheme, a["block_ptrs"], a["block_precisions"], a["blocks"], *tail)
                        elif adv:
                            orc.ref_jacobi_apply(a["num_blocks"], scheme, a["block_ptrs"], a["blocks"], *tail)
                        else:
                            orc.ref_jacobi_simple_apply(a["num_blocks"], scheme, a["block_ptrs"], a["blocks"], a["nrhs"], a["b"], a["b_stride"],
                                                        a["x"], a["x_stride"])
                    return kernel
                add("jacobi_apply_adaptive_f64_i32" if adaptive else "jacobi_apply_f64_i32", tag, _jac, _jac_ref, column=nrhs == 1,
                    targets="jacobi.hip apply kernels: strided b and x")
    for nrhs in (1, 3):
        for adv in (False, True):
            def _sjac(orc, nrhs=nrhs, adv=adv, n=513 if max_bs == 4 else 1030):
                rng = _seed("sjacobi", n, nrhs)
                return collections.OrderedDict(nrows=n, nrhs=nrhs, inv_diag=Vec(rng.standard_normal(n) + 3), b=Mat(rng.standard_normal((n, nrhs))),
                                               x=Mat(rng.standard_normal((n, nrhs))), **_ab(adv))

            def _sjac_ref(orc, adv=adv):
                def kernel(a):
                    if adv:
                        orc.ref_jacobi_scalar_apply(a["nrows"], a["nrhs"], a["inv_diag"], float(a["alpha"][0]), a["b"], a["b_stride"],
                                                    float(a["beta"][0]), a["x"], a["x_stride"])
                    else:
                        orc.ref_jacobi_simple_scalar_apply(a["nrows"], a["nrhs"], a["inv_diag"], a["b"], a["b_stride"], a["x"], a["x_stride"])
                return kernel
            add("jacobi_scalar_apply_f64", f"{513 if max_bs == 4 else 1030}-{'advanced' if adv else 'simple'}-{nrhs}", _sjac, _sjac_ref,
                column=nrhs == 1, targets="jacobi.hip scalar apply: strided b and x")


# ---- triangular solves: direct, plan, bricks ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tri(lower, bricks):
    if bricks:
        from test_trs_bricks_analysis import triangle
        n, rp, ci, v = matgen.poisson_2d_5pt(70, 45)
        v = v * (1.0 + 0.3 * np.random.default_rng(n).random(len(v)))
        return (n,) + tuple(triangle(n, rp, ci, v, lower))
    from test_trs_ilu_gpu import random_triangular
    return (257,) + tuple(random_triangular(257, lower, seed=257))


def _trs_ref(lower, bricks):
    def ref(orc):
        n, rp, ci, v = _tri(lower, bricks)
        fn = orc.ref_lower_trs_solve if lower else orc.ref_upper_trs_solve
        return lambda a: fn(n, a["nrhs"], rp, ci, v, a["unit_diag"], a["b"], a["b_stride"], a["x"], a["x_stride"])
    return ref


def _overrun(check, what):
    """the post-call check: the solve did not hit its spin bound"""
    def post(gk, named):
        import ctypes
        import torch
        flag = ctypes.c_int(-1)
        getattr(gk, check)(torch.cuda.current_stream().cuda_stream, named[what], ctypes.addressof(flag))
        assert flag.value == 0, "triangular solve hit its spin bound"
    return post


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


for lower in (True, False):
    for nrhs in (1, 3):
        for unit in (0, 1):
            tag = f"{'unit' if unit else 'diag'}-{nrhs}"

            def _trs(orc, lower=lower, nrhs=nrhs, unit=unit, kind="direct"):
                n, rp, ci, v = _tri(lower, kind == "bricks")
                rng = _seed("trs", lower, nrhs)
                args = collections.OrderedDict(n=n, nrhs=nrhs, unit_diag=unit, b=Mat(rng.standard_normal((n, nrhs))),
                                               x=Mat(np.full((n, nrhs), 777.0)))
                if kind == "direct":
                    args.update(row_ptrs=Vec(rp), col_idxs=Vec(ci), vals=Vec(v), workspace=Work(lambda gk: gk.trs_workspace_bytes()))
                return args
            add("lower_trs_solve_f64_i32" if lower else "upper_trs_solve_f64_i32", tag, _trs, _trs_ref(lower, False), column=nrhs == 1,
                state=lambda gk, args: {"_post": _overrun("trs_check_overrun", "workspace")},
                targets="trs.hip: x polled through x_stride, b read through b_stride")

            def _plan_state(gk, args, lower=lower):
                from gkomi import solvers
                n, rp, ci, v = _tri(lower, False)
                tp = solvers.TrsPlan(gk, n, _dev(rp), _dev(ci), _dev(v), lower)
                return dict(plan=tp.plan, nslices=tp.nslices, entries=tp.entries, max_deps=tp.max_deps, _keep=tp,
                            _post=_overrun("trs_plan_check_overrun", "plan"))
            add("trs_solve_plan_f64", ("lower-" if lower else "upper-") + tag, functools.partial(_trs, kind="plan"), _trs_ref(lower, False),
                column=nrhs == 1, state=_plan_state, targets="trs_levels.hip: the analysed plan's solve, strided b and x")

            def _bricks_state(gk, args, lower=lower):
                from gkomi import solvers
                n, rp, ci, v = _tri(lower, True)
                bk = solvers.TrsBricks(gk, n, _dev(rp), _dev(ci), _dev(v), lower)
                return dict(h=bk.handle.value, plan=bk.plan, _keep=bk, _post=_overrun("trs_bricks_check_overrun", "plan"))
            add("trs_bricks_solve_f64", ("lower-" if lower else "upper-") + tag, functools.partial(_trs, kind="bricks"),
                _trs_ref(lower, True), column=nrhs == 1, state=_bricks_state, targets="trs_bricks.hip: the brick plan's solve, strided b and x")


# ---- dense GEMM and transpose ----------------------------------------------------------------------------------------------
def _gemm_shape(kind, i):
    """the i-th smallest non-empty shape that tests/test_dense_gemm_gpu.py uses for this kernel"""
    import gkomi
    import dense_gemm_util as du
    geo = du.geometry(gkomi.lib())
    shapes = du.split_shapes(geo) if kind == "split" else [s[1:] for s in du.ordered_shapes(geo) if s[0] == kind]
    shapes = sorted({s for s in shapes if s[0] * s[1] * s[2] > 0}, key=lambda s: (s[0] * s[1] * s[2], s))
    return shapes[i], geo


for kind in ("tile", "narrow", "split"):
    for i in (0, 1):
        for adv in (False, True):
            mode = 2 if kind == "split" else 1

            def _gemm(orc, kind=kind, i=i, adv=adv, mode=mode):
                import dense_gemm_util as du
                (m, n, k), _ = _gemm_shape(kind, i)
                a, b, c0 = du.operands(m, n, k, [m, n, k, 1], period=None)
                return collections.OrderedDict(m=m, n=n, k=k, a=Mat(a), b=Mat(b), c=Mat(c0 if adv else np.full((m, n), np.nan)),
                                               alpha=Vec(np.array([2.5])) if adv else None, beta=Vec(np.array([-1.0])) if adv else None,
                                               mode=mode, workspace=Work(lambda gk: gk.dense_gemm_workspace_bytes(m, n, k, mode)))

            def _gemm_ref(orc, kind=kind, i=i, adv=adv):
                import dense_gemm_util as du
                _, geo = _gemm_shape(kind, i)

                def kernel(x):
                    m, n, k = x["m"], x["n"], x["k"]
                    a, b, c = live2d(x, "a", m, k), live2d(x, "b", k, n), live2d(x, "c", m, n)
                    al, be = (2.5, -1.0) if adv else (None, None)
                    c[...] = du.split(a, b, c.copy(), al, be, chunk=geo["L"]) if kind == "split" else du.ordered(a, b, c.copy(), al, be)
                return kernel
            # ordered: the reference's bits; split: the chunked restatement's bits (test_split_equals_the_chunked_restatement)
            add("dense_gemm_f64", f"{kind}-{i}-{'advanced' if adv else 'simple'}", _gemm, _gemm_ref,
                targets="dense_gemm.hip: a_stride, b_stride, c_stride pairwise different, offset bases")

for rows, cols in ((1, 1), (63, 65), (65, 63), (1, 300), (300, 1)):
    def _tr(orc, rows=rows, cols=cols):
        a = np.random.default_rng(rows * 1000 + cols).standard_normal((rows, cols))
        a.flat[0] = -0.0
        return collections.OrderedDict(nrows=rows, ncols=cols, **{"in": Mat(a), "out": Mat(np.full((cols, rows), -77.0))})

    def _tr_ref(orc):
        def kernel(x):
            live2d(x, "out", x["ncols"], x["nrows"])[...] = live2d(x, "in", x["nrows"], x["ncols"]).T
        return kernel
    add("dense_transpose_f64", f"{rows}x{cols}", _tr, _tr_ref, targets="dense_gemm.hip transpose: in_stride != out_stride, offset bases")


def lv(a, name, sname, nr, nc):
    """the live nr x nc view of operand `name` whose stride parameter is called `sname`"""
    return live2d(a, name, nr, nc, a[sname])


# ---- GMRES helper kernels (oracle/gmres.c) ---------------------------------------------------------------------------------
GMRES_ALIAS = {"rnc": "residual_norm_collection", "gsin": "givens_sin", "gcos": "givens_cos", "hess": "hessenberg_iter",
               "before_precond": "before_preconditioner"}
R10 = 10 * np.finfo(np.float64).eps      # r<double>::value, the bound of test_hessenberg_qr_known_answers

for n, k in ((513, 3), (1030, 1)):
    d = 7

    def _g_init(orc, n=n, k=k, d=d):
        rng = _seed("gmres_init", n, k)
        return collections.OrderedDict(n=n, nrhs=k, krylov_dim=d, b=Mat(rng.standard_normal((n, k))), residual=Mat(np.zeros((n, k))),
                                       givens_sin=Vec(np.ones(d * k)), givens_cos=Vec(np.ones(d * k)), stop_status=Vec(np.full(k, 9, np.uint8)))
    add("gmres_initialize_f64", f"{n}x{k}", _g_init, _by_name("ref_gmres_initialize"), column=k == 1, targets="gmres.hip: strided b and residual")
    add("cb_gmres_initialize_f64", f"{n}x{k}", _g_init, _by_name("ref_gmres_initialize"), column=k == 1,
        targets="cb_gmres.hip: strided b and residual (the same operation as gmres::initialize)")

    def _g_restart(orc, n=n, k=k, d=d):
        b = _seed("gmres_restart", n, k).standard_normal((n, k))
        return collections.OrderedDict(n=n, nrhs=k, residual=Mat(b), residual_norm=Vec(np.sqrt((b * b).sum(axis=0))),
                                       residual_norm_collection=Vec(np.full((d + 1) * k, np.nan)), krylov_bases=Mat(np.full((n, k), 9999.0)),
                                       final_iter_nums=Vec(np.full(k, 999, np.uint64)))
    add("gmres_restart_f64", f"{n}x{k}", _g_restart, _by_name("ref_gmres_restart", GMRES_ALIAS), column=k == 1,
        targets="gmres.hip: r_stride != kb_stride")

    def _g_axpy(orc, n=n, k=k, d=d):
        rng = _seed("gmres_axpy", n, k)
        return collections.OrderedDict(n=n, nrhs=k, krylov_bases=Mat(rng.standard_normal(((d + 1) * n, k))), y=Vec(rng.standard_normal(d * k)),
                                       before_preconditioner=Mat(np.full((n, k), -5.0)), final_iter_nums=Vec(np.array([7, 3, 5][:k], np.uint64)),
                                       stop_status=Vec(np.array([0, 2, 0x42][:k], np.uint8)))
    add("gmres_multi_axpy_f64", f"{n}x{k}", _g_axpy, _by_name("ref_gmres_multi_axpy", GMRES_ALIAS), column=k == 1,
        targets="gmres.hip: kb_stride != bp_stride")

for k in (1, 3):
    d, it = 7, 3

    def _g_qr(orc, k=k, d=d, it=it):
        rng = _seed("gmres_qr", k)
        stop = np.zeros(k, np.uint8)
        stop[k // 2] = 2 if k > 1 else 0
        return collections.OrderedDict(nrhs=k, givens_sin=Vec(rng.standard_normal(d * k)), givens_cos=Vec(rng.standard_normal(d * k)),
                                       residual_norm=Vec(np.ones(k)), residual_norm_collection=Vec(rng.standard_normal((d + 1) * k)),
                                       hessenberg_iter=Mat(rng.standard_normal((it + 2, k))), iter=it,
                                       final_iter_nums=Vec(np.full(k, it, np.uint64)), stop_status=Vec(stop))
    # the suite holds hessenberg_qr to r<double> (hypot and the rotations may contract); between layouts: the same bits
    add("gmres_hessenberg_qr_f64", f"nrhs{k}", _g_qr, _by_name("ref_gmres_hessenberg_qr", GMRES_ALIAS), column=k == 1,
        tol={x: R10 for x in ("givens_sin", "givens_cos", "residual_norm", "residual_norm_collection", "hessenberg_iter")},
        targets="gmres.hip: h_stride > nrhs (a column block of the Hessenberg matrix)")

    def _g_sk(orc, k=k, d=d):
        rng = _seed("gmres_sk", k)
        h = rng.standard_normal((d + 1, d * k))
        for i in range(d):
            h[i, i * k:(i + 1) * k] += 4.0
        return collections.OrderedDict(nrhs=k, residual_norm_collection=Vec(rng.standard_normal((d + 1) * k)), hessenberg=Mat(h),
                                       y=Vec(np.full(d * k, 5.0)), final_iter_nums=Vec(np.array([d, 1, d - 2][:k], np.uint64)),
                                       stop_status=Vec(np.zeros(k, np.uint8)))
    add("gmres_solve_krylov_f64", f"nrhs{k}", _g_sk, _by_name("ref_gmres_solve_krylov", GMRES_ALIAS), tol={"y": R10},
        targets="gmres.hip: h_stride > krylov_dim * nrhs")


# ---- CB-GMRES kernels (tests/cb_gmres_util.py) -------------------------------------------------------------------------------
def _cb_sid(storage):
    import cb_gmres_util as cu
    return cu.STORAGES.index(storage)


for storage, n, k in (("keep", 64, 1), ("reduce1", 65, 3), ("ireduce1", 64, 3)):
    kd, it = 5, 2

    def _cb_givens(orc, k=k, kd=kd, it=it):
        rng = _seed("cb_givens", k)
        stop = np.zeros(k, np.uint8)
        stop[k // 2] = 0x42 if k > 1 else 0
        return collections.OrderedDict(nrhs=k, givens_sin=Vec(rng.standard_normal(kd * k)), givens_cos=Vec(rng.standard_normal(kd * k)),
                                       residual_norm=Vec(np.abs(rng.standard_normal(k))), residual_norm_collection=Vec(rng.standard_normal((kd + 1) * k)),
                                       hessenberg_iter=Mat(rng.standard_normal((it + 2, k))), iter=it, stop_status=Vec(stop))

    def _cb_givens_ref(orc, k=k, kd=kd, it=it):
        import cb_gmres_util as cu

        def kernel(a):
            cu.givens(a["givens_sin"][:kd * k].reshape(kd, k), a["givens_cos"][:kd * k].reshape(kd, k), a["residual_norm"],
                      a["residual_norm_collection"][:(kd + 1) * k].reshape(kd + 1, k), lv(a, "hessenberg_iter", "h_stride", it + 2, k), it,
                      (a["stop_status"][:k] & 0x3f) != 0)
        return kernel
    if storage != "ireduce1":
        add("cb_gmres_givens_f64", f"nrhs{k}", _cb_givens, _cb_givens_ref, column=k == 1, targets="cb_gmres.hip: h_stride > nrhs")

    def _cb_basis(rng, storage, n, k, kd):
        import cb_gmres_util as cu
        basis = cu.Basis(kd, n, k, storage, "rne")
        for j in range(kd + 1):
            for c in range(k):
                q = rng.standard_normal(n) / np.sqrt(n)
                basis.write_scalar(j, c, np.max(np.abs(q)))
                basis.write(j, c, q)
        return basis

    def _cb_sk(orc, storage=storage, n=n, k=k, kd=kd):
        rng = _seed("cb_sk", storage, n, k)
        basis = _cb_basis(rng, storage, n, k, kd)
        tri = rng.standard_normal((kd + 1, kd * k))
        for i in range(kd):
            tri[i, i * k:(i + 1) * k] += 4.0
        return collections.OrderedDict(n=n, nrhs=k, storage=_cb_sid(storage), residual_norm_collection=Vec(rng.standard_normal((kd + 1) * k)),
                                       krylov_bases=Vec(basis.data.reshape(-1)), scalars=Vec(basis.scalars.reshape(-1)), hessenberg=Mat(tri),
                                       y=Vec(np.zeros(kd * k)), before_preconditioner=Vec(np.full(n * k, 5.0)),
                                       final_iter_nums=Vec(np.array([kd, 1, kd - 2][:k], np.uint64)))

    def _cb_sk_ref(orc, storage=storage, n=n, k=k, kd=kd):
        import cb_gmres_util as cu

        def kernel(a):
            basis = cu.Basis(kd, n, k, storage, "rne")
            basis.data[...] = a["krylov_bases"][:basis.data.size].reshape(basis.data.shape)
            basis.scalars[...] = a["scalars"][:(kd + 1) * k].reshape(kd + 1, k)
            y, before = cu.solve_krylov(a["residual_norm_collection"][:(kd + 1) * k].reshape(kd + 1, k), basis,
                                        lv(a, "hessenberg", "h_stride", kd + 1, kd * k), a["final_iter_nums"])
            a["y"][:kd * k] = y.reshape(-1)
            a["before_preconditioner"][:n * k] = before.reshape(-1)
        return kernel
    add("cb_gmres_solve_krylov_f64", f"{storage}-{n}x{k}", _cb_sk, _cb_sk_ref, targets="cb_gmres.hip: h_stride > krylov_dim * nrhs")

    for fn in ("cb_gmres_finish_arnoldi_f64", "cb_gmres_arnoldi_f64"):
        def _cb_arn(orc, storage=storage, n=n, k=k, fn=fn):
            from test_cb_gmres_gpu import build_state, step_input      # the inputs of the existing finish_arnoldi tests
            kd, it = 30, 2
            state = build_state(n, k, kd, it, storage, 1)
            v_in = step_input(state, "natural", it)
            basis = state["basis"]
            stop = np.zeros(k, np.uint8)
            stop[k // 2] = 0x41 if k > 1 else 0
            args = collections.OrderedDict(n=n, nrhs=k, krylov_dim=kd, storage=_cb_sid(storage), next_krylov_basis=Vec(v_in, True))
            if fn == "cb_gmres_arnoldi_f64":
                args.update(givens_sin=Vec(state["gsin"]), givens_cos=Vec(state["gcos"]), residual_norm=Vec(state["rn"]),
                            residual_norm_collection=Vec(state["rnc"]))
            args.update(krylov_bases=Vec(basis.data.reshape(-1)), scalars=Vec(basis.scalars.reshape(-1)),
                        hessenberg_iter=Mat(np.full((kd + 1, k), 7.0)), buffer_iter=Vec(np.full((kd + 1) * k, 7.0)),
                        arnoldi_norm=Vec(np.full(3 * k, -1.0)), iter=it)
            if fn == "cb_gmres_arnoldi_f64":
                args["final_iter_nums"] = Vec(np.asarray(state["fin"], np.uint64))
            args.update(stop_status=Vec(stop), num_reorth=Vec(np.full(k, 99, np.int64)),
                        workspace=Work(lambda gk: gk.cb_gmres_step_workspace_bytes(k, kd)))
            return args
        # The existing suite holds these two to properties of the step (their sums run in the device's order), not to
        # bits, so there is no host twin: every layout must give the bits of the control and leave the poison alone.
        # "+v": next_krylov_basis 8 bytes off, the scalar side of vector_path(); compared with the control of the same offset.
        add(fn, f"{storage}-{n}x{k}", _cb_arn, None, vec_offset=True,
            targets="cb_gmres.hip:620 vector_path: nrhs == 1 && n * size % 16 == 0 && aligned(basis) && aligned(v0) && aligned(v1); h_stride > nrhs")


# ---- IDR step kernels (tests/idr_util.py) ----------------------------------------------------------------------------------
EPS = np.finfo(np.float64).eps


def _idr_data(n, nrhs, s, k):
    from test_idr_gpu import step_data          # the inputs of the existing step-kernel tests
    return step_data(n, nrhs, 0, s, 100 * s + n % 97 + k)


def _budget(key):
    """test_idr_gpu.budget: what a device sum in another order may be off by, against extended precision"""
    def pair(a, g, w):
        import matgen
        exact = a["_ld"][key].astype(np.float64)
        n = a["n"]
        return matgen.rel_err(g, exact), max(4 * EPS * np.sqrt(n), 4 * matgen.rel_err(w, exact))
    pair.pair = True
    return pair


for n, nrhs in ((513, 3), (1030, 1)):
    for s in (1, 4):
        wide = s * nrhs

        def _idr_init(orc, n=n, nrhs=nrhs, s=s):
            rng = _seed("idr_init", n, nrhs, s)
            return collections.OrderedDict(n=n, nrhs=nrhs, subspace_dim=s, m=Mat(np.full((s, s * nrhs), 7.0)),
                                           subspace_vectors=Mat(rng.standard_normal((s, n))), stop_status=Vec(np.ones(nrhs, np.uint8)))

        def _idr_init_ref(orc, n=n, nrhs=nrhs, s=s):
            import idr_util

            def kernel(a):
                m, p = lv(a, "m", "m_stride", s, s * nrhs), lv(a, "subspace_vectors", "subspace_stride", s, n)
                pld = p.astype(np.longdouble)
                idr_util.initialize(nrhs, np.zeros((s, s * nrhs), np.longdouble), pld, np.ones(nrhs, np.uint8))
                idr_util.initialize(nrhs, m, p, a["stop_status"])
                a["_ld"] = {"subspace_vectors": pld}
            return kernel
        add("idr_initialize_f64", f"{n}x{nrhs}-s{s}", _idr_init, _idr_init_ref, tol={"subspace_vectors": _budget("subspace_vectors")},
            targets="idr.hip: m_stride, subspace_stride")

        for k in sorted({0, s - 1}):

            def _idr1(orc, n=n, nrhs=nrhs, s=s, k=k):
                d, stop = _idr_data(n, nrhs, s, k)
                return collections.OrderedDict(n=n, nrhs=nrhs, subspace_dim=s, k=k, m=Mat(d["m"]), f=Mat(d["f"]), residual=Mat(d["residual"]),
                                               g=Mat(d["g"]), c=Mat(d["c"]), v=Mat(d["v"]), stop_status=Vec(stop))

            def _idr1_ref(orc, n=n, nrhs=nrhs, s=s, k=k):
                import idr_util
                w = s * nrhs
                return lambda a: idr_util.step_1(nrhs, k, lv(a, "m", "m_stride", s, w), lv(a, "f", "f_stride", s, nrhs),
                                                 lv(a, "residual", "residual_stride", n, nrhs), lv(a, "g", "g_stride", n, w),
                                                 lv(a, "c", "c_stride", s, nrhs), lv(a, "v", "v_stride", n, nrhs), a["stop_status"])
            add("idr_step_1_f64", f"{n}x{nrhs}-s{s}-k{k}", _idr1, _idr1_ref, targets="idr.hip: six strides, pairwise different")

            def _idr2(orc, n=n, nrhs=nrhs, s=s, k=k):
                d, stop = _idr_data(n, nrhs, s, k)
                return collections.OrderedDict(n=n, nrhs=nrhs, subspace_dim=s, k=k, omega=Vec(d["omega"]), preconditioned_vector=Mat(d["pv"]),
                                               c=Mat(d["c"]), u=Mat(d["u"]), stop_status=Vec(stop))

            def _idr2_ref(orc, n=n, nrhs=nrhs, s=s, k=k):
                import idr_util
                w = s * nrhs
                return lambda a: idr_util.step_2(nrhs, k, a["omega"], lv(a, "preconditioned_vector", "pv_stride", n, nrhs),
                                                 lv(a, "c", "c_stride", s, nrhs), lv(a, "u", "u_stride", n, w), a["stop_status"])
            add("idr_step_2_f64", f"{n}x{nrhs}-s{s}-k{k}", _idr2, _idr2_ref, targets="idr.hip: pv_stride, c_stride, u_stride")

            def _idr3(orc, n=n, nrhs=nrhs, s=s, k=k):
                d, stop = _idr_data(n, nrhs, s, k)
                return collections.OrderedDict(n=n, nrhs=nrhs, subspace_dim=s, k=k, subspace_vectors=Mat(d["p"]), g=Mat(d["g"]), g_k=Mat(d["g_k"]),
                                               u=Mat(d["u"]), m=Mat(d["m"]), f=Mat(d["f"]), alpha=Vec(np.zeros(nrhs)), residual=Mat(d["residual"]),
                                               x=Mat(d["x"]), stop_status=Vec(stop),
                                               workspace=Work(lambda gk: gk.idr_step_3_workspace_bytes(nrhs, s)))

            def _idr3_ref(orc, n=n, nrhs=nrhs, s=s, k=k):
                import idr_util
                w = s * nrhs
                names = (("subspace_vectors", "subspace_stride", s, n), ("g", "g_stride", n, w), ("g_k", "g_k_stride", n, nrhs),
                         ("u", "u_stride", n, w), ("m", "m_stride", s, w), ("f", "f_stride", s, nrhs), ("residual", "residual_stride", n, nrhs),
                         ("x", "x_stride", n, nrhs))

                def kernel(a):
                    views = [lv(a, *nm) for nm in names]
                    ld = [v.astype(np.longdouble) for v in views]
                    idr_util.step_3(nrhs, k, *ld, a["stop_status"])
                    idr_util.step_3(nrhs, k, *views, a["stop_status"])
                    a["_ld"] = {nm[0]: x for nm, x in zip(names, ld)}
                return kernel
            # sums over the rows in the device's order: test_step_3_within_the_error_of_a_reordered_sum's budget per output;
            # alpha and g_k are scratch of the kernel
            add("idr_step_3_f64", f"{n}x{nrhs}-s{s}-k{k}", _idr3, _idr3_ref,
                tol=dict({x: _budget(x) for x in ("g", "u", "m", "f", "residual", "x")}, _skip=("alpha", "g_k")),
                targets="idr.hip: ten operands, strides pairwise different")


# ---- multigrid K-cycle kernels (tests/multigrid_util.py) ---------------------------------------------------------------------
for n, nrhs in STEP_SHAPES:
    def _kc(orc, n=n, nrhs=nrhs, step=1):
        import multigrid_util as mu
        alpha, rho, gamma, beta, zeta, v, g, d, e = mu.kcycle_operands(n, nrhs)
        args = collections.OrderedDict(nrows=n, nrhs=nrhs, alpha=Vec(alpha), rho=Vec(rho))
        if step == 1:
            args.update(v=Mat(v), g=Mat(g), d=Mat(d), e=Mat(e))
        else:
            args.update(gamma=Vec(gamma), beta=Vec(beta), zeta=Vec(zeta), d=Mat(d), e=Mat(e))
        return args

    def _kc_ref(orc, n=n, nrhs=nrhs, step=1):
        import multigrid_util as mu

        def kernel(a):
            m = lambda name: live2d(a, name, n, nrhs)
            if step == 1:
                mu.kcycle_step_1(a["alpha"], a["rho"], m("v"), m("g"), m("d"), m("e"))
            else:
                mu.kcycle_step_2(a["alpha"], a["rho"], a["gamma"], a["beta"], a["zeta"], m("d"), m("e"))
        return kernel
    add("multigrid_kcycle_step_1_f64", f"{n}x{nrhs}", _kc, _kc_ref, column=nrhs == 1, targets="multigrid.hip: v, g, d, e strides pairwise different")
    add("multigrid_kcycle_step_2_f64", f"{n}x{nrhs}", functools.partial(_kc, step=2), functools.partial(_kc_ref, step=2), column=nrhs == 1,
        targets="multigrid.hip: d_stride != e_stride")


# ---- Fbcsr -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fbcsr(bs):
    import fbcsr_util
    nbrows, nbcols = 40, 23
    nrows, ncols, rp, ci, v = fbcsr_util.random_block_csr(nbrows, nbcols, bs, 4, seed=bs)
    return (nbrows, nbcols) + tuple(fbcsr_util.csr_to_fbcsr(nrows, ncols, bs, rp, ci, v))


def _fb_ref(bs, adv):
    def ref(orc):
        import fbcsr_util
        nbrows, nbcols, rp, ci, vals = _fbcsr(bs)

        def kernel(a):
            nrhs = a["nrhs"]
            b, c = live2d(a, "b", nbcols * bs, nrhs), live2d(a, "c", nbrows * bs, nrhs)
            c[...] = fbcsr_util.spmv(bs, rp, ci, vals, b, c.copy(), ALPHA if adv else None, BETA if adv else None)
        return kernel
    return ref


for bs in (3, 5):                 # 3: an instantiated block size; 5: the run-time one
    for nrhs in (1, 3):
        for adv in (False, True):
            def _fb(orc, bs=bs, nrhs=nrhs, adv=adv):
                nbrows, nbcols, rp, ci, vals = _fbcsr(bs)
                rng = _seed("fbcsr", bs, nrhs)
                return collections.OrderedDict(nbrows=nbrows, nbcols=nbcols, bs=bs, nbnz=len(ci), row_ptrs=Vec(rp), col_idxs=Vec(ci), vals=Vec(vals, True),
                                               b=Mat(rng.standard_normal((nbcols * bs, nrhs))), nrhs=nrhs,
                                               c=Mat(rng.standard_normal((nbrows * bs, nrhs)) if adv else np.full((nbrows * bs, nrhs), np.nan)), **_ab(adv))
            # "+v": vals 8 bytes off a 16-byte boundary, which Fbcsr accepts (fbcsr.hip:477 refuses only what is off 8)
            add("fbcsr_spmv_f64_i32", f"bs{bs}-{'advanced' if adv else 'simple'}-{nrhs}", _fb, _fb_ref(bs, adv), column=nrhs == 1, vec_offset=True,
                targets="fbcsr.hip: strided b and c; the value stream's pairs shift with vals % 16")

    def _fill(orc, bs=bs):
        nbrows, nbcols, rp, ci, vals = _fbcsr(bs)
        return collections.OrderedDict(nbrows=nbrows, nbcols=nbcols, bs=bs, nbnz=len(ci), row_ptrs=Vec(rp), col_idxs=Vec(ci), vals=Vec(vals),
                                       result=Mat(np.zeros((nbrows * bs, nbcols * bs))))

    def _fill_ref(orc, bs=bs):
        import fbcsr_util
        nbrows, nbcols, rp, ci, vals = _fbcsr(bs)

        def kernel(a):
            lv(a, "result", "result_stride", nbrows * bs, nbcols * bs)[...] = fbcsr_util.fill_in_dense(nbcols, bs, rp, ci, vals)
        return kernel
    add("fbcsr_fill_in_dense_f64_i32", f"bs{bs}", _fill, _fill_ref, targets="fbcsr.hip: result_stride > ncols, offset base")


# ---- CSR with srow, the column-partitioned copy, the apply callbacks ---------------------------------------------------------------
def _apply_args(mat, nrhs, adv, orc=None):
    b, c, sc = _bc(mat, nrhs, adv)
    return collections.OrderedDict(nrhs=nrhs, alpha=sc["alpha"], b=b, beta=sc["beta"], c=c)


def _keep_ctx(obj):
    cb = obj.callback()
    return dict(ctx=cb.ctx_ptr, _keep=(obj, cb))


for adv in (False, True):
    for nrhs in (1, 3):
        tag = f"{'advanced' if adv else 'simple'}-{nrhs}"
        mat = "rand532x231"

        def _srow(orc, adv=adv, nrhs=nrhs, idx=np.int32):
            n, nc, rp, ci, v = _mat("rand532x231")
            b, c, sc = _bc("rand532x231", nrhs, adv)
            return collections.OrderedDict(nrows=n, ncols=nc, nrhs=nrhs, nnz=int(rp[-1]), row_ptrs=Vec(rp.astype(idx)), col_idxs=Vec(ci.astype(idx)),
                                           vals=Vec(v), b=b, c=c, **sc, strategy=0, max_row_nnz_hint=int(np.max(np.diff(rp))))

        def _srow_state(gk, args, sfx="i32"):
            import torch
            rp = _dev(args["row_ptrs"].a)
            tile = int(gk.csr_srow_tile())
            ns = int(gk.csr_srow_entries(args["nnz"], tile))
            srow = torch.full((ns,), -1, dtype=rp.dtype, device="cuda:0")
            getattr(gk, "csr_make_srow_" + sfx)(torch.cuda.current_stream().cuda_stream, args["nrows"], args["nnz"], rp, tile, srow, ns)
            return dict(srow=srow, srow_tile=tile)
        # short rows: the automatic strategy keeps its bit-exact kernels (include/gkomi.h), with srow the nonzero-split one
        add("csr_spmv_srow_f64_i32", tag, _srow, _csr_ref(adv), column=nrhs == 1, state=_srow_state,
            targets="csr_spmv.hip: the nonzero-split kernel over srow, strided b and c")
        add("csr_spmv_srow_f64_i64", tag, functools.partial(_srow, idx=np.int64), _csr64_ref(adv), column=nrhs == 1,
            state=functools.partial(_srow_state, sfx="i64"), targets="csr_spmv.hip (i64): the nonzero-split kernel over srow")

        def _host_csr_ref(orc, adv=adv):
            _, _, rp, ci, v = _mat("rand532x231")
            inner = _csr_ref(adv)(orc)
            return lambda a: inner(dict(a, nrows=532, row_ptrs=rp, col_idxs=ci, vals=v))

        def _fmt_state(gk, args, fmt="csr"):
            from gkomi import formats
            n, nc, rp, ci, v = _mat("rand532x231")
            if fmt == "csr64":
                return _keep_ctx(formats.Csr64.from_host(gk, n, nc, rp.astype(np.int64), ci.astype(np.int64), v))
            A = formats.Csr.from_host(gk, n, nc, rp, ci, v)
            return _keep_ctx(A if fmt == "csr" else A.to(fmt, kind=0, num_columns=1) if fmt == "hybrid" else A.to(fmt))
        for fmt in ("csr", "csr64", "ell", "sellp", "coo", "hybrid"):
            atomics = fmt in ("coo", "hybrid")
            add(f"{fmt}_matrix_apply_cb", tag, functools.partial(_apply_args, mat, nrhs, adv), _host_csr_ref, column=nrhs == 1,
                state=functools.partial(_fmt_state, fmt=fmt), tol={"c": 1e-14, "_order": True} if atomics else None,
                targets=f"precond.hip: forwards b_stride and c_stride to {fmt}'s SpMV")

        def _fbcb(orc, adv=adv, nrhs=nrhs):
            nbrows, nbcols, rp, ci, vals = _fbcsr(3)
            rng = _seed("fbcb", nrhs)
            return collections.OrderedDict(nrhs=nrhs, b=Mat(rng.standard_normal((nbcols * 3, nrhs))),
                                           c=Mat(rng.standard_normal((nbrows * 3, nrhs)) if adv else np.full((nbrows * 3, nrhs), np.nan)), **_ab(adv))

        def _fbcb_state(gk, args):
            from gkomi import formats
            nbrows, nbcols, rp, ci, vals = _fbcsr(3)
            return _keep_ctx(formats.Fbcsr.from_host(gk, nbrows, nbcols, 3, rp, ci, vals))
        add("fbcsr_matrix_apply_cb", tag, _fbcb, _fb_ref(3, adv), column=nrhs == 1, state=_fbcb_state,
            targets="fbcsr.hip: forwards b_stride and c_stride")

        def _dcb(orc, adv=adv, nrhs=nrhs):
            import dense_gemm_util as du
            a, b, c0 = du.operands(40, nrhs, 30, [40, nrhs, 30, 2], period=None)
            return collections.OrderedDict(nrhs=nrhs, b=Mat(b), c=Mat(c0 if adv else np.full((40, nrhs), np.nan)),
                                           alpha=Vec(np.array([2.5])) if adv else None, beta=Vec(np.array([-1.0])) if adv else None)

        def _dcb_state(gk, args, nrhs=nrhs):
            import dense_gemm_util as du
            from gkomi import formats
            a = du.operands(40, nrhs, 30, [40, nrhs, 30, 2], period=None)[0]
            return _keep_ctx(formats.Dense.from_host(gk, a))      # mode 1: the ordered kernels

        def _dcb_ref(orc, adv=adv, nrhs=nrhs):
            import dense_gemm_util as du
            a = du.operands(40, nrhs, 30, [40, nrhs, 30, 2], period=None)[0]

            def kernel(x):
                b, c = live2d(x, "b", 30, nrhs), live2d(x, "c", 40, nrhs)
                c[...] = du.ordered(a, b, c.copy(), 2.5 if adv else None, -1.0 if adv else None)
            return kernel
        add("dense_matrix_apply_cb", tag, _dcb, _dcb_ref, column=nrhs == 1, state=_dcb_state, targets="dense_gemm.hip: forwards b_stride and c_stride")

    # the column-partitioned copy: one column per call; partial sums per column block -> tolerance (test_csr_colpart_gpu)
    @functools.lru_cache(maxsize=None)
    def _cp_mat():
        n = 4000
        rng = np.random.default_rng(3)
        return (n, n) + tuple(matgen.random_rows_csr(n, n, rng.integers(4, 20, size=n), 4))

    def _cp(orc, adv=adv, cb=False):
        n, nc, rp, ci, v = _cp_mat()
        rng = _seed("colpart")
        args = collections.OrderedDict(b=Mat(rng.standard_normal((nc, 1))), c=Mat(rng.standard_normal((n, 1)) if adv else np.full((n, 1), np.nan)), **_ab(adv))
        if cb:
            args["nrhs"] = 1
        return args

    def _cp_state(gk, args, cb=False):
        from gkomi import formats
        n, nc, rp, ci, v = _cp_mat()
        M = formats.Csr.from_host(gk, n, nc, rp, ci, v, strategy=formats.Csr.CSR_STRATEGIES["csrp"])
        assert M.colpart(2) is not None
        return {"ctx" if cb else "h": M._colpart[0], "_keep": M}

    def _cp_ref(orc, adv=adv):
        n, nc, rp, ci, v = _cp_mat()
        inner = _csr_ref(adv)(orc)
        return lambda a: inner(dict(a, nrows=n, nrhs=1, row_ptrs=rp, col_idxs=ci, vals=v))
    tag = "advanced" if adv else "simple"
    add("csr_colpart_spmv_f64", tag, _cp, _cp_ref, column=True, state=_cp_state, tol={"c": 1e-14, "_order": True},
        targets="csr_colpart.hip: b_stride and c_stride of the single column")
    add("csr_colpart_matrix_apply_cb", tag, functools.partial(_cp, cb=True), _cp_ref, column=True, state=functools.partial(_cp_state, cb=True),
        tol={"c": 1e-14, "_order": True}, targets="csr_colpart.hip: forwards b_stride and c_stride, one call per column")


# ---- distributed: Vector::read_distributed's local block -----------------------------------------------------------------------
for ncols in (1, 3):
    def _dist(orc, ncols=ncols):
        bounds = np.array([0, 10, 25, 40], np.int64)
        ids = np.array([0, 1, 0], np.int32)
        starts, sizes = np.zeros(3, np.int32), np.zeros(2, np.int32)
        orc.ref_partition_build_starting_indices(bounds, ids, 3, 2, starts, sizes)
        rng = _seed("dist", ncols)
        rows = np.repeat(np.arange(40, dtype=np.int64), ncols)
        cols = np.tile(np.arange(ncols, dtype=np.int64), 40)
        return collections.OrderedDict(nnz=len(rows), rows=Vec(rows), cols=Vec(cols), vals=Vec(rng.standard_normal(len(rows))), range_bounds=Vec(bounds),
                                       part_ids=Vec(ids), starts=Vec(starts), num_ranges=3, local_part=0, local=Mat(np.zeros((int(sizes[0]), ncols))))
    add("dist_vector_build_local_f64", f"ncols{ncols}", _dist, _by_name("ref_dist_vector_build_local", {"bounds": "range_bounds", "stride": "local_stride"}),
        column=ncols == 1, targets="distributed.hip: local_stride > ncols, offset base")
