"""Keeps the layout sweep (tests/test_views_gpu.py) complete, and shows on the CPU that its checker
can fail: every function of include/gkomi.h with a `*stride*` parameter is swept, covered by a
named test that already passes unequal padded strides and an offset base, or exempt for one of
two written reasons; and the oracle itself, driven as a wrong kernel in the three ways the sweep
exists for, is rejected."""
import importlib

import numpy as np
import pytest

import view_cases
from gkomi._lib import parse_header
from view_util import LAYOUTS, Prepared, check_case, run_host

# entry point -> (module, test function) that sweeps unequal padded strides AND an offset base
COVERED_BY = {}

# entry point -> (kind, reason); only these two kinds exist
STORAGE, CALLBACK = "storage stride", "apply callback"
EXEMPT = {
    "gkomi_csr_convert_to_ell_f64_i32": (STORAGE, "`stride` is the ELL column stride of the output format"),
    "gkomi_sellp_compute_slice_sets_i32": (STORAGE, "`stride_factor` rounds the slice lengths of SELL-P"),
    "gkomi_csr_convert_to_hybrid_f64_i32": (STORAGE, "`ell_stride` is the column stride of the ELL part"),
}
NEVER_EXEMPT = ("dense_", "cg_", "bicgstab_", "fcg_", "cgs_", "bicg_", "gmres_", "idr_", "multigrid_", "_spmv", "jacobi_",
                "trs_", "gemm", "transpose", "convert_f")


def strided_entry_points():
    return {name for name, (_, params) in parse_header().items() if any("stride" in p[2] for p in params)}


def test_every_strided_entry_point_is_swept_covered_or_exempt():
    want = strided_entry_points()
    assert len(want) >= 96
    swept, covered, exempt = view_cases.registry(), set(COVERED_BY), set(EXEMPT)
    assert not (swept & exempt) and not (covered & exempt)
    missing = sorted(want - swept - covered - exempt)
    assert not missing, f"{len(missing)} strided entry points are in no layout test: {missing}"
    assert not sorted((swept | covered | exempt) - want), "names that the header does not have (any more)"


def test_covering_tests_exist():
    for fn, (module, test) in COVERED_BY.items():
        assert callable(getattr(importlib.import_module(module), test)), (fn, module, test)


def test_exemptions_are_of_the_two_kinds():
    protos = parse_header()
    for fn, (kind, reason) in EXEMPT.items():
        assert kind in (STORAGE, CALLBACK) and reason
        if kind == CALLBACK:
            assert fn.endswith("_matrix_apply_cb")
        else:
            assert "convert_to" in fn or "slice_sets" in fn
            # a storage stride belongs to no dense operand: no pointer parameter right before it
            params = protos[fn][1]
            for i, p in enumerate(params):
                if "stride" in p[2]:
                    assert not params[i - 1][1], (fn, p[2])
        assert not any(tag in fn for tag in NEVER_EXEMPT if not (kind == STORAGE and tag == "_spmv")), fn


def test_every_case_lists_the_control_and_names_its_predicate():
    for c in view_cases.CASES.values():
        assert c.layouts[0] == "L0" and len(c.layouts) >= 5, c.id
        assert c.targets, c.id
    # the layout set of the sweep: padded with both parities, offset, mixed both ways, a column of a wider matrix
    assert {"L0", "L1a", "L1b", "L2", "L3a", "L3b", "L4"} <= set(LAYOUTS)


# ---- the checker must be able to fail ----------------------------------------------------------------------------------
PLANTED = {   # case id -> (two strides to swap, an input whose stride is taken as ncols, the output to smear)
    "cg_step_2_f64-513x3": (("x_stride", "r_stride"), "q", "x"),
    "dense_compute_dot_f64-2051x3": (("x_stride", "y_stride"), "y", "result"),
    "ell_spmv_f64_i32-rand532x231-advanced-3": (("b_stride", "c_stride"), "b", "c"),
}


def honest(case, oracle):
    return lambda c, prep: run_host(c.ref(oracle), c.fn, prep)


@pytest.mark.parametrize("cid", sorted(PLANTED))
def test_the_oracle_passes_its_own_sweep(oracle, cid):
    case = view_cases.CASES[cid]
    cache = {}
    for lname in case.layouts:
        check_case(case, lname, oracle, honest(case, oracle), cache)


@pytest.mark.parametrize("fault", ["strides_swapped", "padding_written", "padding_read"])
@pytest.mark.parametrize("cid", sorted(PLANTED))
def test_planted_faults_are_rejected(oracle, cid, fault):
    case = view_cases.CASES[cid]
    swap, read_as_contiguous, smeared = PLANTED[cid]

    def wrong(c, prep):
        ref = c.ref(oracle)
        if fault == "strides_swapped":
            kernel = lambda a: ref(dict(a, **{swap[0]: a[swap[1]], swap[1]: a[swap[0]]}))
        elif fault == "padding_read":
            ncols = prep.geom[read_as_contiguous][2]
            kernel = lambda a: ref(dict(a, **{read_as_contiguous + "_stride": ncols}))
        else:
            kernel = ref
        bufs = run_host(kernel, c.fn, prep)
        if fault == "padding_written":
            lead, nr, nc, st = prep.geom[smeared]
            first_pad = int(np.flatnonzero(~prep.mask[smeared][lead:])[0]) + lead   # the first element behind a live one
            bufs[smeared][first_pad] = bufs[smeared][lead]
        return bufs
    # the control cannot see a stride fault (all strides equal) -- the padded layouts must
    for lname in ("L1a", "L3a"):
        with pytest.raises(AssertionError):
            check_case(case, lname, oracle, wrong, {})
    if fault == "padding_written":
        with pytest.raises(AssertionError):
            check_case(case, "L2", oracle, wrong, {})


def test_every_reference_is_itself_layout_independent(oracle):
    """every case builds, its reference runs on the host twin with unequal strides and offset bases, leaves the poison
    alone and gives the bits of the contiguous run: the references are fit to judge the kernels"""
    cache = {}
    for case in view_cases.CASES.values():
        if case.ref is not None:
            for lname in ("L3a", case.layouts[-1]):
                check_case(case, lname, oracle, honest(case, oracle), cache)


# ---- every conjunct of every dispatch predicate is true under one layout of its case and false under another ------------------
def layouts_of(cid, oracle):
    """layout name -> {operand: (stride, bytes past a 16-byte boundary, ncols)} of a case, from the buffers the sweep builds"""
    from view_util import parse_layout
    case = view_cases.CASES[cid]
    out = {}
    for lname in case.layouts:
        layout, which = parse_layout(lname)
        prep = Prepared(case.build(oracle), layout, which)
        out[lname] = {k: (st, lead * prep.bufs[k].dtype.itemsize % 16, nc) for k, (lead, nr, nc, st) in prep.geom.items()}
    return out


def contiguous(*names):
    return lambda g: all(g[n][0] == g[n][2] for n in names)


def aligned(name, to=16):
    return lambda g: g[name][1] % to == 0


def even(name):
    return lambda g: g[name][0] % 2 == 0


# predicate (file:line of the launcher) -> (a case of the sweep, its conjuncts over the layout's geometry)
PREDICATES = {
    "dense.hip:92-95 elementwise flat path": ("dense_add_scaled_f64-513x1-a1", [contiguous("x"), contiguous("y"), aligned("x"), aligned("y")]),
    "dense.hip:295-299 reduction flat path": ("dense_compute_dot_f64-2051x1", [contiguous("x"), contiguous("y"), aligned("x"), aligned("y")]),
    "dense.hip:334 fill": ("dense_fill_f64-513x3", [contiguous("x"), aligned("x")]),
    "dense.hip:354-356 copy": ("dense_copy_f64-513x3", [contiguous("in"), contiguous("out"), aligned("in"), aligned("out")]),
    "f32.hip elementwise twin": ("dense_add_scaled_f32-513x1-a1", [contiguous("x"), contiguous("y"), aligned("x"), aligned("y")]),
    "f32.hip reduction twin": ("dense_compute_dot_f32-2051x1", [contiguous("x"), contiguous("y"), aligned("x"), aligned("y")]),
    "mixed.hip:73-75 conversion": ("dense_convert_f64_to_f32-513x1", [contiguous("in"), contiguous("out"), aligned("in"), aligned("out")]),
    "cg.hip:181 cg_step_1": ("cg_step_1_f64-513x1", [contiguous("p"), contiguous("z"), aligned("p"), aligned("z")]),
    "cg.hip:206 cg_step_2": ("cg_step_2_f64-513x1", [contiguous("x", "r", "p", "q"), aligned("x"), aligned("r"), aligned("p"), aligned("q")]),
    "f32.hip cg_step_2 twin": ("cg_step_2_f32-513x1", [contiguous("x", "r", "p", "q"), aligned("x"), aligned("r"), aligned("p"), aligned("q")]),
    "csr_spmv.hip:1123-1125 launch_spmm": ("csr_spmv_f64_i32-rand532x231-simple-8", [aligned("b"), aligned("c"), even("b"), even("c")]),
    "formats.hip:281-282 ELL / SELL-P": ("ell_spmv_f64_i32-rand532x231-simple-15", [aligned("b"), aligned("c"), even("b"), even("c")]),
    "formats.hip:476 COO arrays": ("coo_spmv_f64_i32-rand532x231-simple-3", [aligned("vals"), aligned("row_idxs", 8), aligned("col_idxs", 8)]),
    "coo_spmv.hip:564 COO apply2 -> fallback": ("coo_spmv2_f64_i32-rand532x231-advanced-8", [aligned("vals"), aligned("row_idxs", 8), aligned("col_idxs", 8)]),
    "coo_spmv.hip:564 Hybrid's COO part": ("hybrid_spmv_f64_i32-rand532x231-simple-8", [aligned("coo_vals"), aligned("coo_row_idxs", 8)]),
    "coo_spmv.hip:536 vec2": ("coo_spmv_sorted_f64_i32-rand532x231-simple-15", [aligned("b"), even("b")]),
    "cb_gmres.hip:620 vector_path": ("cb_gmres_finish_arnoldi_f64-keep-64x1", [aligned("next_krylov_basis")]),
}


@pytest.mark.parametrize("name", sorted(PREDICATES))
def test_each_conjunct_is_true_under_one_layout_and_false_under_another(oracle, name):
    cid, conjuncts = PREDICATES[name]
    geoms = layouts_of(cid, oracle)
    assert any(all(c(g) for c in conjuncts) for g in geoms.values()), f"{name}: no layout of {cid} takes the fast path"
    for i, c in enumerate(conjuncts):
        false_alone = [l for l, g in geoms.items() if not c(g) and all(o(g) for o in conjuncts if o is not c)]
        assert false_alone, f"{name}: conjunct {i} is never the only false one in {cid}"
        print(f"{name}: conjunct {i} false alone under {false_alone}")
