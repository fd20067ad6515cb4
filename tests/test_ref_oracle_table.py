"""Completeness of the reference-parity tests: every ref_* export of the C
oracle and every public function of the eleven Python restatements is looked
up in the table below.  An entry names the ref_driver verb whose cases pin it
to the reference itself, or says why nothing does -- which only the distributed
family, the cpu_baseline port, pure helpers (functions that compute nothing
the reference computes: generators, packers, comparison helpers) and second
forms may do.  A second form restates the device's way to something the
reference computes in another order; its entry names the pinned function it
is a form of and the CPU test that holds the two equal, or within a stated
bound of each other.

The table is checked mechanically as far as text can be: the verb exists in
oracle/ref_driver.cpp and is used by the parity modules; a pinned name is
called by the parity modules themselves, or -- `via` -- inside the definition
of another pinned function."""
import inspect
import os
import re

import cb_gmres_util
import fbcsr_util
import idr_util
import ilu_exact_util
import isai_util
import lu_util
import multigrid_util
import oracle_lib
import par_ict_util
import par_ilut_util
import pgm_util
import spgemm_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a family pinned through a JSON fixture has a parity module of its own: the restatement against the fixture, the
# fixture against the driver.  Its functions are looked up there, under the name the module imports it by.
OWN = {"par_ilut_util": ("test_par_ilut_reference.py", "pu"), "par_ict_util": ("test_par_ict_reference.py", "iu"),
       "isai_util": ("test_isai_reference.py", "iu"), "cb_gmres_util": ("test_cb_gmres_reference.py", "cu"),
       "multigrid_util": ("test_multigrid_reference.py", "mu"), "pgm_util": ("test_pgm_reference.py", "pu")}
SHARED = ["test_ref_oracle_parity.py", "test_ref_oracle_parity_solvers.py"]
PARITY = SHARED + [f for f, _ in OWN.values()]
# modules through which the parity tests call the oracle
GLUE = ["formats_util.py", "ilu_util.py"]
UTILS = {"fbcsr_util": fbcsr_util, "spgemm_util": spgemm_util, "idr_util": idr_util,
         "ilu_exact_util": ilu_exact_util, "lu_util": lu_util, "par_ilut_util": par_ilut_util,
         "par_ict_util": par_ict_util, "isai_util": isai_util, "cb_gmres_util": cb_gmres_util,
         "multigrid_util": multigrid_util, "pgm_util": pgm_util}


def V(verb, via=None):
    return ("verb", verb, via)


def R(kind, why, of=None, test=None):
    """of, test: the pinned function a second form is a form of, and the test of its parity module that relates them"""
    assert kind in ("distributed", "cpu_baseline", "helper", "second_form") and (kind == "second_form") == (of is not None)
    return ("reason", kind, why, of, test)


DIST = R("distributed", "the reference's distributed classes need MPI; oracle/distributed.c stays on its golden vectors")
ORACLE = {
    # SpMV
    **{n: V("spmv") for n in (
        "ref_csr_spmv", "ref_csr_advanced_spmv", "ref_csr_spmv_f32", "ref_csr_advanced_spmv_f32", "ref_ell_spmv",
        "ref_ell_advanced_spmv", "ref_sellp_spmv", "ref_sellp_advanced_spmv", "ref_coo_spmv", "ref_coo_advanced_spmv",
        "ref_coo_spmv2", "ref_coo_advanced_spmv2")},
    # Dense
    **{n: V("dense") for n in (
        "ref_dense_scale", "ref_dense_inv_scale", "ref_dense_add_scaled", "ref_dense_sub_scaled", "ref_dense_compute_dot",
        "ref_dense_compute_norm2", "ref_dense_compute_norm1", "ref_dense_fill", "ref_dense_copy", "ref_dense_row_gather",
        "ref_dense_scale_f32", "ref_dense_inv_scale_f32", "ref_dense_add_scaled_f32", "ref_dense_sub_scaled_f32",
        "ref_dense_compute_dot_f32", "ref_dense_compute_norm2_f32", "ref_dense_fill_f32", "ref_dense_copy_f32")},
    "ref_dense_compute_squared_norm2": R("distributed", "a kernel only distributed::Vector::compute_norm2 launches; "
                                                        "Dense has no public entry to it"),
    "ref_dense_compute_sqrt": R("distributed", "the second half of distributed::Vector::compute_norm2"),
    # conversions and Csr operations
    **{n: V("convert") for n in (
        "ref_compute_max_row_nnz", "ref_csr_convert_to_ell", "ref_sellp_compute_slice_sets", "ref_csr_convert_to_sellp",
        "ref_hybrid_ell_width", "ref_hybrid_compute_coo_row_ptrs", "ref_csr_convert_to_hybrid",
        "ref_convert_idxs_to_ptrs")},
    "ref_convert_ptrs_to_sizes": V("convert", via="ref_hybrid_ell_width"),
    "ref_prefix_sum_i32": V("convert", via="ref_convert_idxs_to_ptrs"),
    "ref_prefix_sum_i64": V("convert", via="ref_hybrid_compute_coo_row_ptrs"),
    "ref_convert_ptrs_to_idxs": V("factor"),
    **{n: V("csr_op") for n in ("ref_csr_transpose", "ref_csr_sort_by_column_index",
                                "ref_csr_is_sorted_by_column_index", "ref_csr_extract_diagonal")},
    **{n: V("mdata") for n in ("ref_matrix_data_sum_duplicates", "ref_matrix_data_remove_zeros",
                               "ref_matrix_data_sort_row_major")},
    # factorizations and triangular solves
    **{n: V("factor") for n in (
        "ref_add_diagonal_elements", "ref_initialize_row_ptrs_l_u", "ref_initialize_l_u", "ref_initialize_row_ptrs_l",
        "ref_initialize_l", "ref_par_ilu_compute_l_u_factors", "ref_par_ic_init_factor", "ref_par_ic_compute_factor")},
    "ref_lower_trs_solve": V("trs"),
    "ref_upper_trs_solve": V("trs"),
    # Jacobi
    **{n: V("jacobi") for n in (
        "ref_jacobi_find_blocks", "ref_jacobi_storage_scheme", "ref_jacobi_storage_space", "ref_jacobi_generate",
        "ref_jacobi_generate_adaptive", "ref_jacobi_apply", "ref_jacobi_simple_apply", "ref_jacobi_apply_adaptive",
        "ref_jacobi_transpose", "ref_jacobi_invert_diagonal", "ref_jacobi_scalar_apply",
        "ref_jacobi_simple_scalar_apply")},
    "ref_jacobi_round_to_precision": V("jacobi", via="ref_jacobi_generate_adaptive"),
    # stopping criteria
    "ref_residual_norm": V("criterion"),
    "ref_residual_norm_f32": V("criterion"),
    "ref_implicit_residual_norm": V("criterion"),
    "ref_set_all_statuses": V("criterion"),
    # solvers: the whole solve is compared, the step kernels are what it is made of
    **{f"ref_{s}_solve": V("solve") for s in ("cg", "fcg", "bicgstab", "cgs", "bicg", "gmres", "ir")},
    "ref_cg_solve_f32": V("solve"),
    **{f"ref_cg_{k}": V("solve", via="ref_cg_solve") for k in ("initialize", "step_1", "step_2")},
    **{f"ref_cg_{k}_f32": V("solve", via="ref_cg_solve_f32") for k in ("initialize", "step_1", "step_2")},
    **{f"ref_fcg_{k}": V("solve", via="ref_fcg_solve") for k in ("initialize", "step_1", "step_2")},
    **{f"ref_bicgstab_{k}": V("solve", via="ref_bicgstab_solve")
       for k in ("initialize", "step_1", "step_2", "step_3", "finalize")},
    **{f"ref_cgs_{k}": V("solve", via="ref_cgs_solve") for k in ("initialize", "step_1", "step_2", "step_3")},
    **{f"ref_bicg_{k}": V("solve", via="ref_bicg_solve") for k in ("initialize", "step_1", "step_2")},
    **{f"ref_gmres_{k}": V("solve", via="ref_gmres_solve")
       for k in ("initialize", "restart", "hessenberg_qr", "solve_krylov", "multi_axpy")},
    "ref_ir_initialize": V("solve", via="ref_ir_solve"),
    # distributed
    **{n: DIST for n in (
        "ref_partition_build_ranges_from_global_size", "ref_partition_build_from_mapping",
        "ref_partition_build_from_contiguous", "ref_partition_build_starting_indices",
        "ref_partition_has_ordered_parts", "ref_dist_build_local_nonlocal", "ref_dist_vector_build_local")},
}

GEN = lambda what: R("helper", "generator: " + what)
DRIVER_END = R("helper", "packs the cases for ref_driver or its results into the fixture's layout")
PYTHON = {
    "fbcsr_util": {
        "spmv": V("spmv"), "csr_to_fbcsr": V("convert"), "to_csr": V("convert"), "fill_in_dense": V("fbcsr_op"),
        "transpose": V("fbcsr_op"), "is_sorted": V("fbcsr_op"), "sort": V("fbcsr_op"), "extract_diagonal": V("fbcsr_op"),
        "random_block_csr": GEN("a random matrix of blocks"),
    },
    "spgemm_util": {
        "spgemm": V("spgemm"), "spgeam": V("spgemm"), "transpose": V("csr_op"),
        "same": R("helper", "compares two results"), "aggregation_2x2": GEN("a prolongation matrix"),
        "random_rows": GEN("random rows"),
    },
    "idr_util": {
        "solve": V("solve"), "csr_apply": V("solve"),
        **{n: V("solve", via="solve") for n in ("initialize", "step_1", "step_2", "step_3", "compute_omega", "seq_dot",
                                                "stopped")},
        "solve_lower_triangular": V("solve", via="step_1"),
        "update_g_and_u": V("solve", via="step_3"),
        "subspace": GEN("a subspace matrix P for the GPU tests; the parity cases build the reference's own"),
    },
    "ilu_exact_util": {
        "ilu_generate": V("factor"), "ic_generate": V("factor"), "sort_by_column_index": V("factor"),
        "transpose": V("csr_op"),
        **{n: V("factor", via="ilu_generate") for n in ("compute_lu", "add_diagonal_elements", "initialize_l_u")},
        **{n: V("factor", via="ic_generate") for n in ("ic_compute", "initialize_l")},
        "bits_equal": R("helper", "compares two results"),
        **{n: GEN("a test matrix") for n in (
            "dense_to_csr", "csr_to_dense", "from_rows", "to_rows", "spd_version", "tridiagonal", "diagonal_blocks_2x2",
            "dense_matrix", "arrow", "random_dominant", "wide_then_narrow", "level_widths",
            "wide_level_with_long_rows")},
    },
    "lu_util": {
        "lu_generate": V("factor"), "direct_apply": V("direct"), "lower_trs": V("trs"), "upper_trs": V("trs"),
        "spmv": V("spmv"),
        "symbolic_cholesky": V("factor", via="lu_generate"),
        **{n: V("factor", via="symbolic_cholesky") for n in ("elimination_forest", "cholesky_symbolic_factorize",
                                                             "merge_patterns")},
        "cholesky_symbolic_count": V("factor"),
        **{n: V("factor", via="lu_generate") for n in ("lu_initialize", "lu_factorize")},
        "read_mtx": R("helper", "reads a MatrixMarket file"), "pattern_rows": R("helper", "repacks a pattern"),
        **{n: GEN("a test matrix") for n in (
            "symmetrize_pattern", "diagonal", "tridiagonal_with_corners", "grid_5pt", "repeated_separable",
            "unsymmetric_values", "with_zero_pivot", "new_values")},
    },
    "par_ilut_util": {
        **{n: V("par_ilut") for n in ("generate", "add_candidates", "compute_l_u_factors", "threshold_select",
                                      "threshold_filter", "threshold_filter_approx", "transpose")},
        "iterate": V("par_ilut", via="generate"), "approx_threshold": V("par_ilut", via="threshold_filter_approx"),
        "dense_to_csr": GEN("a matrix of the reference's tests"), "made_cases": GEN("the recorded matrices"),
        **{n: DRIVER_END for n in ("queue_cases", "case_arrays", "group_records", "fixture_record", "fixture_from")},
    },
    "par_ict_util": {
        **{n: V("par_ict") for n in ("generate", "add_candidates", "compute_factor", "initialize_l")},
        "iterate": V("par_ict", via="generate"), "transpose": V("par_ict", via="iterate"),
        "dense_to_csr": GEN("a matrix of the reference's tests"), "made_cases": GEN("the recorded matrices"),
        **{n: DRIVER_END for n in ("queue_cases", "group_records", "fixture_from")},
    },
    "isai_util": {
        **{n: V("isai") for n in ("generate_inverse", "generic_generate", "generate_excess_system",
                                  "scatter_excess_solution", "row_lengths", "long_rows")},
        **{n: V("isai", via="generate_inverse") for n in ("extend_sparsity", "excess_blocks", "dense_block_solve",
                                                          "scale_excess_solution")},
        **{n: V("isai", via="generic_generate") for n in ("trs_solve", "general_solve", "forall_matching")},
        **{n: GEN("a test matrix") for n in ("golden_mtx", "ilu0_factors", "ic0_factor", "banded", "alternating",
                                             "general_banded", "spd_banded", "made_cases")},
        **{n: DRIVER_END for n in ("queue_cases", "case_arrays", "fixture_record", "fixture_from")},
    },
    "cb_gmres_util": {
        **{n: V("cb_gmres") for n in ("initialize", "restart", "arnoldi", "solve_krylov", "restated_solve",
                                      "float_to_half_bits", "half_bits_to_double")},
        "solve": V("cb_gmres", via="restated_solve"), "jacobi_apply": V("cb_gmres", via="restated_solve"),
        "finish_arnoldi": V("cb_gmres", via="arnoldi"), "givens": V("cb_gmres", via="arnoldi"),
        "correction": V("cb_gmres", via="restart"), "ssum": V("cb_gmres", via="restart"),
        "residual_norm_check": V("cb_gmres", via="solve"),
        "device_sum": R("second_form", "the order in which the device adds", of="ssum",
                        test="test_the_device_s_sum_is_a_reordering_of_the_sequential_one"),
        "reordered_counts": R("second_form", "iteration counts with grouped and device-order sums, rne halves",
                              of="restated_solve",
                              test="test_the_fixture_knows_which_iteration_counts_survive_a_reordered_sum"),
        "compress": R("second_form", "what the device's write of a vector stores (rne halves)", of="float_to_half_bits",
                      test="test_compress_stores_what_a_basis_write_stores"),
        "is_scaled": R("helper", "names the storages with scalars"),
        "count_is_stable": R("helper", "compares the iteration counts of a fixture record"),
        "solve_problem": GEN("the system of a case"), "right_hand_side": GEN("right-hand sides"),
        **{n: DRIVER_END for n in ("queue_cases", "case_arrays", "fixture_from", "dump_fixture")},
    },
    "multigrid_util": {
        **{n: V("multigrid") for n in ("restated_records", "restated", "fixed_coarsening", "spmv", "advanced_spmv",
                                       "preconditioned_cg")},
        **{n: V("multigrid", via="restated_records") for n in ("restated_kcycle", "restated_coarsening",
                                                               "restated_smoother", "restated_solve")},
        **{n: V("multigrid", via="restated_kcycle") for n in ("kcycle_step_1", "kcycle_step_2", "kcycle_check_stop")},
        **{n: V("multigrid", via="fixed_coarsening") for n in ("sort_by_column_index", "transpose", "spgemm")},
        **{n: V("multigrid", via="restated_smoother") for n in ("jacobi_sweeps", "inverted_diagonal")},
        **{n: V("multigrid", via="preconditioned_cg") for n in ("dot", "norm2")},
        **{n: R("helper", "a level factory over fixed_coarsening") for n in ("every_second", "no_reduction")},
        **{n: R("helper", "a call trace against the sequences transcribed from the reference's tests")
           for n in ("cycle_steps", "steps_of", "expected_steps", "steps_match")},
        "csr": R("helper", "packs a matrix"), "record_matches": R("helper", "compares with a fixture record"),
        **{n: GEN("a matrix or the vectors of a case") for n in (
            "read_mtx", "case_matrix", "unsorted_5x5", "shuffled_rows", "right_hand_side", "initial_guess",
            "kcycle_operands")},
        **{n: DRIVER_END for n in ("solve_arguments", "queue_cases", "case_arrays", "fixture_from", "dump_fixture")},
    },
    "pgm_util": {
        **{n: V("pgm") for n in ("generate", "restated", "restated_records", "weight_matrix", "find_strongest_neighbor",
                                 "match_edge", "count_unagg", "assign_to_exist_agg", "renumber", "pgm_level_factory")},
        **{n: V("pgm", via="restated_records") for n in ("level_records", "restated_solve")},
        **{n: V("pgm", via="generate") for n in ("agg_to_restrict", "generate_coarse")},
        **{n: V("pgm", via="weight_matrix") for n in ("compute_absolute", "extract_diagonal", "spgeam")},
        **{n: V("pgm", via="generate_coarse") for n in ("sort_row_major", "compute_coarse_coo")},
        "solve_parts": V("pgm", via="restated_solve"),
        "assign_to_exist_agg_parallel": R("second_form", "the device's static choice followed by pointer jumping",
                                          of="assign_to_exist_agg", test="test_kernel_known_answers"),
        "jump_rounds": R("helper", "counts the rounds of pointer jumping"),
        **{n: R("helper", "the lanes per row the device kernels pick: a condition on the cases")
           for n in ("subwave_width", "case_subwave_width")},
        "record_matches": R("helper", "compares with a fixture record"),
        **{n: GEN("a test matrix") for n in (
            "from_dense_pattern", "reference_5x5", "grid", "grid27", "path", "diagonal", "blocks_2x2", "random_matrix",
            "star_plus_ring", "stencil3", "case_matrix", "solve_matrix")},
        **{n: R("helper", "the cases as text for the mirror's example and its output as arrays")
           for n in ("recorder_input", "parse_example_output", "arrays_from_text")},
        **{n: DRIVER_END for n in ("queue_cases", "fixture_from")},
    },
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _called_in(name, text):
    """`name(` or `.name(` appears; ref_dense_* and the ref_*_solve family are also reached by their f-string spellings"""
    return re.search(r"(?<![\w])" + re.escape(name) + r"\b", text) is not None


def _parity_text():
    return "".join(_read("tests", f) for f in SHARED + GLUE)


def _parity_names():
    """Oracle names the parity modules call, the ones spelled through getattr included."""
    text = _parity_text()
    names = set(re.findall(r"\bref_\w+", text))
    ops = ["scale", "inv_scale", "add_scaled", "sub_scaled", "compute_dot", "compute_norm2", "compute_norm1"]
    assert str(ops).replace("'", '"') in text, "the dense op list of test_ref_oracle_parity.py changed"
    for op in ops + ["fill", "copy"]:
        names |= {f"ref_dense_{op}", f"ref_dense_{op}_f32"}
    names.discard("ref_dense_compute_norm1_f32")
    for s in ("fcg", "bicgstab", "cgs", "bicg"):       # getattr(oracle, f"ref_{solver}_solve")
        names.add(f"ref_{s}_solve")
    names |= {"ref_csr_spmv_f32", "ref_csr_advanced_spmv_f32", "ref_residual_norm_f32"}
    return names


def _driver_verbs():
    return set(re.findall(r'v == "(\w+)"', _read("oracle", "ref_driver.cpp")))


def _c_definition(name):
    """The text of the oracle source file that defines `name`, comments removed."""
    for f in sorted(os.listdir(os.path.join(ROOT, "oracle"))):
        if f.endswith(".c"):
            text = re.sub(r"/\*.*?\*/", "", _read("oracle", f), flags=re.S)
            if re.search(r"ORACLE_API[^;{]*\b" + name + r"\s*\(", text):
                return text
    raise AssertionError(name + " is not defined in oracle/*.c")


def _test_text(text, test):
    """the code of one test function of a module: its docstring and its comments say nothing"""
    m = re.search(r"^def " + re.escape(test) + r"\(.*?(?=^\S|\Z)", text, re.S | re.M)
    if m is None:
        return None
    code = re.sub(r'""".*?"""', "", m.group(0), count=1, flags=re.S)
    return re.sub(r"#[^\n]*", "", code)


def _check_entry(name, entry, direct, via_text, table=None, text="", queues=None):
    """text: the parity module in which a second form's test is looked up; queues: the text that must queue the verb
    on the driver (default: the shared parity modules and their glue)"""
    kind = entry[0]
    if kind == "reason":
        assert entry[1] in ("distributed", "cpu_baseline", "helper", "second_form") and entry[2].strip(), name
        if entry[1] == "second_form":
            _, _, _, of, test = entry
            short = name.split(".")[-1]
            assert table[of][0] == "verb", f"{name}: {of} is not pinned itself"
            body = _test_text(text, test)
            assert body is not None, f"{name}: no test {test} in its parity module"
            assert _called_in(short, body) and _called_in(of, body), f"{name}: {test} does not call it and {of}"
        return
    _, verb, via = entry
    assert verb in _driver_verbs(), f"{name}: ref_driver has no verb {verb}"
    assert f'"{verb}"' in (_parity_text() if queues is None else queues), f"{name}: no parity case uses the verb {verb}"
    if via is None:
        assert direct(name), f"{name}: said to be pinned by {verb}, but no parity module calls it"
    else:
        assert direct(via) or via_text(via) is not None, f"{name}: {via} is not pinned itself"
        assert _called_in(name, via_text(via)), f"{name}: {via} does not call it"


def test_every_oracle_export_is_pinned_or_explained():
    exports = sorted(n for n in oracle_lib._parse() if n.startswith("ref_"))
    missing = [n for n in exports if n not in ORACLE]
    assert not missing, f"oracle exports without a table entry: {missing}"
    stale = [n for n in ORACLE if n not in exports]
    assert not stale, f"table entries for exports that are gone: {stale}"
    called = _parity_names()
    for n in exports:
        if ORACLE[n][0] == "verb" and ORACLE[n][2] is not None:
            assert ORACLE[ORACLE[n][2]][0] == "verb", n
        _check_entry(n, ORACLE[n], lambda x: x in called, _c_definition)
        if ORACLE[n][0] == "reason":
            assert ORACLE[n][1] == "distributed", f"{n}: an oracle export is no pure helper"


def test_every_restatement_function_is_pinned_or_explained():
    for modname, mod in UTILS.items():
        text = _read("tests", OWN[modname][0]) if modname in OWN else _parity_text()
        # a family's own module queues its verb where it calls Batch.add: in its queue_cases
        queues = inspect.getsource(mod.queue_cases) if modname in OWN else None
        if modname in OWN:      # and its parity module runs them through the driver under the one skip rule
            assert OWN[modname][0] in PARITY and "ref_exec.may_skip()" in text and "difference_from_driver(" in text
        public = sorted(n for n, f in vars(mod).items()
                        if inspect.isfunction(f) and f.__module__ == mod.__name__ and not n.startswith("_"))
        table = PYTHON[modname]
        missing = [n for n in public if n not in table]
        assert not missing, f"{modname}: functions without a table entry: {missing}"
        stale = [n for n in table if n not in public]
        assert not stale, f"{modname}: table entries for functions that are gone: {stale}"
        alias = OWN[modname][1] if modname in OWN else {"ilu_exact_util": "xu"}.get(modname, modname)

        def direct(n, alias=alias, text=text):
            return re.search(r"\b" + alias + r"\." + n + r"\b", text) is not None

        def via_text(n, mod=mod):
            return inspect.getsource(getattr(mod, n))

        for n in public:
            entry = table[n]
            if entry[0] == "verb" and entry[2] is not None:
                assert table[entry[2]][0] == "verb", f"{modname}.{n}"
            _check_entry(f"{modname}.{n}" if entry[0] == "reason" else n, entry, direct, via_text, table, text, queues)


def test_no_parity_case_may_skip_where_the_reference_is():
    """A missing driver fails the parity modules wherever the reference or oracle/_ref/ exists."""
    import ref_exec
    if ref_exec.may_skip():
        return
    assert os.path.exists(ref_exec.driver())


def test_the_recorded_results_of_the_gpu_module_are_the_driver_s(oracle):
    """tests/golden/ref_parity_gpu.bin stands in for the driver on a machine without the reference: it must have
    been recorded for the inputs test_ref_parity_gpu.py builds now, and hold what the driver gives for them now.
    (Storage the reference allocates and never writes is left out: the GPU module masks it too.)"""
    import ref_exec
    import test_ref_parity_gpu as gpu
    batch, _ = gpu.REG.queue(oracle)
    recorded = batch.unpack(ref_exec.read_recording(gpu.RECORDING, batch.pack()))
    if ref_exec.may_skip():
        return
    live = batch.run()
    unwritten = {"sellp_ci", "sellp_v", "blocks"}
    for i, (want, got) in enumerate(zip(live, recorded)):
        assert sorted(want) == sorted(got), (i, batch.cases[i][0])
        for k in want:
            if k not in unwritten and k != "error":
                ref_exec.assert_bits(got[k], want[k], f"case {i} ({batch.cases[i][0]}) {k}")
