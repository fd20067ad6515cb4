"""The two ParICT kernels and ParIct::generate in plain Python, loop for loop as the reference executor writes them
(reference/factorization/par_ict_kernels.cpp:65-199, core/factorization/par_ict.cpp:174-292): Python floats (IEEE
double, one rounding per operation), math.sqrt, bisect for std::lower_bound.  Selection, filter, spgemm and transpose
are those of par_ilut_util / spgemm_util.  The yardstick of tests/test_par_ict_gpu.py and, pinned itself to the
reference's known answers and to results recorded from the reference executor, of tests/test_par_ict_reference.py."""
from bisect import bisect_left

import ilu_exact_util as xu
import par_ilut_util as pu
import spgemm_util as su
from ilu_exact_util import _arrays, _div, _lists, _sqrt
from par_ilut_util import _finite

SENTINEL = su.SENTINEL


def initialize_l(m, diag_sqrt):
    """factorization::initialize_l (reference/factorization/factorization_kernels.cpp:278-318)"""
    rp, ci, v = _lists(xu.initialize_l(m))
    if diag_sqrt:
        for row in range(len(rp) - 1):
            d = _sqrt(v[rp[row + 1] - 1])
            v[rp[row + 1] - 1] = d if _finite(d) else 1.0
    return _arrays(rp, ci, v)


def compute_factor(a, l, rejected=None):
    """:65-121: one sequential sweep, in place on a copy -> L.  rejected: a list that receives the (row, col) of every
    value that was not finite and left the old one in place"""
    arp, aci, av = _lists(a)
    lrp, lci, lv = _lists(l)
    for row in range(len(arp) - 1):
        for l_nz in range(lrp[row], lrp[row + 1]):
            col = lci[l_nz]
            a_begin, a_end = arp[row], arp[row + 1]
            a_nz = bisect_left(aci, col, a_begin, a_end)
            has_a = a_nz < a_end and aci[a_nz] == col
            a_val = av[a_nz] if has_a else 0.0
            total = 0.0
            l_begin, l_end = lrp[row], lrp[row + 1]
            lh_begin, lh_end = lrp[col], lrp[col + 1]
            while l_begin < l_end and lh_begin < lh_end:
                l_col, lh_row = lci[l_begin], lci[lh_begin]
                if l_col == lh_row and l_col < col:
                    total += lv[l_begin] * lv[lh_begin]
                l_begin += l_col <= lh_row
                lh_begin += lh_row <= l_col
            new_val = a_val - total
            if row == col:
                new_val = _sqrt(new_val)
            else:
                new_val = _div(new_val, lv[lrp[col + 1] - 1])
            if _finite(new_val):
                lv[l_nz] = new_val
            elif rejected is not None:
                rejected.append((row, col))
    return _arrays(lrp, lci, lv)


def add_candidates(llh, a, l):
    """:127-199 over abstract_spgeam(a, llh) -> L_new"""
    arp, aci, av = _lists(a)
    brp, bci, bv = _lists(llh)
    lrp, lci, lv = _lists(l)
    nrp, nci, nv = [0], [], []
    for row in range(len(arp) - 1):
        a_begin, a_end = arp[row], arp[row + 1]
        b_begin, b_end = brp[row], brp[row + 1]
        l_old_begin, l_old_end = lrp[row], lrp[row + 1]
        total_size = (a_end - a_begin) + (b_end - b_begin)
        skip = False
        for _ in range(total_size):
            if skip:
                skip = False
                continue
            a_col = su._checked_load(aci, a_begin, a_end, SENTINEL)
            b_col = su._checked_load(bci, b_begin, b_end, SENTINEL)
            a_val = su._checked_load(av, a_begin, a_end, 0.0)
            b_val = su._checked_load(bv, b_begin, b_end, 0.0)
            col = min(a_col, b_col)
            r_val = (a_val if a_col == col else 0.0) - (b_val if b_col == col else 0.0)
            l_col = su._checked_load(lci, l_old_begin, l_old_end, SENTINEL)
            l_val = su._checked_load(lv, l_old_begin, l_old_end, 0.0)
            if row >= col:
                diag = lv[lrp[col + 1] - 1]
                nci.append(col)
                nv.append(l_val if l_col == col else _div(r_val, diag))
            l_old_begin += l_col == col
            a_begin += a_col <= b_col
            b_begin += b_col <= a_col
            skip = a_col == b_col
        nrp.append(len(nci))
    return _arrays(nrp, nci, nv)


def transpose(m):
    return pu.transpose(m)


def iterate(a, l, lh, l_nnz_limit, use_approx_select, trace=None):
    """ParIctState::iterate (core/factorization/par_ict.cpp:228-292) -> (L, L^H); trace: a dict that receives the
    intermediate matrices, the threshold and the entries each sweep rejected"""
    llh = su.spgemm(l, lh)
    l_cand = add_candidates(llh, a, l)
    rejected_first, rejected_second = [], []
    l_new = compute_factor(a, l_cand, rejected_first)
    l_filter_rank = max(0, len(l_new[2]) - l_nnz_limit - 1)
    if use_approx_select:
        l_threshold, l = pu.threshold_filter_approx(l_new, l_filter_rank)
    else:
        l_threshold = pu.threshold_select(l_new, l_filter_rank)
        l = pu.threshold_filter(l_new, l_threshold)
    if trace is not None:
        trace.update(llh=llh, l_cand=l_cand, l_new=l_new, l_rank=l_filter_rank, l_threshold=l_threshold, l_filtered=l,
                     rejected=(rejected_first, rejected_second))
    l = compute_factor(a, l, rejected_second)
    return l, transpose(l)


def generate(m, iterations=5, fill_in_limit=2.0, approximate_select=True, skip_sorting=False, traces=None):
    """ParIct::generate_l_lt (:174-225) -> (L, L^H).  traces: a list that receives one dict per iteration"""
    assert fill_in_limit > 0.0
    if not skip_sorting:
        m = xu.sort_by_column_index(m)
    l = initialize_l(m, True)
    l_nnz_limit = int(len(l[2]) * fill_in_limit)      # static_cast<IndexType>
    lh = transpose(l)
    for _ in range(iterations):
        trace = {} if traces is not None else None
        l, lh = iterate(m, l, lh, l_nnz_limit, approximate_select, trace)
        if traces is not None:
            trace.update(l_nnz=len(l[2]))
            traces.append(trace)
    return l, lh


def dense_to_csr(a):
    """gko::initialize<Csr>: zeros are not stored"""
    return xu.dense_to_csr(a)


# ---- results recorded from the reference executor (ref_driver's verb par_ict -> golden/par_ict_ref.json) -----------

def _ani1_with_some_diagonals_halved():
    """ani1 with the diagonal entry of every fifth row halved: not positive definite any more, so both sweeps of
    every iteration meet roots of negative numbers and keep the old values"""
    rows = xu.to_rows(pu._golden_mtx("ani1.mtx"))
    for i in range(0, len(rows), 5):
        rows[i][i] = 0.5 * rows[i][i]
    return xu.from_rows(rows)


RECORDED_CASES = {
    "1138_bus": pu.RECORDED_CASES["1138_bus"],
    "ani1": pu.RECORDED_CASES["ani1"],
    "ani4": pu.RECORDED_CASES["ani4"],
    "grid_24x20": pu.RECORDED_CASES["grid_24x20"],
    "random_spd_300": lambda: xu.spd_version(xu.random_dominant(300, 2, 9, 11)),
    "ani1_without_some_diagonals": pu.RECORDED_CASES["ani1_without_some_diagonals"],
    "ani1_with_some_diagonals_halved": _ani1_with_some_diagonals_halved,
}
RECORDED_LIMITS = pu.RECORDED_LIMITS

case_arrays = pu.case_arrays


def made_cases():
    return {name: make() for name, make in RECORDED_CASES.items()}


def queue_cases(batch):
    return pu.queue_cases(batch, "par_ict", made_cases())


def group_records(arrays):
    """as par_ilut_util.group_records; the entry counts of 1 ... 5 iterations of one configuration as one list"""
    out = pu.group_records(arrays)
    return {k: ([x[0] for x in r] if k.endswith("/nnz") else r) for k, r in out.items()}


def fixture_from(recorded):
    return pu.fixture_from(recorded, "par_ict", made_cases(), group_records)
