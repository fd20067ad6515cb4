"""The five ParILUT kernels and ParIlut::generate in plain Python, loop for loop as the reference executor writes them
(reference/factorization/par_ilut_kernels.cpp:73-464, core/factorization/par_ilut.cpp:190-344): Python floats (IEEE
double, one rounding per operation), sorted() for std::sort / std::nth_element (the element of rank r is the same
whatever the algorithm), bisect for std::upper_bound / std::lower_bound.  The yardstick of tests/test_par_ilut_gpu.py
and, pinned itself to the reference's known answers and to results recorded from the reference executor, of
tests/test_par_ilut_reference.py."""
import math
from bisect import bisect_left, bisect_right

import numpy as np

import ilu_exact_util as xu
import ref_exec
import spgemm_util as su
from ilu_exact_util import _arrays, _div, _lists
from ref_exec import digest

SENTINEL = su.SENTINEL
# core/factorization/par_ilut_kernels.hpp:99-100
SEARCHTREE_HEIGHT = 8
OVERSAMPLING = 4
BUCKET_COUNT = 1 << SEARCHTREE_HEIGHT
SAMPLE_SIZE = BUCKET_COUNT * OVERSAMPLING


def _finite(x):
    return x == x and abs(x) != math.inf


def threshold_select(m, rank):
    """:73-90: std::nth_element by magnitude, then abs(*target)"""
    vals = [abs(float(x)) for x in m[2]]
    return sorted(vals)[rank]


def _abstract_filter(m, pred, with_coo):
    """:103-161"""
    rp, ci, v = _lists(m)
    nrp, nci, nv, rows = [0], [], [], []
    for row in range(len(rp) - 1):
        for nz in range(rp[row], rp[row + 1]):
            if pred(row, nz):
                rows.append(row)
                nci.append(ci[nz])
                nv.append(v[nz])
        nrp.append(len(nci))
    out = _arrays(nrp, nci, nv)
    return (out, np.array(rows, np.int32)) if with_coo else out


def threshold_filter(m, threshold, with_coo=False):
    """:170-182: abs(val) >= threshold || col == row (a NaN compares false)"""
    _, ci, v = _lists(m)
    return _abstract_filter(m, lambda row, nz: abs(v[nz]) >= threshold or ci[nz] == row, with_coo)


def approx_threshold(m, rank):
    """the threshold of threshold_filter_approx, :206-247"""
    vals = [float(x) for x in m[2]]
    size = len(vals)
    stride = float(size) / SAMPLE_SIZE
    sample = [abs(vals[int(i * stride)]) for i in range(SAMPLE_SIZE)]      # static_cast<IndexType>: towards zero
    sample.sort()
    splitters = [sample[(i + 1) * OVERSAMPLING] for i in range(BUCKET_COUNT - 1)]
    histogram = [0] * (BUCKET_COUNT + 1)
    for x in vals:
        histogram[bisect_right(splitters, abs(x))] += 1
    total = 0                                                              # components::prefix_sum over bucket_count + 1
    for b in range(BUCKET_COUNT + 1):
        histogram[b], total = total, total + histogram[b]
    threshold_bucket = bisect_right(histogram, rank) - 1                    # distance(histogram + 1, upper_bound(...))
    return splitters[threshold_bucket - 1] if threshold_bucket > 0 else 0.0


def threshold_filter_approx(m, rank, with_coo=False):
    """:198-253 -> (threshold, filtered matrix [, coo rows])"""
    threshold = approx_threshold(m, rank)
    return threshold, threshold_filter(m, threshold, with_coo)


def compute_l_u_factors(a, l, u, u_csc):
    """:264-341: one sequential sweep, in place on copies -> (L, U, U_csc)"""
    arp, aci, av = _lists(a)
    lrp, lci, lv = _lists(l)
    urp, uci, uv = _lists(u)
    utp, utr, utv = _lists(u_csc)

    def compute_sum(row, col):
        a_begin, a_end = arp[row], arp[row + 1]
        a_nz = bisect_left(aci, col, a_begin, a_end)
        has_a = a_nz < a_end and aci[a_nz] == col
        a_val = av[a_nz] if has_a else 0.0
        total = 0.0
        ut_nz = 0
        l_begin, l_end = lrp[row], lrp[row + 1]
        u_begin, u_end = utp[col], utp[col + 1]
        last_entry = min(row, col)
        while l_begin < l_end and u_begin < u_end:
            l_col, u_row = lci[l_begin], utr[u_begin]
            if l_col == u_row and l_col < last_entry:
                total += lv[l_begin] * utv[u_begin]
            if u_row == row:
                ut_nz = u_begin
            l_begin += l_col <= u_row
            u_begin += u_row <= l_col
        return a_val - total, ut_nz

    for row in range(len(arp) - 1):
        for l_nz in range(lrp[row], lrp[row + 1] - 1):
            col = lci[l_nz]
            u_diag = utv[utp[col + 1] - 1]
            new_val = _div(compute_sum(row, col)[0], u_diag)
            if _finite(new_val):
                lv[l_nz] = new_val
        for u_nz in range(urp[row], urp[row + 1]):
            col = uci[u_nz]
            new_val, ut_nz = compute_sum(row, col)
            if _finite(new_val):
                uv[u_nz] = new_val
                utv[ut_nz] = new_val
    return _arrays(lrp, lci, lv), _arrays(urp, uci, uv), _arrays(utp, utr, utv)


def add_candidates(lu, a, l, u):
    """:355-464 over abstract_spgeam(a, lu) -> (L_new, U_new)"""
    arp, aci, av = _lists(a)
    brp, bci, bv = _lists(lu)
    lrp, lci, lv = _lists(l)
    urp, uci, uv = _lists(u)
    nlrp, nlci, nlv, nurp, nuci, nuv = [0], [], [], [0], [], []
    for row in range(len(arp) - 1):
        a_begin, a_end = arp[row], arp[row + 1]
        b_begin, b_end = brp[row], brp[row + 1]
        l_old_begin, l_old_end = lrp[row], lrp[row + 1] - 1      # skip diagonal
        u_old_begin, u_old_end = urp[row], urp[row + 1]
        finished_l = l_old_begin == l_old_end
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
            if finished_l:
                lpu_col = su._checked_load(uci, u_old_begin, u_old_end, SENTINEL)
                lpu_val = su._checked_load(uv, u_old_begin, u_old_end, 0.0)
            else:
                lpu_col, lpu_val = lci[l_old_begin], lv[l_old_begin]
            diag = uv[urp[col]] if col < row else 1.0
            out_val = lpu_val if lpu_col == col else _div(r_val, diag)
            if row >= col:
                nlci.append(col)
                nlv.append(1.0 if row == col else out_val)
            if row <= col:
                nuci.append(col)
                nuv.append(out_val)
            if finished_l:
                u_old_begin += lpu_col == col
            else:
                l_old_begin += lpu_col == col
                finished_l = l_old_begin == l_old_end
            a_begin += a_col <= b_col
            b_begin += b_col <= a_col
            skip = a_col == b_col
        nlrp.append(len(nlci))
        nurp.append(len(nuci))
    return _arrays(nlrp, nlci, nlv), _arrays(nurp, nuci, nuv)


def transpose(m):
    n = len(m[0]) - 1
    return su.transpose(n, n, m)


def iterate(a, l, u, l_nnz_limit, u_nnz_limit, use_approx_select, trace=None):
    """ParIlutState::iterate (core/factorization/par_ilut.cpp:257-344) -> (L, U); trace: a dict that receives the
    intermediate matrices and thresholds"""
    lu = su.spgemm(l, u)
    l_new, u_new = add_candidates(lu, a, l, u)
    u_new_csc = transpose(u_new)
    if trace is not None:
        trace.update(lu=lu, l_cand=l_new, u_cand=u_new)
    l_new, u_new, u_new_csc = compute_l_u_factors(a, l_new, u_new, u_new_csc)
    l_nnz, u_nnz = len(l_new[2]), len(u_new[2])
    l_filter_rank = max(0, l_nnz - l_nnz_limit - 1)
    u_filter_rank = max(0, u_nnz - u_nnz_limit - 1)
    if use_approx_select:
        l_threshold, l = threshold_filter_approx(l_new, l_filter_rank)
        u_threshold, u_csc = threshold_filter_approx(u_new_csc, u_filter_rank)
    else:
        l_threshold = threshold_select(l_new, l_filter_rank)
        u_threshold = threshold_select(u_new_csc, u_filter_rank)
        l = threshold_filter(l_new, l_threshold)
        u_csc = threshold_filter(u_new_csc, u_threshold)
    u = threshold_filter(u_new, u_threshold)
    if trace is not None:
        trace.update(l_new=l_new, u_new=u_new, u_new_csc=u_new_csc, l_rank=l_filter_rank, u_rank=u_filter_rank,
                     l_threshold=l_threshold, u_threshold=u_threshold, l_filtered=l, u_filtered=u)
    l, u, u_csc = compute_l_u_factors(a, l, u, u_csc)
    return l, u


def generate(m, iterations=5, fill_in_limit=2.0, approximate_select=True, skip_sorting=False, traces=None):
    """ParIlut::generate_l_u (:190-253) -> (L, U).  traces: a list that receives one dict per iteration"""
    assert fill_in_limit > 0.0
    if not skip_sorting:
        m = xu.sort_by_column_index(m)
    l, u = xu.initialize_l_u(m)
    l_nnz_limit = int(len(l[2]) * fill_in_limit)      # static_cast<IndexType>
    u_nnz_limit = int(len(u[2]) * fill_in_limit)
    for _ in range(iterations):
        trace = {} if traces is not None else None
        l, u = iterate(m, l, u, l_nnz_limit, u_nnz_limit, approximate_select, trace)
        if traces is not None:
            trace.update(l_nnz=len(l[2]), u_nnz=len(u[2]))
            traces.append(trace)
    return l, u


def dense_to_csr(a):
    """gko::initialize<Csr>: zeros are not stored"""
    return xu.dense_to_csr(a)


# ---- results recorded from the reference executor (ref_driver's verb par_ilut -> golden/par_ilut_ref.json) ---------

def _golden_mtx(name):
    import os
    import matgen
    kind, nr, nc, rows, cols, vals = matgen.read_mtx(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))
    assert kind == "coo" and nr == nc
    return xu.sort_by_column_index(tuple(matgen.coo_to_csr(nr, rows, cols, vals)))


def _without_some_diagonals():
    """ani1 without the diagonal entry of every fifth row"""
    rows = xu.to_rows(_golden_mtx("ani1.mtx"))
    for i in range(0, len(rows), 5):
        rows[i].pop(i, None)
    return xu.from_rows(rows)


def _grid_24x20():
    import matgen
    n, rp, ci, v = matgen.poisson_2d_5pt(20, 24)
    return xu.sort_by_column_index((rp, ci, v))


RECORDED_CASES = {
    "ani1": lambda: _golden_mtx("ani1.mtx"),
    "ani4": lambda: _golden_mtx("ani4.mtx"),
    "1138_bus": lambda: _golden_mtx("1138_bus.mtx"),
    "grid_24x20": _grid_24x20,
    "random_300": lambda: xu.random_dominant(300, 2, 9, 11),
    "ani1_without_some_diagonals": _without_some_diagonals,
}
RECORDED_LIMITS = (0.75, 1.2, 2.0)
FULL_ARRAYS_UP_TO = 64       # rows: the fixture holds whole arrays up to here, SHA-256 digests beyond


def made_cases():
    return {name: make() for name, make in RECORDED_CASES.items()}


def queue_cases(batch, verb="par_ilut", cases=None):
    """queues what the fixture records of every matrix on a ref_exec.Batch: generate for approximate_select 0 / 1,
    fill_in_limit 0.75 / 1.2 / 2.0 and 1 ... 5 iterations, then each kernel alone on the intermediate matrices of
    the first iteration -> [(case, section, index of the result, whether the fixture keeps the factors)]"""
    where = []
    for name, (rp, ci, v) in (made_cases() if cases is None else cases).items():
        arrays, size = ref_exec.csr_arrays(len(rp) - 1, len(rp) - 1, rp, ci, v)
        for select in ("exact", "approx"):
            for limit in RECORDED_LIMITS:
                for iterations in range(1, 6):
                    i = batch.add(verb, arrays, op=0, iterations=iterations, fill_in_limit=limit,
                                  approximate_select=select == "approx", **size)
                    where.append((name, f"generate/{select}/{limit:g}/{iterations}", i, iterations in (1, 5)))
        where.append((name, "kernels", batch.add(verb, arrays, op=1, **size), True))
    return where


def case_arrays(results, where):
    """{case: {"<section>/<array>": numpy array}} from the driver's results: the number of entries of the factors
    of every generate, the factors after 1 and 5 iterations"""
    res = {}
    for name, section, i, factors in where:
        for what, a in results[i].items():
            if factors or what == "nnz":
                res.setdefault(name, {})[f"{section}/{what}"] = a
    return res


def group_records(arrays):
    """the arrays of one case, as case_arrays gives them, grouped: the three arrays of a CSR matrix under
    the matrix' name, the entry counts of 1 ... 5 iterations of one configuration as one list of pairs"""
    out = {}
    for key in sorted(arrays):
        for suffix in (".row_ptrs", ".col_idxs", ".vals"):
            if key.endswith(suffix):
                out.setdefault(key[:-len(suffix)], {})[suffix[1:]] = arrays[key]
                break
        else:
            t = key.split("/")
            if t[0] == "generate" and t[-1] == "nnz":
                out.setdefault("/".join(t[:3]) + "/nnz", []).append([int(x) for x in arrays[key]])
            else:
                out[key] = arrays[key]
    return out


def _items(arr):
    return [float(x).hex() for x in arr] if arr.dtype == np.float64 else [int(x) for x in arr]


def fixture_record(n, key, rec):
    """what the fixture keeps of one record: a list of counts as it is; of an array or matrix the digest and, for a
    short array or a small matrix, the items (values as hexadecimal floats)"""
    if isinstance(rec, list):
        return rec
    # (of the twelve configurations the default one: the whole arrays of all would be megabytes)
    small = n <= FULL_ARRAYS_UP_TO and key.startswith("generate/approx/2/5/")
    if isinstance(rec, dict):
        out = {"nnz": int(len(rec["vals"])), "sha256": digest(rec)}
        if small:
            out["items"] = {k: _items(a) for k, a in rec.items()}
        return out
    out = {"sha256": digest(rec)}
    if len(rec) <= 8 or small:
        out["items"] = _items(rec)
    return out


def fixture_from(recorded, verb="par_ilut", cases=None, group=None):
    cases = made_cases() if cases is None else cases
    group = group or group_records
    klass = {"par_ilut": "ParIlut", "par_ict": "ParIct"}[verb]
    return {"source": f"oracle/ref_driver.cpp, verb {verb}, over the reference executor ({klass}::generate and "
                      f"kernels::reference::{verb}_factorization) on RECORDED_CASES of tests/{verb}_util.py; "
                      "generate/<select>/<fill_in_limit>/<iterations>/<factor>; sha256: see digest() in "
                      "tests/ref_exec.py",
            "cases": {name: {"n": len(cases[name][0]) - 1, "nnz": len(cases[name][1]),
                             "records": {k: fixture_record(len(cases[name][0]) - 1, k, r)
                                         for k, r in group(recorded[name]).items()}}
                      for name in cases}}
