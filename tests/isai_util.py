"""The five ISAI kernels and Isai::generate_inverse in plain Python, loop for loop as the reference executor writes
them (reference/preconditioner/isai_kernels.cpp:60-447, core/preconditioner/isai.cpp:87-265): Python floats (IEEE
double, one rounding per operation), math.sqrt.  The triangular excess systems go through the triangular-solve
restatement of lu_util, the general and spd ones through a dense solve per block (the reference's default there is
an iterative solver, so those rows are compared at its tolerance, not bit for bit).  spgemm, transpose, sort and
initialize_l are those of spgemm_util / ilu_exact_util.  The yardstick of tests/test_isai_gpu.py and, pinned itself
to the reference's known answers and to results recorded from the reference executor, of
tests/test_isai_reference.py; with the case generators both use."""
import math
import os

import numpy as np

import ilu_exact_util as xu
import lu_util
import ref_exec
import spgemm_util as su
from ilu_exact_util import _arrays, _div, _lists, _sqrt
from ref_exec import digest

ROW_SIZE_LIMIT = 32          # kernels::isai::row_size_limit (core/preconditioner/isai_kernels.hpp)
KINDS = ("lower", "upper", "general", "spd")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _finite(x):
    return not (math.isinf(x) or math.isnan(x))


def forall_matching(fst, fst_begin, fst_size, snd, snd_begin, snd_size, cb):
    """:60-76"""
    fst_idx = snd_idx = 0
    while fst_idx < fst_size and snd_idx < snd_size:
        fst_val, snd_val = fst[fst_begin + fst_idx], snd[snd_begin + snd_idx]
        if fst_val == snd_val:
            cb(fst_val, fst_idx, snd_idx)
        fst_idx += fst_val <= snd_val
        snd_idx += fst_val >= snd_val


def trs_solve(system, size, lower):
    """:198-232 -> rhs"""
    rhs = [0.0] * size
    if size <= 0:
        return rhs
    rhs[size - 1 if lower else 0] = 1.0
    if lower:
        for col in range(size - 1, -1, -1):
            bot = _div(rhs[col], system[col][col])
            rhs[col] = bot
            for row in range(col - 1, -1, -1):
                rhs[row] -= bot * system[col][row]
    else:
        for col in range(size):
            top = _div(rhs[col], system[col][col])
            rhs[col] = top
            for row in range(col + 1, size):
                rhs[row] -= top * system[col][row]
    return rhs


def general_solve(ts, size, rhs_one_idx, spd):
    """:275-327 on the transposed system ts (a list of rows, changed in place) -> rhs"""
    rhs = [0.0] * size
    if size <= 0:
        return rhs
    rhs[rhs_one_idx] = 1.0
    for col in range(size):
        cp = 0                                           # choose_pivot :243-253 on column col from row col on
        for i in range(1, size - col):
            if abs(ts[col + cp][col]) < abs(ts[col + i][col]):
                cp = i
        row = cp + col
        ts[col], ts[row] = ts[row], ts[col]
        rhs[row], rhs[col] = rhs[col], rhs[row]
        d = ts[col][col]
        for i in range(size):
            ts[i][col] = _div(ts[i][col], -d)
        ts[col][col] = 0.0
        rhs_key_val = rhs[col]
        for i in range(size):
            scal = ts[i][col]
            for j in range(size):
                ts[i][j] += scal * ts[col][j]
            rhs[i] += rhs_key_val * scal
        for j in range(size):
            ts[col][j] = _div(ts[col][j], d)
        rhs[col] = _div(rhs[col], d)
        ts[col][col] = _div(1.0, d)
    if spd:
        scal = _div(1.0, _sqrt(rhs[size - 1]))
        for row in range(size):
            rhs[row] *= scal
    return rhs


def generic_generate(m, inverse, kind):
    """:80-188 -> (inverse with the values of its short rows, excess_rhs_ptrs, excess_nz_ptrs)"""
    assert kind in KINDS
    tri = kind in ("lower", "upper")
    mrp, mci, mv = _lists(m)
    irp, ici, iv = _lists(inverse)
    n = len(mrp) - 1
    excess_rhs_ptrs, excess_nz_ptrs = [0] * (n + 1), [0] * (n + 1)
    excess_rhs_begin = excess_nz_begin = 0
    for row in range(n):
        i_begin, i_size = irp[row], irp[row + 1] - irp[row]
        excess_rhs_ptrs[row], excess_nz_ptrs[row] = excess_rhs_begin, excess_nz_begin
        if i_size <= ROW_SIZE_LIMIT:
            system = [[0.0] * i_size for _ in range(i_size)]
            one_idx = [0]
            for i in range(i_size):
                col = ici[i_begin + i]
                m_begin, m_size = mrp[col], mrp[col + 1] - mrp[col]

                def cb(_, m_idx, i_idx):
                    if mci[m_idx + m_begin] < row and col == row:
                        one_idx[0] += 1
                    if tri:
                        system[i][i_idx] = mv[m_idx + m_begin]
                    else:
                        system[i_idx][i] = mv[m_idx + m_begin]
                forall_matching(mci, m_begin, m_size, ici, i_begin, i_size, cb)
            rhs = trs_solve(system, i_size, kind == "lower") if tri else general_solve(system, i_size, one_idx[0], kind == "spd")
            for i in range(i_size):
                idx = i_begin + i
                iv[idx] = rhs[i] if _finite(rhs[i]) else (1.0 if ici[idx] == row else 0.0)
        else:
            for i in range(i_size):
                col = ici[i_begin + i]
                count = [0]
                forall_matching(mci, mrp[col], mrp[col + 1] - mrp[col], ici, i_begin, i_size,
                                lambda *_: count.__setitem__(0, count[0] + 1))
                excess_nz_begin += count[0]
                excess_rhs_begin += 1
    excess_rhs_ptrs[n], excess_nz_ptrs[n] = excess_rhs_begin, excess_nz_begin
    return _arrays(irp, ici, iv), np.array(excess_rhs_ptrs, np.int32), np.array(excess_nz_ptrs, np.int32)


def generate_excess_system(m, inverse, excess_rhs_ptrs, excess_nz_ptrs, e_start, e_end):
    """:338-394 -> (excess system as CSR, excess rhs)"""
    mrp, mci, mv = _lists(m)
    irp, ici, _ = _lists(inverse)
    e_dim = int(excess_rhs_ptrs[e_end] - excess_rhs_ptrs[e_start])
    e_nnz = int(excess_nz_ptrs[e_end] - excess_nz_ptrs[e_start])
    e_row_ptrs, e_cols, e_vals, e_rhs = [0] * (e_dim + 1), [0] * e_nnz, [0.0] * e_nnz, [0.0] * e_dim
    for row in range(e_start, e_end):
        i_begin, i_size = irp[row], irp[row + 1] - irp[row]
        e_begin = int(excess_rhs_ptrs[row] - excess_rhs_ptrs[e_start])
        e_nz = [int(excess_nz_ptrs[row] - excess_nz_ptrs[e_start])]
        if i_size > ROW_SIZE_LIMIT:
            for i in range(i_size):
                e_row = e_begin + i
                col = ici[i_begin + i]
                m_begin = mrp[col]
                e_row_ptrs[e_row] = e_nz[0]
                e_rhs[e_row] = 1.0 if row == col else 0.0

                def cb(_, m_idx, i_idx):
                    e_cols[e_nz[0]] = i_idx + e_begin
                    e_vals[e_nz[0]] = mv[m_idx + m_begin]
                    e_nz[0] += 1
                forall_matching(mci, m_begin, mrp[col + 1] - m_begin, ici, i_begin, i_size, cb)
    e_row_ptrs[e_dim] = e_nnz
    return _arrays(e_row_ptrs, e_cols, e_vals), np.array(e_rhs, np.float64)


def scale_excess_solution(excess_block_ptrs, solution, e_start, e_end):
    """:401-422 -> the scaled solution"""
    v = [float(x) for x in solution]
    offset = int(excess_block_ptrs[e_start])
    for row in range(e_start, e_end):
        block_start, block_end = int(excess_block_ptrs[row]) - offset, int(excess_block_ptrs[row + 1]) - offset
        if block_end == block_start:
            continue
        scal = _div(1.0, _sqrt(v[block_end - 1]))
        for i in range(block_start, block_end):
            v[i] *= scal
    return np.array(v, np.float64)


def scatter_excess_solution(excess_block_ptrs, solution, inverse, e_start, e_end):
    """:429-447 -> the inverse with the rows of [e_start, e_end) filled"""
    irp, ici, iv = inverse[0], inverse[1], np.array(inverse[2], np.float64)
    offset = int(excess_block_ptrs[e_start])
    for row in range(e_start, e_end):
        b, e = int(excess_block_ptrs[row]) - offset, int(excess_block_ptrs[row + 1]) - offset
        iv[int(irp[row]):int(irp[row]) + e - b] = solution[b:e]
    return irp, ici, iv


def extend_sparsity(m, power):
    """isai.cpp:87-118: the pattern of m^power by square-and-multiply, through csr::spgemm"""
    assert power >= 1
    if power == 1:
        return tuple(np.array(a) for a in m)
    id_power, acc = m, m
    i = power - 1
    while i > 1:
        if i % 2 != 0:
            acc = su.spgemm(id_power, acc)
            i -= 1
        id_power = su.spgemm(id_power, id_power)
        i //= 2
    return su.spgemm(id_power, acc)


def excess_blocks(excess_rhs_ptrs, excess_limit):
    """the block loop of isai.cpp:191-209 -> [(excess_start, block)] of the non-empty blocks"""
    n = len(excess_rhs_ptrs) - 1
    total = int(excess_rhs_ptrs[n])
    lim = total if excess_limit == 0 else excess_limit
    out = []
    if total > 0:
        block = 0
        while block < n:
            start, offset = block, int(excess_rhs_ptrs[block])
            dim = 0
            while dim < lim and block < n:
                block += 1
                dim = int(excess_rhs_ptrs[block]) - offset
            if dim == 0:
                break
            out.append((start, block))
    return out


def dense_block_solve(system_t, rhs, block_ptrs):
    """the transposed excess system is block diagonal: one dense solve per block (numpy)"""
    a = xu.csr_to_dense(system_t)
    x = np.zeros(len(rhs))
    for b, e in zip(block_ptrs[:-1], block_ptrs[1:]):
        if e > b:
            x[b:e] = np.linalg.solve(a[b:e, b:e], rhs[b:e])
    return x


def generate_inverse(m, kind, sparsity_power=1, excess_limit=0, skip_sorting=False, trace=None):
    """Isai::generate_inverse (isai.cpp:121-265) -> the approximate inverse (for spd: L; the caller transposes).
    trace: a dict that receives the pattern, the prefix arrays, the inverse before the excess rows and the excess
    systems"""
    assert kind in KINDS and sparsity_power >= 1
    to_invert = m if skip_sorting else xu.sort_by_column_index(m)
    n = len(to_invert[0]) - 1
    if kind != "spd":
        inverted = extend_sparsity(to_invert, sparsity_power)
    else:
        base = xu.initialize_l(to_invert)
        inverted = base if sparsity_power == 1 else extend_sparsity(base, sparsity_power)
    inverted, rhs_ptrs, nz_ptrs = generic_generate(to_invert, inverted, kind)
    if trace is not None:
        trace.update(excess_rhs_ptrs=rhs_ptrs, excess_nz_ptrs=nz_ptrs, direct=tuple(np.array(a) for a in inverted), excess=[])
    for start, block in excess_blocks(rhs_ptrs, excess_limit):
        system, rhs = generate_excess_system(to_invert, inverted, rhs_ptrs, nz_ptrs, start, block)
        e_dim = len(rhs)
        system_t = su.transpose(e_dim, e_dim, system)
        if kind == "lower":
            sol = lu_util.upper_trs(system_t, rhs, False)[:, 0]
        elif kind == "upper":
            sol = lu_util.lower_trs(system_t, rhs, False)[:, 0]
        else:
            sol = dense_block_solve(system_t, rhs, [int(x) - int(rhs_ptrs[start]) for x in rhs_ptrs[start:block + 1]])
        if trace is not None:
            trace["excess"].append({"start": start, "end": block, "system": system, "rhs": rhs, "solution": np.array(sol)})
        if kind == "spd":
            sol = scale_excess_solution(rhs_ptrs, sol, start, block)
        inverted = scatter_excess_solution(rhs_ptrs, sol, inverted, start, block)
    return inverted


def row_lengths(m):
    return np.diff(np.asarray(m[0]))


def long_rows(m):
    """(rows over the limit, their excess unknowns)"""
    ln = row_lengths(m)
    return int((ln > ROW_SIZE_LIMIT).sum()), int(ln[ln > ROW_SIZE_LIMIT].sum())


# ---- matrices ----------------------------------------------------------------------------------------------------

def golden_mtx(name, stored_zero=None):
    """a MatrixMarket file of tests/golden as sorted CSR; stored_zero: the value that stands for a stored zero (the
    isai_* files of the reference hold 12345 there, reference/test/preconditioner/isai_kernels.cpp:85-104)"""
    import matgen
    kind, nr, nc, rows, cols, vals = matgen.read_mtx(os.path.join(GOLDEN, name))
    assert kind == "coo" and nr == nc
    vals = np.array(vals, np.float64)
    if stored_zero is not None:
        vals[vals == stored_zero] = 0.0
    return xu.sort_by_column_index(tuple(matgen.coo_to_csr(nr, rows, cols, vals)))


def ilu0_factors(name):
    """(L, U) of the exact ILU(0) of a golden matrix"""
    return xu.ilu_generate(golden_mtx(name))


def ic0_factor(name):
    return xu.ic_generate(golden_mtx(name))[0]


def banded(n, k, lower, seed=5):
    """a triangular factor with exactly min(k, available) entries per row next to the diagonal, diagonal dominant"""
    rng = np.random.RandomState(seed)
    rows = []
    for r in range(n):
        cols = range(max(0, r - k + 1), r + 1) if lower else range(r, min(n, r + k))
        row = {c: float(rng.uniform(-1.0, 1.0)) for c in cols}
        row[r] = float(rng.uniform(2.0, 3.0)) * (1 if r % 3 else -1)
        rows.append(row)
    return xu.from_rows(rows)


def alternating(n, short, long, lower, seed=7, long_if=lambda r: r % 2 == 1):
    """rows of `short` and of `long` entries (where the triangle has room) in turn"""
    rng = np.random.RandomState(seed)
    rows = []
    for r in range(n):
        k = long if long_if(r) else short
        cols = range(max(0, r - k + 1), r + 1) if lower else range(r, min(n, r + k))
        row = {c: float(rng.uniform(-1.0, 1.0)) for c in cols}
        row[r] = float(rng.uniform(2.0, 3.0))
        rows.append(row)
    return xu.from_rows(rows)


def general_banded(n, below, above, seed=9):
    rng = np.random.RandomState(seed)
    rows = []
    for r in range(n):
        row = {c: float(rng.uniform(-1.0, 1.0)) for c in range(max(0, r - below), min(n, r + above + 1))}
        row[r] = float(rng.uniform(4.0, 5.0)) + below + above
        rows.append(row)
    return xu.from_rows(rows)


def spd_banded(n, half, seed=11):
    g = xu.csr_to_dense(general_banded(n, half, half, seed))
    s = 0.5 * (g + g.T)
    rows = [{c: float(s[r, c]) for c in range(max(0, r - half), min(n, r + half + 1))} for r in range(n)]
    return xu.from_rows(rows)


# ---- results recorded from the reference executor (ref_driver's verb isai -> golden/isai_ref.json) -------------------

def _ani1_lower(change):
    rows = xu.to_rows(ilu0_factors("ani1.mtx")[0])
    for i in range(0, len(rows), 5):
        if change == "zero":
            rows[i][i] = 0.0
        else:
            rows[i].pop(i, None)
    return xu.from_rows(rows)


def _cases():
    """name -> (kind, sparsity_power, excess_limit, matrix maker)"""
    c = {}
    for p in (1, 2, 3, 4):
        c[f"ani1_l_p{p}"] = ("lower", p, 0, lambda: ilu0_factors("ani1.mtx")[0])
        c[f"ani1_u_p{p}"] = ("upper", p, 0, lambda: ilu0_factors("ani1.mtx")[1])
    for p in (1, 3):
        c[f"ani4_l_p{p}"] = ("lower", p, 0, lambda: ilu0_factors("ani4.mtx")[0])
        c[f"ani4_u_p{p}"] = ("upper", p, 0, lambda: ilu0_factors("ani4.mtx")[1])
    for lim in (0, 1000):
        c[f"ani4_l_p4_limit{lim}"] = ("lower", 4, lim, lambda: ilu0_factors("ani4.mtx")[0])
        c[f"ani4_u_p4_limit{lim}"] = ("upper", 4, lim, lambda: ilu0_factors("ani4.mtx")[1])
    c["1138_bus_ic_l_p3"] = ("lower", 3, 0, lambda: ic0_factor("1138_bus.mtx"))
    c["1138_bus_ic_lt_p2"] = ("upper", 2, 0, lambda: xu.transpose(ic0_factor("1138_bus.mtx")))
    c["isai_l"] = ("lower", 1, 0, lambda: golden_mtx("isai_l.mtx", 12345.0))
    c["isai_u"] = ("upper", 1, 0, lambda: golden_mtx("isai_u.mtx", 12345.0))
    c["ani1_l_zero_diagonals"] = ("lower", 1, 0, lambda: _ani1_lower("zero"))
    c["ani1_l_missing_diagonals"] = ("lower", 1, 0, lambda: _ani1_lower("missing"))
    for p in (1, 2):
        c[f"ani1_general_p{p}"] = ("general", p, 0, lambda: golden_mtx("ani1.mtx"))
        c[f"ani1_spd_p{p}"] = ("spd", p, 0, lambda: golden_mtx("ani1.mtx"))
    c["1138_bus_spd_p1"] = ("spd", 1, 0, lambda: golden_mtx("1138_bus.mtx"))
    c["isai_a_general"] = ("general", 1, 0, lambda: golden_mtx("isai_a.mtx", 12345.0))
    c["isai_spd_spd"] = ("spd", 1, 0, lambda: golden_mtx("isai_spd.mtx", 12345.0))
    c["ani1_general_p3"] = ("general", 3, 0, lambda: golden_mtx("ani1.mtx"))
    return c


RECORDED_CASES = _cases()
# name -> (rows over the limit, their entries, longest row, blocks of the excess loop): computed on the CPU from the
# patterns of the all-ones powers of the matrices; the driver's counts are what it meets and the tests compare
EXPECTED_COUNTS = {
    "ani4_l_p3": (0, 0, 28, 0), "ani4_u_p3": (0, 0, 25, 0),
    "ani4_l_p4_limit0": (157, 5574, None, 1), "ani4_u_p4_limit0": (51, 1829, None, 1),
    "ani4_u_p4_limit1000": (51, 1829, None, 2),
    "1138_bus_ic_l_p3": (1, 33, 33, 1), "1138_bus_ic_lt_p2": (0, 0, 32, 0),
    "ani1_general_p2": (0, 0, 21, 0), "ani1_general_p3": (1, 36, 36, 1),
}


def made_cases():
    return {name: (kind, power, limit, make()) for name, (kind, power, limit, make) in RECORDED_CASES.items()}


def queue_cases(batch):
    """queues every recorded case on a ref_exec.Batch -> {name: index of its result}"""
    where = {}
    for name, (kind, power, limit, (rp, ci, v)) in made_cases().items():
        arrays, size = ref_exec.csr_arrays(len(rp) - 1, len(rp) - 1, rp, ci, v)
        where[name] = batch.add("isai", arrays, kind=ref_exec.word("isai", kind), sparsity_power=power,
                                excess_limit=limit, **size)
    return where


def case_arrays(results, where):
    """{case: {"<section>/<name>": array or {"row_ptrs", "col_idxs", "vals"}}} from the driver's results"""
    res = {}
    for name, i in where.items():
        rec = res.setdefault(name, {})
        for what, arr in results[i].items():
            if "." in what:
                mat, part = what.split(".")
                rec.setdefault(mat, {})[part] = arr
            else:
                rec[what] = arr
    return res


def fixture_record(rec):
    """what the fixture keeps of one record: the digest and, for an array of at most 40 entries, the items"""
    if isinstance(rec, dict):
        return {"nnz": int(len(rec["vals"])), "sha256": digest(rec)}
    out = {"sha256": digest(rec)}
    if len(rec) <= 40:
        out["items"] = [float(x).hex() for x in rec] if rec.dtype == np.float64 else [int(x) for x in rec]
    return out


def fixture_from(recorded):
    cases = made_cases()
    return {"source": "oracle/ref_driver.cpp, verb isai, over the reference executor (preconditioner::Isai::generate "
                      "and kernels::reference::isai) on RECORDED_CASES of tests/isai_util.py; sha256: see digest() in "
                      "tests/ref_exec.py",
            "cases": {name: {"kind": cases[name][0], "sparsity_power": cases[name][1], "excess_limit": cases[name][2],
                             "n": len(cases[name][3][0]) - 1, "nnz": len(cases[name][3][1]),
                             "records": {k: fixture_record(r) for k, r in sorted(recorded[name].items())}}
                      for name in cases}}
