"""ilu_factorization::compute_lu and ic_factorization::compute in plain Python, loop for loop as the reference
executor writes them (reference/factorization/ilu_kernels.cpp:56-97, ic_kernels.cpp:53-100), and the generate
chains around them (core/factorization/ilu.cpp:67-124, ic.cpp:67-120): Python floats (IEEE double, one rounding
per operation), bisect for std::lower_bound, math.sqrt.  The yardstick of tests/test_ilu_exact_gpu.py, with the
matrices both test files share."""
import math
from bisect import bisect_left

import numpy as np


def _lists(m):
    rp, ci, v = m
    return [int(x) for x in rp], [int(x) for x in ci], [float(x) for x in v]


def _arrays(rp, ci, v):
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(v, np.float64)


def _div(a, b):
    """IEEE quotient; Python raises where C++ gives inf / nan"""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(a):
    return math.sqrt(a) if a >= 0.0 else math.nan if a == a else a


def compute_lu(m):
    """in place on a copy of the values; rows sorted, diagonal stored (the reference asserts neither)"""
    row_ptrs, col_idxs, values = _lists(m)
    n = len(row_ptrs) - 1
    diagonals = [-1] * n
    for row in range(n):
        begin, end = row_ptrs[row], row_ptrs[row + 1]
        for nz in range(begin, end):
            col = col_idxs[nz]
            if col == row:
                diagonals[row] = nz
            value = values[nz]
            for l_nz in range(begin, end):
                l_col = col_idxs[l_nz]
                if l_col >= min(row, col):
                    continue
                u_begin, u_end = row_ptrs[l_col], row_ptrs[l_col + 1]
                u_nz = bisect_left(col_idxs, col, u_begin, u_end)
                if u_nz != u_end and col_idxs[u_nz] == col:
                    value -= values[l_nz] * values[u_nz]
            if row <= col:
                values[nz] = value
            else:
                assert diagonals[col] != -1
                values[nz] = _div(value, values[diagonals[col]])
    return _arrays(row_ptrs, col_idxs, values)


def ic_compute(m):
    row_ptrs, col_idxs, values = _lists(m)
    n = len(row_ptrs) - 1
    diagonals = [-1] * n
    for row in range(n):
        begin, end = row_ptrs[row], row_ptrs[row + 1]
        for nz in range(begin, end):
            col = col_idxs[nz]
            if col == row:
                diagonals[row] = nz
            if col > row:
                continue
            total = 0.0
            l_idx, l_end = begin, end
            lh_idx, lh_end = row_ptrs[col], row_ptrs[col + 1]
            while l_idx < l_end and lh_idx < lh_end:
                l_col, lh_row = col_idxs[l_idx], col_idxs[lh_idx]
                if max(l_col, lh_row) > row:
                    break
                if l_col == lh_row and l_col < col:
                    total += values[l_idx] * values[lh_idx]
                l_idx += 1 if l_col <= lh_row else 0
                lh_idx += 1 if lh_row <= l_col else 0
            if row == col:
                values[nz] = _sqrt(values[nz] - total)
            else:
                assert diagonals[col] != -1
                values[nz] = _div(values[nz] - total, values[diagonals[col]])
    return _arrays(row_ptrs, col_idxs, values)


def sort_by_column_index(m):
    rp, ci, v = _lists(m)
    for row in range(len(rp) - 1):
        b, e = rp[row], rp[row + 1]
        order = sorted(range(b, e), key=lambda z: ci[z])   # stable, like the reference's sort of (col, value) pairs
        ci[b:e], v[b:e] = [ci[z] for z in order], [v[z] for z in order]
    return _arrays(rp, ci, v)


def add_diagonal_elements(m):
    """factorization::add_diagonal_elements (reference/factorization/factorization_kernels.cpp): an explicit zero
    where a row of the square matrix stores no diagonal, rows sorted"""
    rp, ci, v = _lists(m)
    nrp, nci, nv = [0], [], []
    for row in range(len(rp) - 1):
        cols = ci[rp[row]:rp[row + 1]]
        vals = v[rp[row]:rp[row + 1]]
        if row not in cols:
            at = bisect_left(cols, row)
            cols.insert(at, row)
            vals.insert(at, 0.0)
        nci += cols
        nv += vals
        nrp.append(len(nci))
    return _arrays(nrp, nci, nv)


def initialize_l_u(m):
    """L: the strictly lower part with a unit diagonal; U: the diagonal and the upper part"""
    rp, ci, v = _lists(m)
    lrp, lci, lv, urp, uci, uv = [0], [], [], [0], [], []
    for row in range(len(rp) - 1):
        diag = 1.0
        for z in range(rp[row], rp[row + 1]):
            if ci[z] < row:
                lci.append(ci[z]); lv.append(v[z])
            elif ci[z] == row:
                diag = v[z]
        lci.append(row); lv.append(1.0)
        uci.append(row); uv.append(diag)
        for z in range(rp[row], rp[row + 1]):
            if ci[z] > row:
                uci.append(ci[z]); uv.append(v[z])
        lrp.append(len(lci)); urp.append(len(uci))
    return _arrays(lrp, lci, lv), _arrays(urp, uci, uv)


def initialize_l(m):
    """L: the lower part with the diagonal as stored (diag_sqrt = false)"""
    rp, ci, v = _lists(m)
    lrp, lci, lv = [0], [], []
    for row in range(len(rp) - 1):
        diag = 1.0
        for z in range(rp[row], rp[row + 1]):
            if ci[z] < row:
                lci.append(ci[z]); lv.append(v[z])
            elif ci[z] == row:
                diag = v[z]
        lci.append(row); lv.append(diag)
        lrp.append(len(lci))
    return _arrays(lrp, lci, lv)


def transpose(m):
    rp, ci, v = _lists(m)
    n = len(rp) - 1
    rows = [[] for _ in range(n)]
    for row in range(n):
        for z in range(rp[row], rp[row + 1]):
            rows[ci[z]].append((row, v[z]))
    trp, tci, tv = [0], [], []
    for r in rows:
        tci += [c for c, _ in r]
        tv += [x for _, x in r]
        trp.append(len(tci))
    return _arrays(trp, tci, tv)


def ilu_generate(m, skip_sorting=False):
    """Ilu::generate_l_u -> (L, U)"""
    if not skip_sorting:
        m = sort_by_column_index(m)
    return initialize_l_u(compute_lu(add_diagonal_elements(m)))


def ic_generate(m, skip_sorting=False):
    """Ic::generate with both_factors -> (L, L^T)"""
    if not skip_sorting:
        m = sort_by_column_index(m)
    L = initialize_l(ic_compute(add_diagonal_elements(m)))
    return L, transpose(L)


# ---- matrices --------------------------------------------------------------------------------------

def dense_to_csr(a, keep_zeros=False):
    a = np.asarray(a, np.float64)
    rp, ci, v = [0], [], []
    for row in a:
        for j, x in enumerate(row):
            if keep_zeros or x != 0.0:
                ci.append(j); v.append(float(x))
        rp.append(len(ci))
    return _arrays(rp, ci, v)


def csr_to_dense(m):
    rp, ci, v = m
    n = len(rp) - 1
    a = np.zeros((n, n))
    for row in range(n):
        for z in range(rp[row], rp[row + 1]):
            a[row, ci[z]] = v[z]
    return a


def from_rows(rows):
    """rows: one {col: value} per row"""
    rp, ci, v = [0], [], []
    for r in rows:
        for c in sorted(r):
            ci.append(c); v.append(float(r[c]))
        rp.append(len(ci))
    return _arrays(rp, ci, v)


def to_rows(m):
    rp, ci, v = m
    return [{int(ci[z]): float(v[z]) for z in range(rp[r], rp[r + 1])} for r in range(len(rp) - 1)]


def spd_version(m):
    """pattern of A + A^T, off-diagonal values -(|a_ij| + |a_ji|) / 2 scaled into (-1, 0), diagonal = 1 + sum of
    the absolute off-diagonal values of the row: symmetric, strictly diagonally dominant, positive diagonal"""
    rows = to_rows(m)
    n = len(rows)
    scale = max([abs(x) for r in rows for x in r.values() if x == x and abs(x) != math.inf] + [1.0])
    out = [dict() for _ in range(n)]
    for i, r in enumerate(rows):
        for j, x in r.items():
            if i == j:
                continue
            x = abs(x) / scale if x == x and abs(x) != math.inf else 0.5
            w = -(0.25 + 0.5 * x)
            out[i][j] = out[i].get(j, 0.0) + w
            out[j][i] = out[j].get(i, 0.0) + w
    for i in range(n):
        out[i][i] = 1.0 + sum(abs(x) for x in out[i].values())
    return from_rows(out)


def tridiagonal(n, lower=-1.0, diag=2.5, upper=-1.25):
    return from_rows([{j: (diag + 0.001 * i if j == i else lower if j < i else upper)
                       for j in (i - 1, i, i + 1) if 0 <= j < n} for i in range(n)])


def diagonal_blocks_2x2(nblocks):
    rows = []
    for b in range(nblocks):
        i = 2 * b
        rows.append({i: 4.0 + (b % 7), i + 1: 1.0 + 0.125 * (b % 5)})
        rows.append({i: -2.0 + 0.25 * (b % 3), i + 1: 3.0 + (b % 11)})
    return from_rows(rows)


def dense_matrix(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, (n, n))
    a += np.diag(np.abs(a).sum(axis=1) + 1.0)
    return dense_to_csr(a, keep_zeros=True)


def arrow(n, seed=3):
    rng = np.random.default_rng(seed)
    rows = [{i: 4.0 + float(rng.uniform()), n - 1: float(rng.uniform(-1, 1))} for i in range(n - 1)]
    last = {j: float(rng.uniform(-1, 1)) for j in range(n - 1)}
    last[n - 1] = float(n)
    return from_rows(rows + [last])


def random_dominant(n, min_len, max_len, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        length = int(rng.integers(min_len, max_len + 1))
        cols = set(int(c) for c in rng.choice(n, size=min(length, n), replace=False)) if length > 1 else set()
        cols.discard(i)
        r = {c: float(rng.uniform(-1, 1)) for c in sorted(cols)[:max(length - 1, 0)]}
        r[i] = 1.0 + sum(abs(x) for x in r.values())
        rows.append(r)
    return from_rows(rows)


def wide_then_narrow(wide_rows, chain, long_row):
    """`wide_rows` independent rows (one level), then a chain of `chain` rows each hanging on its predecessor and on
    row 0 (narrow levels), then one row of `long_row` entries over the leading rows"""
    n = wide_rows + chain + 1
    rows = [{i: 2.0 + 0.01 * (i % 13)} for i in range(wide_rows)]
    for c in range(chain):
        i = wide_rows + c
        rows.append({0: 0.5, i - 1: -0.75, i: 3.0 + 0.1 * (c % 5)})
    last = {j: 0.001 * ((j % 17) - 8) for j in range(long_row - 1)}
    last[n - 1] = 5.0
    rows.append(last)
    for j in last:          # give the long row's columns an entry in the last column: U has fill candidates
        if j < n - 1 and j % 3 == 0:
            rows[j][n - 1] = 0.25
    return from_rows(rows)


def level_widths(widths):
    """rows in level order, widths[l] rows in level l: a row of level l stores one row of level l - 1 and, from
    level 2 on, one of level l - 2 (so the row it hangs on has something to eliminate), its diagonal and two
    entries to the right"""
    first = [0]
    for w in widths:
        first.append(first[-1] + w)
    n = first[-1]
    rows = []
    for lvl, w in enumerate(widths):
        for r in range(w):
            i = first[lvl] + r
            row = {i: 4.0 + 0.03125 * (i % 9)}
            if lvl >= 1:
                row[first[lvl - 1] + r % widths[lvl - 1]] = -1.0 - 0.0625 * (r % 5)
            if lvl >= 2:
                row[first[lvl - 2] + r % widths[lvl - 2]] = 0.5 + 0.125 * (r % 3)
            for off in (widths[lvl] + 1, 2 * widths[lvl] + 3):
                if i + off < n:
                    row[i + off] = 0.25 - 0.015625 * ((i + off) % 7)
            rows.append(row)
    return from_rows(rows)


def wide_level_with_long_rows(n, wide, long_rows):
    """three leading rows with every second column to their right; then `wide` rows of one level that store
    those three, their diagonal and a few entries to the right -- row 3 + 2 k stores long_rows[k] entries to its
    right instead; the remaining rows are diagonal"""
    rows = [{j: (5.0 + i if j == i else 0.001 * ((i + j) % 11 - 5)) for j in range(i, n) if j == i or j % 2 == 0}
            for i in range(3)]
    for r in range(wide):
        i = 3 + r
        row = {0: 0.5, 1: -0.25 + 0.01 * r, 2: 0.125, i: 6.0 + 0.1 * r}
        extra = long_rows[r // 2] if r % 2 == 0 and r // 2 < len(long_rows) else 5
        step = max((n - i - 1) // extra, 1)
        for j in list(range(i + 1, n, step))[:extra]:
            row[j] = 0.002 * ((i * j) % 13 - 6)
        rows.append(row)
    rows += [{i: 2.0 + 0.001 * i} for i in range(3 + wide, n)]
    return from_rows(rows)


def bits_equal(a, b):
    """int64 views equal, NaNs equal by position"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb])
