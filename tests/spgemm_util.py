"""csr::spgemm, csr::advanced_spgemm and csr::spgeam in plain Python, loop for loop as the reference executor writes
them (reference/matrix/csr_kernels.cpp:146-357, reference/components/csr_spgeam.hpp:58-104): Python floats, one
multiply and one add per term, a dict plus sorted keys for std::map.  The yardstick of tests/test_spgemm_gpu.py."""
import numpy as np

SENTINEL = np.iinfo(np.int32).max   # std::numeric_limits<IndexType>::max()


def _lists(m):
    rp, ci, v = m
    return [int(x) for x in rp], [int(x) for x in ci], [float(x) for x in v]


def _arrays(rp, ci, v):
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(v, np.float64)


def spgemm(a, b, alpha=None, beta=None, d=None):
    """a, b, d: (row_ptrs, col_idxs, values).  alpha is None: csr::spgemm (scale one<ValueType>()), else advanced_spgemm"""
    arp, aci, av = _lists(a)
    brp, bci, bv = _lists(b)
    scale = 1.0 if alpha is None else float(alpha)
    if alpha is not None:
        drp, dci, dv = _lists(d)
        vbeta = float(beta)
    rp, ci, v = [0], [], []
    for row in range(len(arp) - 1):
        cols = {}                                   # map<IndexType, ValueType>: operator[] starts an entry at 0.0
        if alpha is not None:                       # spgemm_accumulate_row(local_row_nzs, d, vbeta, a_row)
            for z in range(drp[row], drp[row + 1]):
                cols[dci[z]] = cols.get(dci[z], 0.0) + vbeta * dv[z]
        for k in range(arp[row], arp[row + 1]):     # spgemm_accumulate_row2
            b_row, a_val = aci[k], av[k]
            for z in range(brp[b_row], brp[b_row + 1]):
                cols[bci[z]] = cols.get(bci[z], 0.0) + scale * a_val * bv[z]
        for col in sorted(cols):
            ci.append(col)
            v.append(cols[col])
        rp.append(len(ci))
    return _arrays(rp, ci, v)


def _checked_load(p, i, size, sentinel):
    """core/base/utils.hpp checked_load"""
    return p[i] if i < size else sentinel


def spgeam(alpha, a, beta, b):
    """abstract_spgeam with the fill callback of csr::spgeam (the count callback sees the same entries)"""
    arp, aci, av = _lists(a)
    brp, bci, bv = _lists(b)
    valpha, vbeta = float(alpha), float(beta)
    rp, ci, v = [0], [], []
    for row in range(len(arp) - 1):
        a_begin, a_end = arp[row], arp[row + 1]
        b_begin, b_end = brp[row], brp[row + 1]
        total_size = (a_end - a_begin) + (b_end - b_begin)
        skip = False
        for _ in range(total_size):
            if skip:
                skip = False
                continue
            a_col = _checked_load(aci, a_begin, a_end, SENTINEL)
            b_col = _checked_load(bci, b_begin, b_end, SENTINEL)
            a_val = _checked_load(av, a_begin, a_end, 0.0)
            b_val = _checked_load(bv, b_begin, b_end, 0.0)
            col = min(a_col, b_col)
            v.append(valpha * (a_val if a_col == col else 0.0) + vbeta * (b_val if b_col == col else 0.0))
            ci.append(col)
            a_begin += a_col <= b_col
            b_begin += b_col <= a_col
            skip = a_col == b_col
        rp.append(len(ci))
    return _arrays(rp, ci, v)


def same(got, want):
    """row_ptrs and col_idxs equal, values equal as 64-bit patterns (signed zeros and NaNs included)"""
    g = [np.asarray(x) for x in got]
    w = [np.asarray(x) for x in want]
    return (np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and g[2].shape == w[2].shape and
            np.array_equal(g[2].astype(np.float64).view(np.uint64), w[2].astype(np.float64).view(np.uint64)))


def transpose(nrows, ncols, m):
    """csr::transpose: column by column, within one in the order of the rows"""
    rp, ci, v = m
    rows = np.repeat(np.arange(nrows), np.diff(rp))
    order = np.argsort(ci, kind="stable")
    trp = np.zeros(ncols + 1, np.int32)
    np.add.at(trp, np.asarray(ci) + 1, 1)
    return np.cumsum(trp).astype(np.int32), rows[order].astype(np.int32), np.asarray(v, np.float64)[order]


def aggregation_2x2(g):
    """piecewise-constant prolongation of a g x g grid over 2 x 2 aggregates: (g*g) x (g/2)^2, one 1.0 per row"""
    p = np.arange(g * g)
    cols = ((p // g) // 2) * (g // 2) + (p % g) // 2
    return np.arange(g * g + 1, dtype=np.int32), cols.astype(np.int32), np.ones(g * g)


def random_rows(nrows, ncols, counts, rng, sort=True, repeat=False):
    """rows of the given lengths with uniformly drawn columns; repeat=True draws with replacement"""
    rp = np.zeros(nrows + 1, np.int32)
    rp[1:] = np.cumsum(counts)
    ci = np.empty(rp[-1], np.int32)
    for r in range(nrows):
        c = rng.choice(ncols, size=counts[r], replace=repeat) if counts[r] else np.empty(0, np.int64)
        ci[rp[r]:rp[r + 1]] = np.sort(c) if sort else c
    return rp, ci, rng.uniform(-1.0, 1.0, rp[-1])
