"""The sparse direct solver in plain Python, loop for loop as the reference executor writes it: the elimination forest
(core/factorization/elimination_forest.cpp:44-152), cholesky_symbolic_count / cholesky_symbolic_factorize
(reference/factorization/cholesky_kernels.cpp:58-128), symbolic_cholesky (core/factorization/symbolic.cpp:66-93),
lu_factorization::initialize / factorize (reference/factorization/lu_kernels.cpp:58-126) and Direct::apply
(core/solver/direct.cpp:186-203) with the triangular loops of reference/solver/{lower,upper}_trs_kernels.cpp:98-118.
Python floats are IEEE doubles, one rounding per operation.  The yardstick of tests/test_lu_gpu.py, with the matrices
both test files share."""
import os

import numpy as np

import ilu_exact_util as xu
import matgen

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- elimination forest ---------------------------------------------------------------------------------

FOREST_FIELDS = ("parents", "child_ptrs", "children", "postorder", "inv_postorder", "postorder_parents")


def elimination_forest(m):
    """dict of the six int32 arrays; the pseudo-root is n"""
    row_ptrs, cols = [int(x) for x in m[0]], [int(x) for x in m[1]]
    n = len(row_ptrs) - 1
    # parents; the disjoint sets only have to answer find / join, their representatives do not reach the result
    up = list(range(n))

    def find(x):
        while up[x] != x:
            up[x] = up[up[x]]
            x = up[x]
        return x

    parent = [n] * n
    subtree_root = list(range(n))
    for row in range(n):
        row_rep = row
        for nz in range(row_ptrs[row], row_ptrs[row + 1]):
            col = cols[nz]
            if col < row:
                col_rep = find(col)
                col_root = subtree_root[col_rep]
                if parent[col_root] == n and col_root != row:
                    parent[col_root] = row
                    up[col_rep] = row_rep          # join: row_rep stays the representative
                    subtree_root[row_rep] = row
    # children
    child_ptr = [0] * (n + 2)
    for i in range(n):
        if parent[i] < n:
            child_ptr[parent[i] + 2] += 1
    for i in range(1, n + 2):
        child_ptr[i] += child_ptr[i - 1]
    child = [0] * n
    for i in range(n):
        p = parent[i]
        child[child_ptr[p + 1]] = i
        child_ptr[p + 1] += 1
    # postorder
    current_child = [0] * (n + 1)
    postorder, inv_postorder = [0] * n, [0] * n
    idx = 0
    for tree in range(child_ptr[n], child_ptr[n + 1]):
        cur = child[tree]
        while cur < n:
            first = child_ptr[cur]
            if current_child[cur] >= child_ptr[cur + 1] - first:
                postorder[idx] = cur
                inv_postorder[cur] = idx
                cur = parent[cur]
                idx += 1
            else:
                old = cur
                cur = child[first + current_child[old]]
                current_child[old] += 1
    postorder_parent = [0] * n
    for row in range(n):
        postorder_parent[inv_postorder[row]] = n if parent[row] == n else inv_postorder[parent[row]]
    vals = (parent, child_ptr, child, postorder, inv_postorder, postorder_parent)
    return {k: np.array(v, np.int32) for k, v in zip(FOREST_FIELDS, vals)}


# ---- symbolic Cholesky ----------------------------------------------------------------------------------

def _row_paths(m, forest):
    """per row, the nodes cholesky_symbolic_factorize emits, in its order, the diagonal last"""
    row_ptrs, cols = [int(x) for x in m[0]], [int(x) for x in m[1]]
    parent = [int(x) for x in forest["parents"]]
    n = len(row_ptrs) - 1
    out = []
    for row in range(n):
        visited = {row}
        r = []
        for nz in range(row_ptrs[row], row_ptrs[row + 1]):
            col = cols[nz]
            if col < row:
                node = col
                while node not in visited:
                    visited.add(node)
                    r.append(node)
                    node = parent[node]
        r.append(row)
        out.append(r)
    return out


def cholesky_symbolic_count(m, forest):
    return np.array([len(r) for r in _row_paths(m, forest)], np.int32)


def cholesky_symbolic_factorize(m, forest):
    """(row_ptrs, cols) of L, rows in the order the reference executor emits them (unsorted)"""
    paths = _row_paths(m, forest)
    rp = np.zeros(len(paths) + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in paths])
    return rp, np.array([c for r in paths for c in r], np.int32)


def merge_patterns(a, b):
    """the pattern csr::spgeam gives for two matrices with sorted rows (reference/components/csr_spgeam.hpp:58-104)"""
    n = len(a[0]) - 1
    rp, ci = [0], []
    for row in range(n):
        ci += sorted(set(int(c) for c in a[1][a[0][row]:a[0][row + 1]]) |
                     set(int(c) for c in b[1][b[0][row]:b[0][row + 1]]))
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32)


def symbolic_cholesky(m):
    """-> (L, combined): the sorted pattern of L and the pattern of L + L^T, both with zero values"""
    forest = elimination_forest(m)
    rp, ci = cholesky_symbolic_factorize(m, forest)
    L = xu.sort_by_column_index((rp, ci, np.zeros(len(ci))))
    Lt = xu.transpose(L)
    crp, cci = merge_patterns(Lt, L)
    return L, (crp, cci, np.zeros(len(cci)))


# ---- lu_factorization -----------------------------------------------------------------------------------

def _lookup(cols, begin, end, col):
    for z in range(begin, end):
        if cols[z] == col:
            return z
    raise KeyError(col)   # lookup_unsafe: undefined in the reference


def lu_initialize(a, factor_pattern):
    """-> (factor with A's values scattered into its pattern, diag_idxs)"""
    arp, aci, av = xu._lists(a)
    frp, fci = [int(x) for x in factor_pattern[0]], [int(x) for x in factor_pattern[1]]
    n = len(frp) - 1
    fv = [0.0] * len(fci)
    diag = [0] * n
    for row in range(n):
        for nz in range(arp[row], arp[row + 1]):
            fv[_lookup(fci, frp[row], frp[row + 1], aci[nz])] = av[nz]
        diag[row] = _lookup(fci, frp[row], frp[row + 1], row)
    return xu._arrays(frp, fci, fv), np.array(diag, np.int32)


def lu_factorize(factor, diag_idxs):
    row_ptrs, cols, vals = xu._lists(factor)
    diag = [int(x) for x in diag_idxs]
    n = len(row_ptrs) - 1
    for row in range(n):
        row_begin, row_end = row_ptrs[row], row_ptrs[row + 1]
        where = {cols[z]: z for z in range(row_begin, row_end)}
        for lower_nz in range(row_begin, diag[row]):
            dep = cols[lower_nz]
            dep_diag_idx = diag[dep]
            scale = xu._div(vals[lower_nz], vals[dep_diag_idx])
            vals[lower_nz] = scale
            for dep_nz in range(dep_diag_idx + 1, row_ptrs[dep + 1]):
                nz = where[cols[dep_nz]]     # lookup_unsafe
                vals[nz] -= scale * vals[dep_nz]
    return xu._arrays(row_ptrs, cols, vals)


def lu_generate(a, symbolic=None):
    """Lu::generate with symmetric_sparsity (symbolic None) or a given pattern -> (combined factor, diag_idxs)"""
    pattern = symbolic if symbolic is not None else symbolic_cholesky(a)[1]
    factor, diag = lu_initialize(a, pattern)
    return lu_factorize(factor, diag), diag


# ---- Direct ----------------------------------------------------------------------------------------------

def _trs(m, b, lower, unit_diag):
    row_ptrs, col_idxs, vals = xu._lists(m)
    n = len(row_ptrs) - 1
    b = np.asarray(b, np.float64).reshape(n, -1)
    x = np.zeros_like(b)
    for j in range(b.shape[1]):
        xj = [0.0] * n
        for step in range(n):
            row = step if lower else n - 1 - step
            diag = 1.0
            acc = float(b[row, j])
            for k in range(row_ptrs[row], row_ptrs[row + 1]):
                col = col_idxs[k]
                if (col < row) if lower else (col > row):
                    acc -= vals[k] * xj[col]
                if col == row:
                    diag = vals[k]
            xj[row] = acc if unit_diag else xu._div(acc, diag)
        x[:, j] = xj
    return x


def lower_trs(m, b, unit_diag):
    return _trs(m, b, True, unit_diag)


def upper_trs(m, b, unit_diag):
    return _trs(m, b, False, unit_diag)


def direct_apply(combined, b):
    """x = U^-1 (L^-1 b) on the combined factor: LowerTrs(unit_diagonal) then UpperTrs"""
    return upper_trs(combined, lower_trs(combined, b, True), False)


def spmv(m, x):
    rp, ci, v = m
    n = len(rp) - 1
    x = np.asarray(x, np.float64).reshape(n, -1)
    y = np.zeros_like(x)
    for row in range(n):
        for z in range(rp[row], rp[row + 1]):
            y[row] += v[z] * x[ci[z]]
    return y


# ---- matrices -------------------------------------------------------------------------------------------

def read_mtx(name):
    kind, nr, nc, rows, cols, vals = matgen.read_mtx(os.path.join(HERE, "golden", name))
    assert kind == "coo" and nr == nc
    return xu.sort_by_column_index(tuple(matgen.coo_to_csr(nr, rows, cols, vals)))


def pattern_rows(m):
    """per row, the sorted list of its columns"""
    return [sorted(int(c) for c in m[1][m[0][r]:m[0][r + 1]]) for r in range(len(m[0]) - 1)]


def symmetrize_pattern(m, fill=0.0):
    """the pattern of A + A^T; entries that A does not store get `fill`"""
    rows = xu.to_rows(m)
    for i, r in enumerate(list(rows)):
        for j in list(r):
            rows[j].setdefault(i, fill)
    return xu.from_rows(rows)


def diagonal(n):
    return xu.from_rows([{i: 2.0 + 0.25 * (i % 5)} for i in range(n)])


def tridiagonal_with_corners(n):
    """tridiagonal plus (n - 1, 0) and (0, n - 1): the last row's first lower entry climbs n - 2 forest steps"""
    rows = xu.to_rows(xu.tridiagonal(n, lower=-1.0, diag=4.0, upper=-1.25))
    rows[n - 1][0] = 0.5
    rows[0][n - 1] = -0.25
    return xu.from_rows(rows)


def grid_5pt(nx, ny):
    """5-point stencil on ny grid lines of nx points, numbered along the lines: bandwidth nx"""
    n, rp, ci, v = matgen.poisson_2d_5pt(ny, nx)
    return xu.sort_by_column_index((rp, ci, v))


def repeated_separable(A, copies=9, seed=5):
    """the pattern A block-diagonally `copies` times, values made diagonally dominant, the entries of every row
    shuffled, every third diagonal entry removed: disconnected forest, unsorted rows, absent diagonals"""
    A = np.asarray(A)
    k = A.shape[0]
    rng = np.random.default_rng(seed)
    rp, ci, v = [0], [], []
    for c in range(copies):
        for i in range(k):
            row = c * k + i
            cols = [c * k + j for j in range(k) if A[i, j] != 0 and not (j == i and row % 3 == 0)]
            order = rng.permutation(len(cols))
            for z in order:
                col = cols[z]
                ci.append(col)
                v.append(float(k + 1 + 0.125 * (row % 7)) if col == row else -0.5 - 0.0625 * ((row + col) % 5))
            rp.append(len(ci))
    return xu._arrays(rp, ci, v)


def unsymmetric_values(n=200, seed=23):
    """random_dominant symmetrized in pattern only: a_ij and a_ji differ, and where only one was stored the other
    one is an explicit small value"""
    m = xu.random_dominant(n, 2, 9, seed)
    rows = xu.to_rows(m)
    for i, r in enumerate(list(rows)):
        for j in list(r):
            rows[j].setdefault(i, 0.03125 * ((i * 7 + j * 3) % 11 - 5))
    return xu.from_rows(rows)


def with_zero_pivot():
    """u_11 becomes 0 in the elimination: inf and nan from there on (dense 4 x 4 pattern)"""
    return xu.dense_to_csr([[1, 1, 0, 2], [1, 1, 1, 0], [0, 1, 1, 1], [1, 0, 1, 0]], keep_zeros=True)


def new_values(m, seed):
    """the same pattern with other values, still diagonally dominant"""
    rng = np.random.default_rng(seed)
    rows = xu.to_rows(m)
    out = []
    for i, r in enumerate(rows):
        nr = {j: float(rng.uniform(-1, 1)) for j in r if j != i}
        if i in r:
            nr[i] = 1.0 + sum(abs(x) for x in nr.values())
        out.append(nr)
    return xu.from_rows(out)
