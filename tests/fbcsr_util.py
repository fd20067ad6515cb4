"""The Fbcsr loops of the reference (reference/matrix/fbcsr_kernels.cpp, csr::convert_to_fbcsr of
reference/matrix/csr_kernels.cpp:464-530) restated in plain Python on numpy arrays: scalar row by scalar row, one
IEEE-double multiply and one add per term (Python floats: no fused multiply-add, no pairwise sums), so the order of
the additions is the reference's.  The checker of tests/test_fbcsr_*.py; tied to the C oracle in
test_fbcsr_reference.py.

Layout: row_ptrs[nbrows + 1], col_idxs[nbnz] (block columns), vals[nbnz * bs * bs], entry (ib, jb) of block z at
z * bs * bs + ib + jb * bs."""
import numpy as np


def spmv(bs, row_ptrs, col_idxs, vals, b, c=None, alpha=None, beta=None):
    """fbcsr::spmv (:72-107) / advanced_spmv (:112-151); b, c 2-d; returns the new c"""
    nbrows = len(row_ptrs) - 1
    nvecs = b.shape[1]
    rp, ci, v, bl = row_ptrs.tolist(), col_idxs.tolist(), vals.tolist(), b.tolist()
    out = [[0.0] * nvecs for _ in range(nbrows * bs)] if alpha is None else np.asarray(c, dtype=np.float64).tolist()
    if alpha is not None:
        alpha, beta = float(alpha), float(beta)
    for ibrow in range(nbrows):
        for row in range(ibrow * bs, (ibrow + 1) * bs):
            for j in range(nvecs):
                out[row][j] = 0.0 if alpha is None else out[row][j] * beta
        for inz in range(rp[ibrow], rp[ibrow + 1]):
            for ib in range(bs):
                row = ibrow * bs + ib
                for jb in range(bs):
                    val = v[inz * bs * bs + ib + jb * bs]
                    col = ci[inz] * bs + jb
                    for j in range(nvecs):
                        if alpha is None:
                            out[row][j] += val * bl[col][j]
                        else:
                            out[row][j] += alpha * val * bl[col][j]   # (valpha * val) * b
    return np.array(out, dtype=np.float64).reshape(nbrows * bs, nvecs)


def csr_to_fbcsr(nrows, ncols, bs, row_ptrs, col_idxs, vals):
    """csr::convert_to_fbcsr (csr_kernels.cpp:464-530) -> (row_ptrs, col_idxs, vals)"""
    assert nrows % bs == 0 and ncols % bs == 0
    entries = [(row, int(col_idxs[nz]), float(vals[nz])) for row in range(nrows)
               for nz in range(int(row_ptrs[row]), int(row_ptrs[row + 1]))]
    entries.sort(key=lambda e: (e[0] // bs, e[1] // bs))   # stable; inside a block the order does not matter
    nbrows = nrows // bs
    out_ptrs = np.zeros(nbrows + 1, dtype=np.int32)
    out_cols, out_vals = [], []
    block_row, block_col = -1, -1
    for row, col, val in entries:
        while row // bs > block_row:
            out_ptrs[block_row + 1] = len(out_cols)
            block_col = -1
            block_row += 1
        if col // bs != block_col:
            out_cols.append(col // bs)
            out_vals.extend([0.0] * (bs * bs))
            block_col = col // bs
        out_vals[len(out_vals) - bs * bs + row % bs + (col % bs) * bs] = val
    while block_row < nbrows:
        out_ptrs[block_row + 1] = len(out_cols)
        block_row += 1
    return out_ptrs, np.array(out_cols, dtype=np.int32), np.array(out_vals, dtype=np.float64)


def to_csr(bs, row_ptrs, col_idxs, vals):
    """fbcsr::convert_to_csr (:252-304) -> (row_ptrs, col_idxs, vals), explicit zeros kept"""
    nbrows = len(row_ptrs) - 1
    nnz = len(col_idxs) * bs * bs
    out_ptrs = np.zeros(nbrows * bs + 1, dtype=np.int32)
    out_cols, out_vals = np.zeros(nnz, dtype=np.int32), np.zeros(nnz, dtype=np.float64)
    for brow in range(nbrows):
        start, count = int(row_ptrs[brow]), int(row_ptrs[brow + 1] - row_ptrs[brow])
        for ib in range(bs):
            out_ptrs[brow * bs + ib] = start * bs * bs + count * bs * ib
        for ibnz in range(start, start + count):
            for ib in range(bs):
                at = out_ptrs[brow * bs + ib] + (ibnz - start) * bs
                for jb in range(bs):
                    out_vals[at + jb] = vals[ibnz * bs * bs + ib + jb * bs]
                    out_cols[at + jb] = col_idxs[ibnz] * bs + jb
    out_ptrs[nbrows * bs] = nnz
    return out_ptrs, out_cols, out_vals


def fill_in_dense(nbcols, bs, row_ptrs, col_idxs, vals):
    """fbcsr::fill_in_dense (:216-245) on a zero matrix"""
    nbrows = len(row_ptrs) - 1
    out = np.zeros((nbrows * bs, nbcols * bs))
    for brow in range(nbrows):
        for ibnz in range(int(row_ptrs[brow]), int(row_ptrs[brow + 1])):
            for ib in range(bs):
                for jb in range(bs):
                    out[brow * bs + ib, col_idxs[ibnz] * bs + jb] = vals[ibnz * bs * bs + ib + jb * bs]
    return out


def transpose(nbcols, bs, row_ptrs, col_idxs, vals):
    """fbcsr::transpose (:310-388) -> (row_ptrs, col_idxs, vals) of the nbcols x nbrows block matrix"""
    nbrows, nbnz = len(row_ptrs) - 1, len(col_idxs)
    t_ptrs = np.zeros(nbcols + 1, dtype=np.int32)
    for i in range(nbnz):
        t_ptrs[col_idxs[i] + 1] += 1
    total = 0
    for i in range(nbcols):            # components::prefix_sum on t_ptrs + 1
        count, t_ptrs[i + 1] = t_ptrs[i + 1], total
        total += count
    cursor = t_ptrs[1:].copy()          # convert_fbcsr_to_fbcsc advances col_ptrs = t_ptrs + 1 ...
    t_cols, t_vals = np.zeros(nbnz, dtype=np.int32), np.zeros(nbnz * bs * bs, dtype=np.float64)
    for brow in range(nbrows):
        for i in range(int(row_ptrs[brow]), int(row_ptrs[brow + 1])):
            dest = cursor[col_idxs[i]]
            cursor[col_idxs[i]] += 1
            t_cols[dest] = brow
            for ib in range(bs):
                for jb in range(bs):
                    t_vals[dest * bs * bs + ib + jb * bs] = vals[i * bs * bs + jb + ib * bs]
    t_ptrs[1:] = cursor                 # ... which leaves the pointers one place further: the row pointers
    t_ptrs[0] = 0
    return t_ptrs, t_cols, t_vals


def is_sorted(row_ptrs, col_idxs):
    """fbcsr::is_sorted_by_column_index (:406-425)"""
    for i in range(len(row_ptrs) - 1):
        for idx in range(int(row_ptrs[i]) + 1, int(row_ptrs[i + 1])):
            if col_idxs[idx - 1] > col_idxs[idx]:
                return False
    return True


def sort(bs, row_ptrs, col_idxs, vals):
    """fbcsr::sort_by_column_index (:434-483) -> (col_idxs, vals); equal block columns keep their order"""
    out_cols, out_vals = np.array(col_idxs, dtype=np.int32), np.array(vals, dtype=np.float64)
    bs2 = bs * bs
    for irow in range(len(row_ptrs) - 1):
        start, end = int(row_ptrs[irow]), int(row_ptrs[irow + 1])
        perm = sorted(range(end - start), key=lambda k: col_idxs[start + k])
        for ibz, src in enumerate(perm):
            out_cols[start + ibz] = col_idxs[start + src]
            for i in range(bs2):
                out_vals[(start + ibz) * bs2 + i] = vals[(start + src) * bs2 + i]
    return out_cols, out_vals


def extract_diagonal(nbcols, bs, row_ptrs, col_idxs, vals, diag=None):
    """fbcsr::extract_diagonal (:490-522); only stored diagonal blocks are written (into `diag`, else zeros)"""
    nbdim = min(len(row_ptrs) - 1, nbcols)
    out = np.zeros(nbdim * bs) if diag is None else np.array(diag, dtype=np.float64)
    for ibrow in range(nbdim):
        for idx in range(int(row_ptrs[ibrow]), int(row_ptrs[ibrow + 1])):
            if col_idxs[idx] == ibrow:
                for ib in range(bs):
                    out[ibrow * bs + ib] = vals[idx * bs * bs + ib + ib * bs]
                break
    return out


def random_block_csr(nbrows, nbcols, bs, blocks_per_row, seed, sorted=True, fill=0.7):
    """A CSR matrix made of bs x bs blocks, `blocks_per_row` blocks (an int or one int per block row) at distinct
    random block columns; every block holds its (0, 0) entry and each other entry with probability `fill`, so some
    blocks are only partly populated.  sorted=False shuffles the entries inside each scalar row.
    -> (nrows, ncols, row_ptrs, col_idxs, vals)"""
    rng = np.random.default_rng(seed)
    counts = [blocks_per_row] * nbrows if np.isscalar(blocks_per_row) else list(blocks_per_row)
    rows = [[] for _ in range(nbrows * bs)]
    for brow in range(nbrows):
        bcols = np.sort(rng.choice(nbcols, size=min(counts[brow], nbcols), replace=False))
        for bcol in bcols:
            keep = rng.random((bs, bs)) < fill
            keep[0, 0] = True
            for ib in range(bs):
                for jb in range(bs):
                    if keep[ib, jb]:
                        rows[brow * bs + ib].append((int(bcol) * bs + jb, float(rng.uniform(-1.0, 1.0))))
    row_ptrs, col_idxs, vals = [0], [], []
    for r in rows:
        if not sorted:
            r = [r[k] for k in rng.permutation(len(r))]
        col_idxs.extend(c for c, _ in r)
        vals.extend(v for _, v in r)
        row_ptrs.append(len(col_idxs))
    return (nbrows * bs, nbcols * bs, np.array(row_ptrs, dtype=np.int32), np.array(col_idxs, dtype=np.int32),
            np.array(vals, dtype=np.float64))
