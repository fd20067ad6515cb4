"""Shared pieces of the reference-parity tests (test_ref_oracle_parity*.py,
test_ref_parity_gpu.py): the case registry that lets one driver process serve
a whole module, and the fixed-seed inputs.  Test infrastructure."""
import os

import numpy as np

import ref_exec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_csr(name):
    """(n, row_ptrs, col_idxs, values) of a square MatrixMarket fixture of tests/golden/."""
    import matgen
    kind, m, n, rows, cols, vals = matgen.read_mtx(os.path.join(GOLDEN, name + ".mtx"))
    assert kind == "coo" and m == n
    rp, ci, v = matgen.coo_to_csr(m, rows, cols, vals)
    return m, rp, ci, v


class Registry:
    """Cases register a function (oracle, batch) -> check; check(results)
    asserts.  prepare() queues every case, runs the driver once and keeps what
    each case needs; a case whose set-up raised re-raises in its own test."""

    def __init__(self):
        self.fns = {}

    def case(self, name):
        def deco(fn):
            assert name not in self.fns, name
            self.fns[name] = fn
            return fn
        return deco

    def names(self):
        return list(self.fns)

    def queue(self, oracle):
        """(batch, checks) with every case queued and nothing run yet."""
        batch = ref_exec.Batch()
        checks = {}
        for name, fn in self.fns.items():
            try:
                checks[name] = fn(oracle, batch)
            except Exception as e:  # noqa: BLE001 -- shown by the case's own test
                checks[name] = e
        return batch, checks

    def prepare(self, oracle, recording=None):
        batch, checks = self.queue(oracle)
        return checks, batch.run(recording)


def run_case(prepared, name, *args):
    checks, results = prepared
    chk = checks[name]
    if isinstance(chk, Exception):
        raise chk
    chk(results, *args)


def ok(res):
    assert "error" not in res, res["error"]
    return res


def rows_csr(nrows, ncols, counts, seed, sort=True, repeat=False):
    """Rows of the given lengths with uniformly drawn columns."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    rp = np.zeros(nrows + 1, np.int32)
    rp[1:] = np.cumsum(counts)
    ci = np.empty(rp[-1], np.int32)
    for r in range(nrows):
        k = int(counts[r])
        c = rng.choice(ncols, size=k, replace=repeat or k > ncols) if k else np.empty(0, np.int64)
        ci[rp[r]:rp[r + 1]] = np.sort(c) if sort else c
    return nrows, ncols, rp, ci, rng.uniform(-1.0, 1.0, int(rp[-1]))


def spmv_matrices():
    """name -> (m, n, rp, ci, v): the shapes at which the GPU tests lean on the restatements."""
    rng = np.random.default_rng(11)
    mats = {}
    mats["empty"] = (0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    counts = rng.integers(0, 9, 40)
    counts[5:17] = 0
    counts[30:] = 0
    mats["empty_rows"] = rows_csr(40, 37, counts, 1)
    mats["one_row"] = rows_csr(1, 50, [23], 2)
    mats["one_col"] = rows_csr(50, 1, rng.integers(0, 2, 50), 3)
    m, n, rp, ci, v = rows_csr(130, 60, rng.integers(0, 30, 130), 4, sort=False, repeat=True)
    v[::5] = 0.0
    mats["unsorted_repeated_zeros"] = (m, n, rp, ci, v)
    m, n, rp, ci, v = rows_csr(65, 65, rng.integers(1, 12, 65), 5)
    v[3], v[10], v[17], v[29] = -0.0, np.inf, -np.inf, np.nan
    mats["special_values"] = (m, n, rp, ci, v)
    counts = np.array([3, 1537, 0, 3073, 7, 5000, 1, 0, 1536, 2])
    mats["long_rows"] = rows_csr(10, 6000, counts, 6)
    mats["irregular"] = rows_csr(700, 650, np.minimum(rng.geometric(0.12, 700) - 1, 400), 7, sort=False)
    for name in ("ani1", "ani4", "1138_bus"):
        n, rp, ci, v = golden_csr(name)
        mats[name] = (n, n, rp, ci, v)
    return mats


def rhs(rows, nrhs, seed, special=False):
    rng = np.random.default_rng(seed)
    b = rng.uniform(-2.0, 2.0, (rows, nrhs))
    if special and rows >= 8:
        b[1, 0], b[4, -1], b[6, 0], b[7, -1] = -0.0, np.inf, np.nan, -np.inf
    return b


def padded(a, stride, fill=-77.0):
    """(rows, stride) buffer holding a in its first columns."""
    buf = np.full((a.shape[0], stride), fill, a.dtype)
    buf[:, :a.shape[1]] = a
    return buf


def grid_5pt_reversed(g):
    """The g x g five-point matrix with every row's entries in descending column order."""
    import matgen
    n, rp, ci, v = matgen.poisson_2d_5pt(g)
    ci, v = ci.copy(), v.copy()
    for r in range(n):
        ci[rp[r]:rp[r + 1]] = ci[rp[r]:rp[r + 1]][::-1]
        v[rp[r]:rp[r + 1]] = v[rp[r]:rp[r + 1]][::-1]
    return n, rp, ci, v


# bytes per stored value of a precision_reduction, as the byte the reference keeps (preserving << 4 | nonpreserving)
PREC_BYTES = {0x00: 8, 0x01: 4, 0x02: 2, 0x10: 4, 0x11: 2, 0x20: 2}


def jacobi_written(scheme, ptrs, prec, nbytes):
    """Mask of the bytes of the block storage that hold block entries
    (block_interleaved_storage_scheme, include/ginkgo/core/preconditioner/jacobi.hpp:63-170)."""
    block_offset, group_offset, group_power = (int(x) for x in scheme)
    stride = block_offset << group_power
    mask = np.zeros(nbytes, bool)
    for b in range(len(ptrs) - 1):
        es = PREC_BYTES[int(prec[b])] if len(prec) else 8
        base = group_offset * (b >> group_power) * 8 + block_offset * (b & ((1 << group_power) - 1)) * es
        bs = int(ptrs[b + 1] - ptrs[b])
        for c in range(bs):
            at = base + c * stride * es
            mask[at:at + bs * es] = True
    return mask
