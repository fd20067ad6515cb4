"""Dense::apply and Dense::transpose restated in numpy, and the case list the CPU and the GPU module share.

ordered:   reference/matrix/dense_kernels.cpp:70-121 -- one chain per c(i,j) over ascending l, product and sum rounded
           separately (numpy never fuses), from +0.0 (simple) or from c * beta (advanced, beta == 0 multiplies too),
           with alpha * a rounded before it meets b.
split:     the chunked order of gkomi_dense_gemm_f64's mode 2: per chunk of `chunk` values of l the ordered chain
           from +0.0, the partials added to c * beta (or +0.0) in ascending chunk order.
transpose: reference/matrix/dense_kernels.cpp:813-822.
"""
import ctypes
import functools

import numpy as np

import ref_exec

VARIANTS = (("simple", None, None), ("adv_2.5_-1", 2.5, -1.0), ("adv_-0.75_0", -0.75, 0.0))
A_PAD, B_PAD, C_PAD = 3, 2, 1     # columns of padding behind a, b and c
FILL = -77.0                      # what the padding holds (ref_exec.dense_arrays' default)


def _chain(acc, sa, b):
    for l in range(sa.shape[1]):
        acc = acc + sa[:, l:l + 1] * b[l:l + 1, :]
    return acc


def ordered(a, b, c0=None, alpha=None, beta=None):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if alpha is None:
            return _chain(np.zeros((a.shape[0], b.shape[1])), a, b)
        return _chain(np.asarray(c0, np.float64) * np.float64(beta), np.float64(alpha) * a, b)


def split(a, b, c0=None, alpha=None, beta=None, chunk=1):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    m, k, n = a.shape[0], a.shape[1], b.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        sa = a if alpha is None else np.float64(alpha) * a
        acc = np.zeros((m, n)) if alpha is None else np.asarray(c0, np.float64) * np.float64(beta)
        for lo in range(0, k, chunk):
            hi = min(k, lo + chunk)
            acc = acc + _chain(np.zeros((m, n)), sa[:, lo:hi], b[lo:hi, :])
        return acc


def transpose(a):
    a = np.asarray(a)
    out = np.empty((a.shape[1], a.shape[0]), a.dtype)
    for i in range(a.shape[0]):
        for j in range(a.shape[1]):
            out[j, i] = a[i, j]
    return out


def split_bound(a, b, c0, alpha, beta):
    """(k + 2) 2^-52 S with S = (|alpha| |a|) |b| + |beta c0|: the ordered and the chunked sum both lie within
    gamma_{k+1} S of the exact value.  Entries whose S is not finite (NaN / Inf in c0) are left to the bit checks."""
    k = a.shape[1]
    al, be = (1.0, 0.0) if alpha is None else (alpha, beta)
    with np.errstate(invalid="ignore"):
        s = (abs(al) * np.abs(a)) @ np.abs(b) + (np.abs(be * c0) if alpha is not None else 0.0)
    return (k + 2) * 2.0 ** -52 * s


@functools.lru_cache(maxsize=None)
def geometry(gk):
    """T_m, T_n, T_k of the tile kernel, widest n, R and K_c of the narrow kernel, L of the split: the library's own."""
    vals = [ctypes.c_int64(0) for _ in range(6)]
    gk.dense_gemm_geometry(*[ctypes.addressof(v) for v in vals])
    names = ("T_m", "T_n", "T_k", "narrow_n", "R", "K_c")
    geo = {k: v.value for k, v in zip(names, vals)}
    geo["L"] = int(gk.dense_gemm_split_chunk())
    return geo


ROW_PERIOD = 5


def operands(m, n, k, seed, period=ROW_PERIOD, signed_zero=False):
    """a (m x k), b (k x n), c0 (m x n).  Standard normal entries, a -0.0 and a 0.0 in a, NaN and Inf in c0 (where c0
    has three entries or more).
    period: rows of a and c0 repeat with this period (so do the rows of every result, which keeps the recording of
    the reference's results small: a row is computed in full, by its own thread, wherever it sits; 5 is coprime to every
    size of the kernels' geometry); None: every row its own.  signed_zero: the case of include/gkomi.h where a padded
    +0.0 product would show -- a = 0, b < 0, c = 0, to be run with alpha = 1, beta = -1: all -0.0."""
    rng = np.random.default_rng(seed)
    if signed_zero:
        return np.zeros((m, k)), -1.0 - rng.random((k, n)), np.zeros((m, n))
    rows = m if period is None else min(m, period)
    a, c0 = rng.standard_normal((rows, k)), rng.standard_normal((rows, n))
    b = rng.standard_normal((k, n))
    if k > 0:
        a[0, 0] = -0.0
        a[rows - 1, k - 1] = 0.0
        if k > 2:
            a[0, 1] = 0.0
    if rows * n >= 3:
        c0[0, 0] = np.nan
        c0[rows - 1, n - 1] = np.inf
    reps = -(-m // rows)
    return np.tile(a, (reps, 1))[:m].copy(), b, np.tile(c0, (reps, 1))[:m].copy()


def ordered_shapes(geo):
    """(kernel, m, n, k) of the ordered checks: the edges of the tile and of the narrow kernel"""
    tm, tn, tk, r, kc = geo["T_m"], geo["T_n"], geo["T_k"], geo["R"], geo["K_c"]
    assert tn - 1 > geo["narrow_n"]
    tile = [(m, n, k) for m in (tm - 1, tm, tm + 1) for n in (tn - 1, tn, tn + 1)
            for k in (1, tk - 1, tk, tk + 1, 2 * tk + 1)]
    tile += [(1, geo["narrow_n"] + 1, 1), (tm, tn + 1, 0), (130, 70, 33)]
    narrow = [(m, n, k) for n in (1, 3, 16) for m in (1, r - 1, r, r + 1, 2 * r + 1) for k in (kc - 1, kc, kc + 1, 100)]
    narrow += [(1, 1, 1), (r + 1, 3, 0)]
    return [("tile",) + s for s in tile] + [("narrow",) + s for s in narrow]


def split_shapes(geo):
    big = geo["L"]
    shapes = [(m, n, k) for k in (big - 1, big, big + 1, 2 * big + 1, 5 * big + 3) for (m, n) in ((1, 1), (3, 2), (16, 16))]
    return shapes + [(5, geo["narrow_n"] + 4, 2 * big + 1)]   # partials by the tile kernel


class Case:
    def __init__(self, group, m, n, k, variant, signed_zero=False):
        self.group, self.m, self.n, self.k, self.signed_zero = group, m, n, k, signed_zero
        self.name, self.alpha, self.beta = variant
        self.id = f"{group}-{m}x{n}x{k}-{self.name}" + ("-signed_zero" if signed_zero else "")

    @functools.cached_property
    def data(self):
        seed = [self.m, self.n, self.k, 7 if self.signed_zero else 0]
        return operands(self.m, self.n, self.k, seed, signed_zero=self.signed_zero)

    def c_buffer(self):
        """what c holds before the apply: c0 (NaN-filled for a simple apply, which must overwrite it) + padding"""
        c0 = self.data[2] if self.alpha is not None else np.full((self.m, self.n), np.nan)
        buf = np.full((self.m, self.n + C_PAD), FILL)
        buf[:, :self.n] = c0
        return buf

    def queue(self, batch):
        a, b, _ = self.data
        m, n, k = self.m, self.n, self.k
        arrays, params = ref_exec.csr_arrays(m, k, np.arange(m + 1) * k, np.tile(np.arange(k), m), a.reshape(-1))
        for name, arr, stride in (("b", b, n + B_PAD), ("x", self.c_buffer()[:, :n], n + C_PAD)):
            arrs, pars = ref_exec.dense_arrays(name, arr, stride)
            arrays.update(arrs)
            params.update(pars)
        if self.alpha is not None:
            params.update(mode=1, alpha=self.alpha, beta=self.beta)
        else:
            params.update(mode=0)
        return batch.add("spmv", arrays, fmt=ref_exec.DENSE, **params)

    def restated(self, fn=ordered, **kw):
        a, b, c0 = self.data
        buf = self.c_buffer()
        buf[:, :self.n] = fn(a, b, c0, self.alpha, self.beta, **kw)
        return buf


def cases(geo):
    """the GPU module's whole case list, in the order of the recording"""
    out = []
    for kernel, m, n, k in ordered_shapes(geo):
        out += [Case(kernel, m, n, k, v) for v in VARIANTS]
    one = ("adv_1_-1", 1.0, -1.0)
    out.append(Case("tile", geo["T_m"] + 1, geo["T_n"] + 1, geo["T_k"] + 1, one, signed_zero=True))
    out.append(Case("narrow", geo["R"] + 1, 3, geo["K_c"] + 1, one, signed_zero=True))
    for m, n, k in split_shapes(geo):
        out += [Case("split", m, n, k, v) for v in VARIANTS]
    return out


def batch_of(case_list):
    batch = ref_exec.Batch()
    return batch, [c.queue(batch) for c in case_list]
