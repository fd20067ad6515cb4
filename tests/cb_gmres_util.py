"""A numpy restatement of CB-GMRES: the four kernels of reference/solver/cb_gmres_kernels.cpp (initialize, restart,
arnoldi, solve_krylov), the storage of accessor/{reduced_row_major,scaled_reduced_row_major}.hpp and the driver of
core/solver/cb_gmres.cpp:204-487, forced-iteration logic included.  Two switches:

  half   "truncate": the reference executor's host conversion (core/base/extended_float.hpp:355-392: the significand is
         cut, subnormals become zero); "rne": double -> float -> half with round-to-nearest-even, subnormals kept,
         which is what the device code does;
  group  0: every sum over rows runs in row order like the reference's loops ("sequential"); g > 0 ("grouped"): rows
         are summed in consecutive groups of g, then the group totals in order -- a stand-in for any two-stage sum;
         ("device", rows per lane): the order in which csrc/cb_gmres.hip adds (device_sum below).

tests/test_cb_gmres_reference.py pins truncate + sequential to results recorded from the reference, bit for bit."""
import functools

import numpy as np

import ref_exec
from ref_exec import as_record, matches, unhex      # the GPU tests reach matches and unhex through this module

STORAGES = ("keep", "reduce1", "reduce2", "integer", "ireduce1", "ireduce2")
STORAGE_DTYPE = {"keep": np.float64, "reduce1": np.float32, "reduce2": np.uint16, "integer": np.int64,
                 "ireduce1": np.int32, "ireduce2": np.int16}
RAW_DTYPE = {"keep": np.int64, "reduce1": np.int32, "reduce2": np.int16, "integer": np.int64, "ireduce1": np.int32,
             "ireduce2": np.int16}
ETA = 1.0 / np.sqrt(2.0)
START_FORCE_RESET = 10
FORCED_ITERATION_FRACTION = 10


def is_scaled(storage):
    return storage in ("integer", "ireduce1", "ireduce2")


def correction(storage):
    """write_scalar (core/solver/cb_gmres_accessor.hpp:165-179)"""
    return 2 / float(np.iinfo(STORAGE_DTYPE[storage]).max) if is_scaled(storage) else 1.0


# ---- half ------------------------------------------------------------------------------------------------------

def float_to_half_bits(v, mode):
    f = np.asarray(v, np.float64).astype(np.float32)
    if mode == "rne":
        return f.astype(np.float16).view(np.uint16)
    assert mode == "truncate"
    bits = f.view(np.uint32).astype(np.uint64)
    sign = (bits & 0x80000000) >> 16
    expo = (bits & 0x7f800000) >> 13
    frac = bits & 0x007fffff
    is_inf = ((bits & 0x7f800000) == 0x7f800000) & (frac == 0)
    is_nan = ((bits & 0x7f800000) == 0x7f800000) & (frac != 0)
    bias_change = 0x1c000
    e = np.where(expo <= bias_change, 0, np.minimum(np.where(expo > bias_change, expo - bias_change, 0), 0x7c00))
    out = np.where(e == 0x7c00, sign | e, np.where(e == 0, sign, sign | e | (frac >> 13)))
    out = np.where(is_inf, sign | 0x7c00, np.where(is_nan, sign | 0x7fff, out))
    return out.astype(np.uint16)


def half_bits_to_double(bits, mode):
    bits = np.asarray(bits, np.uint16)
    if mode == "truncate":  # subnormals read as signed zero
        bits = np.where((bits & 0x7c00) == 0, bits & 0x8000, bits).astype(np.uint16)
    return bits.view(np.float16).astype(np.float32).astype(np.float64)


# ---- sums --------------------------------------------------------------------------------------------------------

def _butterfly(v):
    """wave_reduce_sum over the last axis of 64 lanes: lane ^ 32, 16, ... 1; every lane ends with the total"""
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ off]
    return v[..., 0]


def device_sum(p, per_lane, dot=False, block=512, cap=512):
    """the sum of p in the order of csrc/cb_gmres.hip: every lane adds its chunks of per_lane consecutive rows trip after
    trip, a wave adds its lanes as a butterfly, thread 0 adds the waves in order; the per-workgroup partials are then
    added by lanes striding over them, a butterfly and the waves in order (dot: the h of the update kernel, one wave
    striding by 64 and a butterfly)"""
    p = np.asarray(p, np.float64)
    chunks = -(-p.size // per_lane)
    blocks = min(cap, max(1, -(-chunks // block)))
    lanes = blocks * block
    trips = max(1, -(-chunks // lanes))
    padded = np.zeros(trips * lanes * per_lane)
    padded[:p.size] = p
    per = padded.reshape(trips, lanes, per_lane).transpose(1, 0, 2).reshape(lanes, trips * per_lane)
    lane_acc = np.cumsum(per, axis=1)[:, -1]
    waves = _butterfly(lane_acc.reshape(blocks, block // 64, 64))
    partials = np.cumsum(waves, axis=1)[:, -1]
    if dot:
        padded = np.zeros(-(-blocks // 64) * 64)
        padded[:blocks] = partials
        return float(_butterfly(np.cumsum(padded.reshape(-1, 64), axis=0)[-1]))
    padded = np.zeros(-(-blocks // block) * block)
    padded[:blocks] = partials
    acc = np.cumsum(padded.reshape(-1, block), axis=0)[-1]
    return float(np.cumsum(_butterfly(acc.reshape(block // 64, 64)))[-1])


def ssum(p, group=0, dot=False):
    """the sum of p in index order, by groups of `group`, or -- group = ("device", rows per lane) -- in the device's order"""
    p = np.asarray(p, np.float64)
    if p.size == 0:
        return 0.0
    if isinstance(group, tuple):
        return device_sum(p, group[1], dot)
    if group <= 0 or p.size <= group:
        return float(np.cumsum(p)[-1])
    full = p.size // group * group
    totals = list(np.cumsum(p[:full].reshape(-1, group), axis=1)[:, -1])
    if full < p.size:
        totals.append(np.cumsum(p[full:])[-1])
    return float(np.cumsum(np.array(totals))[-1])


# ---- storage -----------------------------------------------------------------------------------------------------

class Basis:
    """(krylov_dim + 1) x n x nrhs stored values, entry (k, row, col) at (k n + row) nrhs + col, and for the integer
    storages one scalar per (k, col), initialised to 1"""

    def __init__(self, krylov_dim, n, nrhs, storage, half="truncate"):
        self.storage, self.half = storage, half
        self.data = np.zeros((krylov_dim + 1, n, nrhs), STORAGE_DTYPE[storage])
        self.scalars = np.ones((krylov_dim + 1, nrhs))

    def read(self, k, col):
        raw = self.data[k, :, col]
        if self.storage == "reduce2":
            return half_bits_to_double(raw, self.half)
        if is_scaled(self.storage):
            return raw.astype(np.float64) * self.scalars[k, col]
        return raw.astype(np.float64)

    def write(self, k, col, v):
        v = np.asarray(v, np.float64)
        if self.storage == "reduce2":
            self.data[k, :, col] = float_to_half_bits(v, self.half)
        elif is_scaled(self.storage):
            self.data[k, :, col] = np.trunc(v / self.scalars[k, col]).astype(STORAGE_DTYPE[self.storage])
        else:
            self.data[k, :, col] = v.astype(STORAGE_DTYPE[self.storage])

    def write_scalar(self, k, col, value):
        if is_scaled(self.storage):
            self.scalars[k, col] = value * correction(self.storage)

    def raw(self):
        """the stored bits as signed integers of the storage's width"""
        return self.data.view(RAW_DTYPE[self.storage])

    def set_raw(self, raw):
        self.data[...] = np.asarray(raw, RAW_DTYPE[self.storage]).reshape(self.data.shape).view(self.data.dtype)


def compress(v, storage, scalar=1.0, half="rne"):
    """what a write of v stores, as raw integers"""
    b = Basis(0, len(v), 1, storage, half)
    b.scalars[0, 0] = scalar
    b.write(0, 0, v)
    return b.raw()[0, :, 0].copy()


# ---- the four kernels --------------------------------------------------------------------------------------------

def initialize(b, krylov_dim):
    nrhs = b.shape[1]
    return b.copy(), np.zeros((krylov_dim, nrhs)), np.zeros((krylov_dim, nrhs)), np.zeros(nrhs, np.uint8)


def restart(residual, basis, krylov_dim, arnoldi_norm, group=0, clear_rest=True):
    """-> residual_norm, residual_norm_collection, next_krylov_basis, final_iter_nums"""
    n, nrhs = residual.shape
    residual_norm = np.zeros(nrhs)
    rnc = np.zeros((krylov_dim + 1, nrhs))
    nxt = np.zeros((n, nrhs))
    for j in range(nrhs):
        r = residual[:, j]
        residual_norm[j] = np.sqrt(ssum(r * r, group))
        if is_scaled(basis.storage):
            arnoldi_norm[2, j] = np.max(np.abs(r)) if n else 0.0
        basis.write_scalar(0, j, arnoldi_norm[2, j] / residual_norm[j])
        rnc[0, j] = residual_norm[j]
        q = r / residual_norm[j]
        basis.write(0, j, q)
        nxt[:, j] = q
    if clear_rest:
        basis.data[1:] = 0
        if is_scaled(basis.storage):
            basis.scalars[1:] = 1.0 * correction(basis.storage)     # write_scalar(k, j, one) applies it too
    return residual_norm, rnc, nxt, np.zeros(nrhs, np.uint64)


def finish_arnoldi(nxt, basis, hess_iter, buffer_iter, arnoldi_norm, it, stopped, group=0, trace=None):
    """finish_arnoldi_CGS; hess_iter and buffer_iter: (it + 2) x nrhs views.  -> re-orthogonalisation passes per column
    (-1: stopped).  trace: a list that receives (norm_after / norm_before) of every loop test."""
    n, nrhs = nxt.shape
    passes = np.full(nrhs, -1, np.int64)
    scaled = is_scaled(basis.storage)
    for i in range(nrhs):
        v = nxt[:, i]
        arnoldi_norm[0, i] = ETA * np.sqrt(ssum(v * v, group))
        if stopped[i]:
            continue
        q = [basis.read(k, i) for k in range(it + 1)]
        for k in range(it + 1):
            hess_iter[k, i] = ssum(v * q[k], group, dot=True)
        for k in range(it + 1):
            v -= hess_iter[k, i] * q[k]
        arnoldi_norm[1, i] = np.sqrt(ssum(v * v, group))
        if scaled:
            arnoldi_norm[2, i] = np.max(np.abs(v)) if n else 0.0
        l = 1
        while True:
            if trace is not None:
                trace.append(arnoldi_norm[1, i] / arnoldi_norm[0, i] * ETA)
            if not (arnoldi_norm[1, i] < arnoldi_norm[0, i] and l < 3):
                break
            arnoldi_norm[0, i] = ETA * arnoldi_norm[1, i]
            for k in range(it + 1):
                buffer_iter[k, i] = ssum(v * q[k], group, dot=True)
            for k in range(it + 1):
                v -= buffer_iter[k, i] * q[k]
                hess_iter[k, i] += buffer_iter[k, i]
            arnoldi_norm[1, i] = np.sqrt(ssum(v * v, group))
            arnoldi_norm[2, i] = np.max(np.abs(v)) if n else 0.0
            l += 1
        passes[i] = l - 1
        basis.write_scalar(it + 1, i, arnoldi_norm[2, i] / arnoldi_norm[1, i])
        hess_iter[it + 1, i] = arnoldi_norm[1, i]
        v /= hess_iter[it + 1, i]
        basis.write(it + 1, i, v)
    return passes


def givens(gsin, gcos, residual_norm, rnc, hess_iter, it, stopped):
    """givens_rotation + calculate_next_residual_norm"""
    for i in range(hess_iter.shape[1]):
        if stopped[i]:
            continue
        for j in range(it):
            temp = gcos[j, i] * hess_iter[j, i] + gsin[j, i] * hess_iter[j + 1, i]
            hess_iter[j + 1, i] = -gsin[j, i] * hess_iter[j, i] + gcos[j, i] * hess_iter[j + 1, i]
            hess_iter[j, i] = temp
        this_h, next_h = hess_iter[it, i], hess_iter[it + 1, i]
        if this_h == 0.0:
            gcos[it, i], gsin[it, i] = 0.0, 1.0
        else:
            scale = abs(this_h) + abs(next_h)
            hyp = scale * np.sqrt(abs(this_h / scale) * abs(this_h / scale) + abs(next_h / scale) * abs(next_h / scale))
            gcos[it, i], gsin[it, i] = this_h / hyp, next_h / hyp
        hess_iter[it, i] = gcos[it, i] * this_h + gsin[it, i] * next_h
        hess_iter[it + 1, i] = 0.0
        rnc[it + 1, i] = -gsin[it, i] * rnc[it, i]
        rnc[it, i] = gcos[it, i] * rnc[it, i]
        residual_norm[i] = abs(rnc[it + 1, i])


def arnoldi(nxt, gsin, gcos, residual_norm, rnc, basis, hess_iter, buffer_iter, arnoldi_norm, it, final_iter_nums,
            stopped, group=0, trace=None):
    final_iter_nums += (1 - np.asarray(stopped, np.uint64)).astype(np.uint64)
    passes = finish_arnoldi(nxt, basis, hess_iter, buffer_iter, arnoldi_norm, it, stopped, group, trace)
    givens(gsin, gcos, residual_norm, rnc, hess_iter, it, stopped)
    return passes


def solve_krylov(rnc, basis, hessenberg, final_iter_nums):
    """hessenberg: rows x (cols nrhs), entry (i, j nrhs + k).  -> y (rows of hessenberg's column count / nrhs), before"""
    nrhs = rnc.shape[1]
    n = basis.data.shape[1]
    dim = basis.data.shape[0] - 1
    y = np.zeros((dim, nrhs))
    before = np.zeros((n, nrhs))
    for k in range(nrhs):
        m = int(final_iter_nums[k])
        for i in range(m - 1, -1, -1):
            temp = rnc[i, k]
            for j in range(i + 1, m):
                temp -= hessenberg[i, j * nrhs + k] * y[j, k]
            y[i, k] = temp / hessenberg[i, i * nrhs + k]
        acc = np.zeros(n)
        for j in range(m):
            acc += basis.read(j, k) * y[j, k]
        before[:, k] = acc
    return y, before


# ---- the system matrix, as the reference executor applies it ------------------------------------------------------------

class CsrOperator:
    """csr::spmv and csr::advanced_spmv of reference/matrix/csr_kernels.cpp:75-128: every row in entry order"""

    def __init__(self, n, row_ptrs, col_idxs, vals):
        self.n = n
        rp = np.asarray(row_ptrs, np.int64)
        self.len = np.diff(rp)
        self.width = int(self.len.max()) if n else 0
        self.cols = np.zeros((n, self.width), np.int64)
        self.vals = np.zeros((n, self.width))
        for k in range(self.width):
            rows = np.nonzero(self.len > k)[0]
            self.cols[rows, k] = np.asarray(col_idxs)[rp[rows] + k]
            self.vals[rows, k] = np.asarray(vals)[rp[rows] + k]

    def apply(self, b, alpha=None, beta=None, c=None):
        out = np.zeros_like(b) if alpha is None else c * beta
        for k in range(self.width):
            rows = self.len > k
            term = self.vals[rows, k, None] * b[self.cols[rows, k]]
            out[rows] += term if alpha is None else (alpha * self.vals[rows, k, None]) * b[self.cols[rows, k]]
        return out


def residual_norm_check(residual_norm, baseline_norm, reduction, status):
    """stop::ResidualNorm on the columns that have not stopped (id 2, finalized) -> all stopped, one changed"""
    changed = False
    for i in range(len(status)):
        if residual_norm[i] < reduction * baseline_norm[i]:
            if status[i] == 0:
                status[i] = 0x80 | 0x40 | 2
            changed = True      # also for a column that had converged before (reference/stop/residual_norm_kernels.cpp)
    return bool(np.all(status != 0)), changed


def solve(matrix, b, x, krylov_dim, storage, max_iters, reduction, baseline="rhs_norm", precond=None, half="truncate",
          group=0, trace=None):
    """CbGmres::apply_dense_impl with Combined(Iteration(max_iters), ResidualNorm(reduction, baseline)).  matrix: an
    object with apply(b, alpha, beta, c); precond: None or a function (n x nrhs) -> (n x nrhs); b, x: n x nrhs, x is
    updated in place.  -> dict(iterations, residual_norm, forced_resets, passes = how many steps took 0, 1, 2
    re-orthogonalisation passes, converged)"""
    n, nrhs = b.shape
    pre = (lambda v: v.copy()) if precond is None else precond
    basis = Basis(krylov_dim, n, nrhs, storage, half)
    hess = np.zeros((krylov_dim + 1, krylov_dim * nrhs))
    buffer = np.zeros((krylov_dim + 1, nrhs))
    arnoldi_norm = np.zeros((3, nrhs))
    passes_seen = [0, 0, 0]
    residual, gsin, gcos, status = initialize(b, krylov_dim)
    residual = matrix.apply(x, -1.0, 1.0, residual)
    residual_norm, rnc, nxt, fin = restart(residual, basis, krylov_dim, arnoldi_norm, group)
    if baseline == "rhs_norm":
        base = np.array([np.sqrt(ssum(b[:, j] * b[:, j], group)) for j in range(nrhs)])
    elif baseline == "initial_resnorm":
        base = residual_norm.copy()
    else:
        base = np.ones(nrhs)
    total_iter, restart_iter = -1, 0
    stop_encountered = np.zeros(nrhs, bool)
    fully_converged = np.zeros(nrhs, bool)
    perform_reset = False
    forced_limit = krylov_dim // FORCED_ITERATION_FRACTION
    forced_iterations = forced_limit
    forced_resets = 0

    def update_solution():
        _, before = solve_krylov(rnc, basis, hess, fin)
        x[...] += pre(before)

    while True:
        total_iter += 1
        if forced_iterations < forced_limit and forced_iterations < total_iter // FORCED_ITERATION_FRACTION:
            forced_iterations += 1
        else:
            if total_iter >= max_iters:
                status[status == 0] = 0x40 | 1
                all_changed = one_changed = True
            else:
                all_changed, one_changed = residual_norm_check(residual_norm, base, reduction, status)
            if one_changed or all_changed:
                host_changed = False
                for i in range(nrhs):
                    if fully_converged[i]:
                        continue
                    if status[i] & 0x80:
                        if stop_encountered[i] or total_iter < START_FORCE_RESET:
                            fully_converged[i] = True
                        else:
                            stop_encountered[i] = True
                            status[i] = 0
                            host_changed = True
                if host_changed:
                    perform_reset = True
                    forced_resets += 1
                else:
                    break
                forced_iterations = 0
            else:
                stop_encountered[:] = False
        if perform_reset or restart_iter == krylov_dim:
            perform_reset = False
            update_solution()
            residual = matrix.apply(x, -1.0, 1.0, b.copy())
            residual_norm, rnc, nxt, fin = restart(residual, basis, krylov_dim, arnoldi_norm, group)
            restart_iter = 0
        nxt = matrix.apply(pre(nxt))
        h_iter = hess[:restart_iter + 2, nrhs * restart_iter:nrhs * (restart_iter + 1)]
        p = arnoldi(nxt, gsin, gcos, residual_norm, rnc, basis, h_iter, buffer[:restart_iter + 2], arnoldi_norm,
                    restart_iter, fin, status != 0, group, trace)
        for c in p:
            if c >= 0:
                passes_seen[c] += 1
        restart_iter += 1
    update_solution()
    return {"iterations": total_iter, "residual_norm": residual_norm.copy(), "forced_resets": forced_resets,
            "passes": passes_seen, "converged": bool(np.all((status & 0x80) != 0)), "baseline_norm": base}


# ---- the recorded cases (ref_driver's verb cb_gmres -> tests/golden/cb_gmres_ref.json) ------------------------------

def _dense_case(rows, b, x, krylov_dim=100, reduction=1e-14, max_iters=100):
    """a known-answer system of reference/test/solver/cb_gmres_kernels.cpp (numbers only): baseline initial_resnorm"""
    return {"dense": rows, "b": b, "expect_x": x, "krylov_dim": krylov_dim, "reduction": reduction,
            "max_iters": max_iters, "baseline": "initial_resnorm", "jacobi": 0}


SOLVE_CASES = {
    "stencil": _dense_case([[1.0, 2.0, 3.0], [3.0, 2.0, -1.0], [0.0, -1.0, 2.0]], [13.0, 7.0, 1.0], [1.0, 3.0, 2.0]),
    "big1": _dense_case([[2295.7, -764.8, 1166.5, 428.9, 291.7, -774.5], [2752.6, -1127.7, 1212.8, -299.1, 987.7, 786.8],
                         [138.3, 78.2, 485.5, -899.9, 392.9, 1408.9], [-1907.1, 2106.6, 1026.0, 634.7, 194.6, -534.1],
                         [-365.0, -715.8, 870.7, 67.5, 279.8, 1927.8], [-848.1, -280.5, -381.8, -187.1, 51.2, -176.2]],
                        [72748.36, 297469.88, 347229.24, 36290.66, 82958.82, -80192.15],
                        [52.7, 85.4, 134.2, -250.0, -16.8, 35.3]),
    "medium_k4": _dense_case([[-86.40, 153.30, -108.90, 8.60, -61.60], [7.70, -77.00, 3.30, -149.20, 74.80],
                              [-121.40, 37.10, 55.30, -74.20, -19.20], [-111.40, -22.60, 110.10, -106.20, 88.90],
                              [-0.70, 111.70, 154.40, 235.00, -76.50]],
                             [-13945.16, 11205.66, 16132.96, 24342.18, -10910.98],
                             [-140.20, -142.20, 48.80, -17.70, -19.60], krylov_dim=4, max_iters=200),
    # the 3-D convection-diffusion stencil of tests/test_gmres_precond_gpu.py at 8^3
    "cd8_k5": {"grid": 8, "nrhs": 1, "krylov_dim": 5, "reduction": 1e-10, "max_iters": 2000, "baseline": "rhs_norm",
               "jacobi": 0},
    "cd8_k30": {"grid": 8, "nrhs": 1, "krylov_dim": 30, "reduction": 1e-10, "max_iters": 2000, "baseline": "rhs_norm",
                "jacobi": 0},
    # GMRES(30) again where the count behind a half basis survives every reordering of the sums (cd8_k30's does not,
    # see reordered_counts): 7^3 rows, an odd n, which the kernels sweep element by element, and 8^3 to 1e-6
    "cd7_k30": {"grid": 7, "nrhs": 1, "krylov_dim": 30, "reduction": 1e-10, "max_iters": 2000, "baseline": "rhs_norm",
                "jacobi": 0},
    "cd8_k30_r6": {"grid": 8, "nrhs": 1, "krylov_dim": 30, "reduction": 1e-6, "max_iters": 2000, "baseline": "rhs_norm",
                   "jacobi": 0},
    "cd8_jacobi": {"grid": 8, "nrhs": 1, "krylov_dim": 20, "reduction": 1e-10, "max_iters": 2000,
                   "baseline": "rhs_norm", "jacobi": 8},
    "cd6_3rhs": {"grid": 6, "nrhs": 3, "krylov_dim": 20, "reduction": 1e-8, "max_iters": 500, "baseline": "rhs_norm",
                 "jacobi": 0},
}
# kernel traces: restart, `steps` Arnoldi steps (column stop_col stopped from step stop_step on), solve_krylov
KERNEL_CASES = {
    "cd3_3rhs": {"grid": 3, "nrhs": 3, "krylov_dim": 5, "steps": 5, "stop_col": 1, "stop_step": 2},
    "cd3_1rhs": {"grid": 3, "nrhs": 1, "krylov_dim": 4, "steps": 4, "stop_col": 0, "stop_step": -1},
}


def right_hand_side(n, nrhs):
    j = np.arange(n, dtype=np.float64)
    return np.stack([np.cos(0.3 * j + 0.7 * c) * (1.0 + 10.0 ** (-3 * c) * (c > 0)) + (c == 2) * 1e-3 * j
                     for c in range(nrhs)], axis=1)


def solve_problem(case):
    """n, row_ptrs, col_idxs, vals, b (n x nrhs) of a case"""
    import matgen
    if "dense" in case:
        a = np.array(case["dense"], np.float64)
        n = a.shape[0]
        rp, ci, v = matgen.dense_to_csr(a)[-3:]
        return n, np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.asarray(v, np.float64), \
            np.array(case["b"], np.float64).reshape(n, 1)
    n, rp, ci, v = matgen.at_like(case["grid"], 0.5)
    return n, rp, ci, v, right_hand_side(n, case["nrhs"])


def queue_cases(batch):
    """queues every solve and every kernel trace, for every storage, on a ref_exec.Batch -> {case/storage: index}"""
    where = {}
    for op, cases in ((0, SOLVE_CASES), (1, KERNEL_CASES)):
        for name, c in cases.items():
            n, rp, ci, v, b = solve_problem(c)
            arrays, size = ref_exec.csr_arrays(n, n, rp, ci, v)
            rhs, shape = ref_exec.dense_arrays("b", b)
            if op == 0:
                params = dict(max_iters=c["max_iters"], reduction=c["reduction"], jacobi=c["jacobi"],
                              baseline=ref_exec.word("baseline", c["baseline"]))
            else:
                params = dict(steps=c["steps"], stop_col=c["stop_col"], stop_step=c["stop_step"])
            for storage in STORAGES:
                where[f"{name}/{storage}"] = batch.add("cb_gmres", {**arrays, **rhs}, op=op, krylov_dim=c["krylov_dim"],
                                                       storage=ref_exec.word("storage", storage), **params, **size, **shape)
    return where


def case_arrays(results, where):
    """{case/storage: {what: array}}; the Krylov basis comes back as the stored bits in the storage's own width and
    is widened here"""
    return {key: {what: a.view(RAW_DTYPE[key.split("/")[-1]]).astype(np.int64) if what.endswith("basis") else a
                  for what, a in results[i].items()} for key, i in where.items()}


def dump_fixture(fix, path):
    """one line per recorded case"""
    import json
    with open(path, "w") as f:
        f.write('{"source": ' + json.dumps(fix["source"]))
        for part in ("solves", "kernels"):
            f.write(',\n"' + part + '": {\n')
            f.write(",\n".join(json.dumps(k) + ": " + json.dumps(v) for k, v in fix[part].items()))
            f.write("\n}")
        f.write("}\n")


def restated_solve(name, storage, half, group=0, trace=None):
    """the restatement's solve of a case -> (x, result)"""
    c = SOLVE_CASES[name]
    n, rp, ci, v, b = solve_problem(c)
    x = np.zeros_like(b)
    res = solve(CsrOperator(n, rp, ci, v), b, x, c["krylov_dim"], storage, c["max_iters"], c["reduction"], c["baseline"],
                precond=jacobi_apply(n, rp, ci, v, c["jacobi"], b.shape[1]) if c["jacobi"] else None, half=half,
                group=group, trace=trace)
    return x, res


@functools.lru_cache(maxsize=None)
def _rne_iterations(name, storage, group):
    """the restatement's iteration count in "rne" mode: computed once, for the tests and for fixture_from"""
    return restated_solve(name, storage, "rne", group)[1]["iterations"]


def reordered_counts(name, storage):
    """the restatement's iteration counts ("rne") with the sums grouped by 64, by 1024 and in the device's own order: a
    case whose counts all stay within 1 of the sequential one is held to +-1 of the sequential count on the device; any
    other says nothing about a sum order but its own and is held to +-1 of the count in the device's order, the last"""
    per_lane = 16 // np.dtype(STORAGE_DTYPE[storage]).itemsize
    return [_rne_iterations(name, storage, g) for g in (64, 1024, ("device", per_lane))]


def count_is_stable(rec):
    return all(abs(c - rec["rne_iterations"]) <= 1 for c in rec["reordered_iterations"])


def jacobi_apply(n, rp, ci, v, max_block_size, nrhs):
    """block-Jacobi as the reference generates and applies it, through the oracle's restatement of it"""
    import oracle_lib
    orc = oracle_lib.load()
    scheme = np.zeros(3, np.int64)
    orc.ref_jacobi_storage_scheme(max_block_size, 32, scheme)
    ptrs = np.zeros(n + 1, np.int32)
    nb = orc.ref_jacobi_find_blocks(n, rp, ci, max_block_size, ptrs)
    blocks = np.zeros(max(int(orc.ref_jacobi_storage_space(scheme, nb)), 1))
    cond = np.zeros(max(nb, 1))
    orc.ref_jacobi_generate(n, rp, ci, v, nb, scheme, ptrs, cond, blocks)

    def apply(vec):
        out = np.zeros_like(vec)
        orc.ref_jacobi_simple_apply(nb, scheme, ptrs, blocks, nrhs, np.ascontiguousarray(vec), nrhs, out, nrhs)
        return out
    return apply


def fixture_from(records):
    """the committed fixture from the driver's arrays (case_arrays) plus what the restatement adds: the iteration
    counts in "rne" mode (sequential sums), which the GPU tests compare the half and integer storages with"""
    fix = {"source": "oracle/ref_driver.cpp, verb cb_gmres, over the reference executor; cases: tests/cb_gmres_util.py "
                     "(SOLVE_CASES with the known-answer systems of reference/test/solver/cb_gmres_kernels.cpp, "
                     "KERNEL_CASES)", "solves": {}, "kernels": {}}
    for name in SOLVE_CASES:
        for storage in STORAGES:
            r = records[f"{name}/{storage}"]
            fix["solves"][f"{name}/{storage}"] = {"x": as_record(r["x"]), "iterations": int(r["iterations"][0]),
                                                 "residual_norm": as_record(r["residual_norm"]),
                                                 "rne_iterations": _rne_iterations(name, storage, 0),
                                                 "reordered_iterations": reordered_counts(name, storage)}
    for name in KERNEL_CASES:
        for storage in STORAGES:
            r = records[f"{name}/{storage}"]
            fix["kernels"][f"{name}/{storage}"] = {k: as_record(v) for k, v in r.items()}
    return fix
