"""IDR(s) in numpy, loop for loop as the reference executor writes it (reference/solver/idr_kernels.cpp) and as
Idr::iterate strings the kernels together (core/solver/idr.cpp:157-290): the yardstick of the IDR tests.

Every function takes 2-D arrays in the reference's layouts (m: s x (s nrhs); g, u: n x (s nrhs), column k nrhs + i
belongs to right-hand side i; p: s x n; f, c: s x nrhs; scalars: length nrhs; stop: one uint8 per column) and works in
place, in the dtype of its arguments: float64 for parity, np.longdouble for the error budget of the re-ordered sums.
Sums over the rows run front to back like the reference's loops (np.cumsum adds sequentially)."""
import numpy as np

ID_MASK = 0x3f


def stopped(stop, i):
    return (int(stop[i]) & ID_MASK) != 0


def seq_dot(a, b):
    """sum_ind a[ind] * b[ind], added in index order"""
    if a.shape[0] == 0:
        return a.dtype.type(0)
    return np.cumsum(a * b)[-1]


def initialize(nrhs, m, p, stop):
    """idr_kernels.cpp:134-189 with deterministic == true: p is used as given"""
    stop[:nrhs] = 0
    for row in range(m.shape[0]):
        for col in range(m.shape[1]):
            m[row, col] = 1.0 if row == col // nrhs else 0.0
    for row in range(p.shape[0]):
        for i in range(row):
            dot = seq_dot(p[row], p[i])
            p[row] -= dot * p[i]
        norm = np.sqrt(seq_dot(p[row], p[row]))
        p[row] /= norm


def solve_lower_triangular(nrhs, m, f, c, stop):
    """idr_kernels.cpp:60-80"""
    for i in range(f.shape[1]):
        if stopped(stop, i):
            continue
        for row in range(m.shape[0]):
            temp = f[row, i]
            for col in range(row):
                temp = temp - m[row, col * nrhs + i] * c[col, i]
            c[row, i] = temp / m[row, row * nrhs + i]


def step_1(nrhs, k, m, f, residual, g, c, v, stop):
    """idr_kernels.cpp:194-219"""
    solve_lower_triangular(nrhs, m, f, c, stop)
    for i in range(nrhs):
        if stopped(stop, i):
            continue
        temp = residual[:, i].copy()
        for j in range(k, m.shape[0]):
            temp -= c[j, i] * g[:, j * nrhs + i]
        v[:, i] = temp


def step_2(nrhs, k, omega, preconditioned_vector, c, u, stop):
    """idr_kernels.cpp:224-244"""
    for i in range(nrhs):
        if stopped(stop, i):
            continue
        temp = omega[i] * preconditioned_vector[:, i]
        for j in range(k, c.shape[0]):
            temp = temp + c[j, i] * u[:, j * nrhs + i]
        u[:, k * nrhs + i] = temp


def update_g_and_u(nrhs, k, p, m, g, g_k, u, stop):
    """idr_kernels.cpp:83-112"""
    for i in range(nrhs):
        if stopped(stop, i):
            continue
        for j in range(k):
            alpha = seq_dot(p[j], g_k[:, i])
            alpha = alpha / m[j, j * nrhs + i]
            g_k[:, i] -= alpha * g[:, j * nrhs + i]
            u[:, k * nrhs + i] -= alpha * u[:, j * nrhs + i]
        g[:, k * nrhs + i] = g_k[:, i]


def step_3(nrhs, k, p, g, g_k, u, m, f, residual, x, stop):
    """idr_kernels.cpp:249-287"""
    update_g_and_u(nrhs, k, p, m, g, g_k, u, stop)
    s = m.shape[0]
    for i in range(nrhs):
        if stopped(stop, i):
            continue
        for j in range(k, s):
            m[j, k * nrhs + i] = seq_dot(p[j], g[:, k * nrhs + i])
        beta = f[k, i] / m[k, k * nrhs + i]
        residual[:, i] -= beta * g[:, k * nrhs + i]
        x[:, i] += beta * u[:, k * nrhs + i]
        if k + 1 < s:
            f[k, i] = 0.0
            for j in range(k + 1, s):
                f[j, i] -= beta * m[j, k * nrhs + i]


def compute_omega(nrhs, kappa, tht, residual_norm, omega, stop):
    """idr_kernels.cpp:292-313"""
    for i in range(nrhs):
        if stopped(stop, i):
            continue
        thr = omega[i]
        normt = np.sqrt(tht[i])
        omega[i] = omega[i] / tht[i]
        absrho = abs(thr / (normt * residual_norm[i]))
        if absrho < kappa:
            omega[i] *= kappa / absrho


def csr_apply(oracle, n, rp, ci, v):
    """x (n x nrhs) -> A x: oracle.ref_csr_spmv in float64, the same row sums in numpy for any other dtype.
    apply.residual(b, x) is b - A x the way core/solver/idr.cpp:172-174 forms it: a copy of b, then the advanced
    apply(-1, x, 1, residual), which starts each row sum at 1 * b and adds (-1 * value) * x term by term."""
    def apply(x):
        if x.dtype == np.float64:
            xin = np.ascontiguousarray(x)
            out = np.zeros_like(xin)
            oracle.ref_csr_spmv(n, x.shape[1], rp, ci, v, xin, x.shape[1], out, x.shape[1])
            return out
        prod = v.astype(x.dtype)[:, None] * x[ci]
        return np.add.reduceat(prod, rp[:-1], axis=0)

    def residual(b, x):
        if x.dtype == np.float64:
            xin = np.ascontiguousarray(x)
            out = np.array(b, np.float64, order="C")
            oracle.ref_csr_advanced_spmv(n, x.shape[1], -1.0, rp, ci, v, xin, x.shape[1], 1.0, out, x.shape[1])
            return out
        out = b.astype(x.dtype) * x.dtype.type(1)
        lens = np.diff(rp)
        for j in range(int(lens.max()) if n else 0):
            rows = np.flatnonzero(lens > j)
            at = rp[rows] + j
            out[rows] += (-v[at]).astype(x.dtype)[:, None] * x[ci[at]]
        return out
    apply.residual = residual
    return apply


def solve(apply, b, p, subspace_dim=2, kappa=0.7, max_iters=1000, reduction=1e-10, precond=None, x=None, literal=False):
    """Idr::iterate (core/solver/idr.cpp:157-290) with Combined(Iteration, ResidualNorm(rhs_norm)).
    literal=True is idr.cpp line for line: the criterion is handed residual_norm, which :273 takes BEFORE the omega
    step (:175 before the first iteration), and Dense::add_scaled at :288-289 moves every column, stopped or not.
    literal=False is what the library's drivers do: the criterion sees the norm of the current residual, so that the
    reported norm is the true one, and a stopped column keeps its x and residual.  Returns
    dict(x, iterations, converged, residual); p is orthonormalised in place."""
    dt = b.dtype
    n, nrhs = b.shape
    s = subspace_dim
    x = np.zeros_like(b) if x is None else x
    precond = precond or (lambda w: w.copy())
    m = np.zeros((s, s * nrhs), dt)
    g = np.zeros((n, s * nrhs), dt)
    u = np.zeros((n, s * nrhs), dt)
    f = np.zeros((s, nrhs), dt)
    c = np.zeros((s, nrhs), dt)
    v = np.zeros((n, nrhs), dt)
    stop = np.zeros(nrhs, np.uint8)
    initialize(nrhs, m, p, stop)
    omega = np.ones(nrhs, dt)
    residual = apply.residual(b, x) if hasattr(apply, "residual") else b - apply(x)         # :172-174
    norm = lambda w: np.sqrt(np.array([seq_dot(w[:, i], w[:, i]) for i in range(nrhs)], dt))
    goal = reduction * norm(b)
    residual_norm = norm(residual)                               # :175
    it = -1
    converged = False
    while True:
        it += 1
        if it >= max_iters:
            break
        stop[(residual_norm if literal else norm(residual)) < goal] = 1
        if stop.all():
            converged = True
            break
        for i in range(nrhs):                                   # f = P^H residual (:221)
            for j in range(s):
                f[j, i] = seq_dot(p[j], residual[:, i])
        for k in range(s):
            step_1(nrhs, k, m, f, residual, g, c, v, stop)
            helper = precond(v)
            step_2(nrhs, k, omega, helper, c, u, stop)
            helper = apply(u[:, k * nrhs:(k + 1) * nrhs])
            step_3(nrhs, k, p, g, helper, u, m, f, residual, x, stop)
        helper = precond(residual)
        t = apply(helper)
        tht = np.zeros(nrhs, dt)
        for i in range(nrhs):
            omega_i = seq_dot(t[:, i], residual[:, i])
            if literal or not stopped(stop, i):
                omega[i] = omega_i
            tht[i] = seq_dot(t[:, i], t[:, i])
        residual_norm = norm(residual)                           # :273
        compute_omega(nrhs, kappa, tht, residual_norm, omega, stop)
        for i in range(nrhs):
            if stopped(stop, i) and not literal:
                continue
            residual[:, i] += omega[i] * -t[:, i]
            x[:, i] += omega[i] * helper[:, i]                    # :289: helper, the preconditioned residual
    return {"x": x, "iterations": it, "converged": converged, "residual": residual}


def subspace(s, n, seed):
    """an s x n matrix P for a solve: normal(0, 1) entries"""
    return np.random.default_rng(seed).standard_normal((s, n))
