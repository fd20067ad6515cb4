"""Thin Python plumbing over the native solver drivers of the C ABI (device
buffers are torch tensors).  Mirrors the factory parameters of
gko::solver::Cg (include/ginkgo/core/solver/cg.hpp) that the hot path uses."""
import ctypes

import numpy as np
import torch

from ._lib import GkomiError
from .formats import Csr, CsrCtx

GKOMI_ENOTSUPPORTED = -2

APPLY_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)
BASELINES = {"rhs_norm": 0, "initial_resnorm": 1, "absolute": 2}


def _check_precond(precond, nrhs):
    """The native preconditioner contexts carry the column count of the vectors they
    are applied to (it is also their stride): a context generated for another count
    would read the n x nrhs row-major vectors as n x ctx.nrhs."""
    ctx = getattr(precond, "ctx", None)
    have = getattr(ctx, "nrhs", None)
    if have is not None and int(have) != int(nrhs):
        raise ValueError(f"preconditioner generated for nrhs = {int(have)}, applied to {int(nrhs)} right-hand sides: "
                         f"pass nrhs={int(nrhs)} to its generate call")


# The frame of every solve function below: operands, workspace, one call of the C ABI, report.

def _operands(n, b, x, *preconds):
    """b as n x nrhs, x (zeros when None) likewise, nrhs; every preconditioner checked against nrhs.  The C ABI
    receives bare pointers and reads them as contiguous n x nrhs vectors, so both must be."""
    b2 = b.reshape(n, -1) if n > 0 else b.reshape(0, b.shape[1] if b.dim() > 1 else 1)
    nrhs = b2.shape[1]
    for p in preconds:
        _check_precond(p, nrhs)
    if x is None:
        x = torch.zeros_like(b2)
    x2 = x.reshape(n, nrhs)
    assert b2.is_contiguous() and x2.is_contiguous()
    return b2, x2, nrhs


def _workspace(nbytes, nrhs, device):
    """the driver's device workspace, its info record (2 + 2 nrhs doubles) and the current stream"""
    return (torch.empty(nbytes, dtype=torch.uint8, device=device), np.zeros(2 + 2 * nrhs, dtype=np.float64),
            torch.cuda.current_stream().cuda_stream)


def _callback(precond):
    """(gkomi_apply_fn, context) of a Preconditioner; (None, None): Identity"""
    return (precond.fn, precond.ctx_ptr) if precond is not None else (None, None)


def _report(info, x2, b, n):
    """the result dict from a driver's info record; x in the shape b came in"""
    res, base = info[2::2].copy(), info[3::2].copy()
    return {"x": x2 if b.dim() > 1 else x2.reshape(n), "iterations": int(info[0]), "converged": bool(info[1]),
            "residual_norm": res, "baseline_norm": base,
            "rel_residual": float(np.max(res / np.where(base == 0, 1.0, base)))}


def cg_solve(gk, n, row_ptrs, col_idxs, vals, b, x=None, max_iters=1000, reduction=1e-10,
             baseline="rhs_norm", mode=1, check_every=16, strategy=0, max_row_nnz=-1,
             precond=None, precond_ctx=None):
    """Cg with Combined(Iteration(max_iters), ResidualNorm(reduction, baseline)).

    b: (n,) or (n, nrhs) float64 device tensor.  precond: None (Identity), a Preconditioner, or an
    integer address / ctypes function pointer of a gkomi_apply_fn with precond_ctx as its context.
    Returns dict(x, iterations, converged, residual_norm, baseline_norm, rel_residual)."""
    b2, x2, nrhs = _operands(n, b, x, precond)
    if mode == 1 and nrhs != 1:
        mode = 0
    nbytes = gk.cg_workspace_bytes(n, nrhs)
    ws, info, stream = _workspace(nbytes, nrhs, b.device)
    if hasattr(precond, "ctx_ptr"):
        pc, precond_ctx = _callback(precond)
    else:
        pc = precond if precond is None or isinstance(precond, int) else ctypes.cast(precond, ctypes.c_void_p).value
    gk.cg_solve_f64_i32(stream, n, nrhs, int(vals.numel()), row_ptrs, col_idxs, vals, strategy, max_row_nnz,
                        pc, precond_ctx, b2, x2, max_iters, reduction, BASELINES[baseline], mode,
                        check_every, ws, nbytes, info)
    return _report(info, x2, b, n)


def krylov_solve(gk, solver, n, row_ptrs, col_idxs, vals, b, x=None, max_iters=1000, reduction=1e-10,
                 baseline="rhs_norm", strategy=0, max_row_nnz=-1, precond=None, check_every=8, fused=False):
    """solver in {"bicgstab", "fcg", "cgs"}: {Bicgstab,Fcg,Cgs}::apply with
    Combined(Iteration(max_iters), ResidualNorm(reduction, baseline)); precond: None or a Preconditioner.
    fused (one right-hand side): the fused driver instead of the reference kernel sequence."""
    assert solver in ("bicgstab", "fcg", "cgs")
    b2, x2, nrhs = _operands(n, b, x, precond)
    assert nrhs == 1 or not fused
    nbytes = gk.krylov_workspace_bytes(n, nrhs)
    ws, info, stream = _workspace(nbytes, nrhs, b.device)
    lead = (stream, n) if fused else (stream, n, nrhs)
    getattr(gk, solver + ("_solve_fused_f64_i32" if fused else "_solve_f64_i32"))(
        *lead, int(vals.numel()), row_ptrs, col_idxs, vals, strategy, max_row_nnz, *_callback(precond), b2, x2,
        max_iters, reduction, BASELINES[baseline], check_every, ws, nbytes, info)
    return _report(info, x2, b, n)


def bicg_solve(gk, n, row_ptrs, col_idxs, vals, b, x=None, max_iters=1000, reduction=1e-10, baseline="rhs_norm",
               strategy=0, max_row_nnz=-1, precond=None, precond_t=None, check_every=8, transposed=None):
    """Bicg::apply: the transposed system matrix is built once here (csr::transpose)
    unless `transposed` = (row_ptrs, col_idxs, vals) is given; precond_t is the
    transposed preconditioner (pass the same object for a symmetric one)."""
    b2, x2, nrhs = _operands(n, b, x, precond, precond_t)
    trp, tci, tv = transposed if transposed is not None else _transpose(gk, n, row_ptrs, col_idxs, vals)
    nbytes = gk.krylov_workspace_bytes(n, nrhs)
    ws, info, stream = _workspace(nbytes, nrhs, b.device)
    gk.bicg_solve_f64_i32(stream, n, nrhs, int(vals.numel()), row_ptrs, col_idxs, vals, trp, tci, tv, strategy,
                          max_row_nnz, *_callback(precond), *_callback(precond_t), b2, x2, max_iters, reduction,
                          BASELINES[baseline], check_every, ws, nbytes, info)
    return _report(info, x2, b, n)


def bicg_solve_op(gk, matrix, matrix_t, b, x=None, max_iters=1000, reduction=1e-10, baseline="rhs_norm", precond=None,
                  precond_t=None, check_every=8):
    """Bicg::apply on a system matrix in any format and its transpose (gkomi.formats objects: a Dense and its
    transpose(), a Csr and its transposed copy): gkomi_bicg_solve_op_f64."""
    n = matrix.nrows
    b2, x2, nrhs = _operands(n, b, x, precond, precond_t)
    cb, cbt = matrix.callback(), matrix_t.callback()
    nbytes = gk.krylov_workspace_bytes(n, nrhs)
    ws, info, stream = _workspace(nbytes, nrhs, b.device)
    gk.bicg_solve_op_f64(stream, n, nrhs, cb.fn, cb.ctx_ptr, cbt.fn, cbt.ctx_ptr, *_callback(precond),
                         *_callback(precond_t), b2, x2, max_iters, reduction, BASELINES[baseline], check_every, ws,
                         nbytes, info)
    return _report(info, x2, b, n)


def ir_solve(gk, n, row_ptrs, col_idxs, vals, b, x=None, relaxation_factor=1.0, inner=None, max_iters=1000,
             reduction=1e-10, baseline="rhs_norm", strategy=0, max_row_nnz=-1):
    """Ir::apply with x as the initial guess; inner: None (Richardson) or a
    Preconditioner-like object whose apply approximates A^-1."""
    b2, x2, nrhs = _operands(n, b, x, inner)
    nbytes = gk.krylov_workspace_bytes(n, nrhs)
    ws, info, stream = _workspace(nbytes, nrhs, b.device)
    gk.ir_solve_f64_i32(stream, n, nrhs, int(vals.numel()), row_ptrs, col_idxs, vals, strategy, max_row_nnz,
                        *_callback(inner), relaxation_factor, b2, x2, max_iters, reduction, BASELINES[baseline], ws,
                        nbytes, info)
    return _report(info, x2, b, n)


def gmres_solve(gk, n, row_ptrs, col_idxs, vals, b, x=None, krylov_dim=100, max_iters=1000, reduction=1e-10,
                baseline="rhs_norm", strategy=0, max_row_nnz=-1, precond=None):
    """Gmres with Combined(Iteration(max_iters), ResidualNorm(reduction, baseline)).
    precond: None or a Preconditioner."""
    b2, x2, nrhs = _operands(n, b, x, precond)
    nbytes = gk.gmres_workspace_bytes(n, nrhs, krylov_dim)
    ws, info, stream = _workspace(nbytes, nrhs, b.device)
    gk.gmres_solve_f64_i32(stream, n, nrhs, int(vals.numel()), row_ptrs, col_idxs, vals, strategy, max_row_nnz,
                           *_callback(precond), b2, x2, krylov_dim, max_iters, reduction, BASELINES[baseline], ws,
                           nbytes, info)
    return _report(info, x2, b, n)


CB_GMRES_STORAGES = {"keep": 0, "reduce1": 1, "reduce2": 2, "integer": 3, "ireduce1": 4, "ireduce2": 5}


def cb_gmres_solve(gk, n, row_ptrs, col_idxs, vals, b, x=None, krylov_dim=100, storage="reduce1", max_iters=1000,
                   reduction=1e-10, baseline="rhs_norm", strategy=0, max_row_nnz=-1, precond=None, matrix=None):
    """CbGmres (GMRES with a compressed Krylov basis) with Combined(Iteration(max_iters), ResidualNorm(reduction,
    baseline)).  storage: solver::cb_gmres::storage_precision by name -- the basis as double, float, half or scaled
    int64 / int32 / int16; all arithmetic stays in double.  precond: None or a Preconditioner.  matrix: a
    gkomi.formats object instead of the CSR arrays.  The result has `forced_resets` besides the usual entries: how often
    a detected convergence was checked by a forced restart with an explicit residual."""
    if storage not in CB_GMRES_STORAGES:
        raise ValueError(f"storage must be one of {sorted(CB_GMRES_STORAGES)}, not {storage!r}")
    if krylov_dim < 1:
        raise ValueError("krylov_dim must be positive")
    st = CB_GMRES_STORAGES[storage]
    b2, x2, nrhs = _operands(n, b, x, precond)
    nbytes = gk.cb_gmres_workspace_bytes(n, nrhs, krylov_dim, st)
    ws, _, stream = _workspace(nbytes, nrhs, b.device)
    info = np.zeros(3 + 2 * nrhs, dtype=np.float64)   # the usual record, then the number of forced resets
    tail = (*_callback(precond), b2, x2, krylov_dim, st, max_iters, reduction, BASELINES[baseline], ws, nbytes, info)
    if matrix is not None:
        cb = matrix.callback()
        gk.cb_gmres_solve_op_f64(stream, n, nrhs, cb.fn, cb.ctx_ptr, *tail)
    else:
        gk.cb_gmres_solve_f64_i32(stream, n, nrhs, int(vals.numel()), row_ptrs, col_idxs, vals, strategy, max_row_nnz,
                                  *tail)
    res = _report(info[:2 + 2 * nrhs], x2, b, n)
    res["forced_resets"] = int(info[2 + 2 * nrhs])
    return res


def ir_mixed(gk, n, row_ptrs, col_idxs, vals, b, x=None, max_iters=100, reduction=1e-12, baseline="rhs_norm",
             inner_max_iters=100, inner_reduction=1e-2, inner_baseline="rhs_norm", relaxation_factor=1.0,
             strategy=0, max_row_nnz=-1):
    """Ir<double> with Cg<float> as its inner solver (mixed-precision iterative refinement), x as the
    initial guess: the outer residual and x stay in double, each correction comes from the fused float
    CG.  vals is the float64 value array; its float copy is made here for this call (one pass over the
    values).  Returns dict(x, iterations, converged, residual_norm, baseline_norm, rel_residual,
    inner_iterations, inner_capped) with float residual_norm / baseline_norm (one right-hand side)."""
    b2, x2, _ = _operands(n, b.reshape(n, 1), x)
    nnz = int(vals.numel())
    stream = torch.cuda.current_stream().cuda_stream
    vals_f32 = torch.empty(nnz, dtype=torch.float32, device=vals.device)
    gk.dense_convert_f64_to_f32(stream, nnz, 1, vals, 1, vals_f32, 1)
    nbytes = gk.ir_mixed_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=b.device)
    info = np.zeros(6, dtype=np.float64)   # this driver's own record: one column and the two inner counts
    gk.ir_mixed_solve_f64_i32(stream, n, 1, nnz, row_ptrs, col_idxs, vals, vals_f32, strategy, max_row_nnz, b2, x2,
                              max_iters, reduction, BASELINES[baseline], inner_max_iters, inner_reduction,
                              BASELINES[inner_baseline], relaxation_factor, ws, nbytes, info)
    res, base = float(info[2]), float(info[3])
    return {"x": x2 if b.dim() > 1 else x2.reshape(n), "iterations": int(info[0]), "converged": bool(info[1]),
            "residual_norm": res, "baseline_norm": base, "rel_residual": res / (base if base != 0 else 1.0),
            "inner_iterations": int(info[4]), "inner_capped": int(info[5])}


IDR_SUBSPACE_SEED = 15


def idr_subspace(subspace_dim, n, device, seed=IDR_SUBSPACE_SEED):
    """The s x n matrix P that idr_solve draws when it is given none: torch.randn under a fixed seed (the library
    itself never draws random numbers; it orthonormalises the rows in place)."""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    return torch.randn((subspace_dim, n), dtype=torch.float64, generator=gen).to(device)


def idr_solve(gk, n, row_ptrs, col_idxs, vals, b, x=None, subspace_dim=2, kappa=0.7, subspace=None, max_iters=1000,
              reduction=1e-10, baseline="rhs_norm", strategy=0, max_row_nnz=-1, precond=None, check_every=8,
              fused=False, matrix=None):
    """Idr::apply with Combined(Iteration(max_iters), ResidualNorm(reduction, baseline)); `iterations` counts outer
    iterations (s + 1 applies of A each).  subspace: None or an s x n float64 device tensor, orthonormalised in place.
    fused (one right-hand side, s <= 8): the driver with 4 s + 2 launches per outer iteration instead of the
    reference kernel sequence.  matrix: a gkomi.formats object instead of the CSR arrays (solve_op)."""
    b2, x2, nrhs = _operands(n, b, x, precond)
    if subspace is None:
        subspace = idr_subspace(subspace_dim, n, b.device)
    assert subspace.dtype == torch.float64 and subspace.is_contiguous() and tuple(subspace.shape) == (subspace_dim, n)
    nbytes = gk.idr_workspace_bytes(n, nrhs, subspace_dim)
    ws, info, stream = _workspace(nbytes, nrhs, b.device)
    tail = (*_callback(precond), subspace_dim, kappa, subspace, b2, x2, max_iters, reduction, BASELINES[baseline],
            check_every, ws, nbytes, info)
    name = "idr_solve_fused" if fused else "idr_solve"
    if matrix is not None:
        cb = matrix.callback()
        getattr(gk, name + "_op_f64")(stream, n, nrhs, cb.fn, cb.ctx_ptr, *tail)
    else:
        getattr(gk, name + "_f64_i32")(stream, n, nrhs, int(vals.numel()), row_ptrs, col_idxs, vals, strategy, max_row_nnz,
                                       *tail)
    return _report(info, x2, b, n)


def solve_op(gk, solver, matrix, b, x=None, max_iters=1000, reduction=1e-10, baseline="rhs_norm", precond=None,
             krylov_dim=100, check_every=8, fused=False, subspace_dim=2, kappa=0.7, subspace=None):
    """Any solver in {"cg", "gmres", "bicgstab", "fcg", "cgs", "idr"} on a system matrix in
    any format (a gkomi.formats object): the *_solve_op_f64 drivers."""
    n = matrix.nrows
    if solver == "idr":
        return idr_solve(gk, n, None, None, None, b, x=x, subspace_dim=subspace_dim, kappa=kappa, subspace=subspace,
                         max_iters=max_iters, reduction=reduction, baseline=baseline, precond=precond,
                         check_every=check_every, fused=fused, matrix=matrix)
    b2, x2, nrhs = _operands(n, b, x, precond)
    cb = matrix.callback()
    # per solver: its workspace size, then the arguments it takes before max_iters and whether it takes check_every
    # (gmres has no fused driver; the fused ones take one right-hand side and no nrhs)
    fused = fused and solver != "gmres"
    assert nrhs == 1 or not fused
    if solver == "gmres":
        nbytes, dim, pace = gk.gmres_workspace_bytes(n, nrhs, krylov_dim), (krylov_dim,), ()
    elif solver == "cg":
        nbytes, dim, pace = gk.cg_workspace_bytes(n, nrhs), (), ((check_every,) if fused else ())
    else:
        nbytes, dim, pace = gk.krylov_workspace_bytes(n, nrhs), (), (check_every,)
    ws, info, stream = _workspace(nbytes, nrhs, b.device)
    lead = (stream, n) if fused else (stream, n, nrhs)
    getattr(gk, solver + ("_solve_fused_op_f64" if fused else "_solve_op_f64"))(
        *lead, cb.fn, cb.ctx_ptr, *_callback(precond), b2, x2, *dim, max_iters, reduction, BASELINES[baseline], *pace,
        ws, nbytes, info)
    return _report(info, x2, b, n)


class JacobiCtx(ctypes.Structure):
    """gkomi_jacobi_ctx (include/gkomi.h)."""
    _fields_ = [("n", ctypes.c_int64), ("nrhs", ctypes.c_int64), ("num_blocks", ctypes.c_int64),
                ("max_block_size", ctypes.c_int32), ("pad_", ctypes.c_int32),
                ("block_ptrs", ctypes.c_void_p), ("blocks", ctypes.c_void_p),
                ("block_precisions", ctypes.c_void_p)]


class IluCtx(ctypes.Structure):
    """gkomi_ilu_ctx (include/gkomi.h)."""
    _fields_ = [("n", ctypes.c_int64), ("nrhs", ctypes.c_int64),
                ("l_row_ptrs", ctypes.c_void_p), ("l_col_idxs", ctypes.c_void_p), ("l_vals", ctypes.c_void_p),
                ("u_row_ptrs", ctypes.c_void_p), ("u_col_idxs", ctypes.c_void_p), ("u_vals", ctypes.c_void_p),
                ("intermediate", ctypes.c_void_p), ("trs_workspace", ctypes.c_void_p),
                ("trs_workspace_bytes", ctypes.c_size_t), ("l_unit_diag", ctypes.c_int32), ("pad_", ctypes.c_int32),
                ("l_plan", ctypes.c_void_p), ("l_nslices", ctypes.c_int64), ("l_entries", ctypes.c_int64),
                ("l_max_deps", ctypes.c_int64),
                ("u_plan", ctypes.c_void_p), ("u_nslices", ctypes.c_int64), ("u_entries", ctypes.c_int64),
                ("u_max_deps", ctypes.c_int64),
                ("l_bricks", ctypes.c_void_p), ("l_bricks_plan", ctypes.c_void_p),
                ("u_bricks", ctypes.c_void_p), ("u_bricks_plan", ctypes.c_void_p)]


class Preconditioner:
    """A native gkomi_apply_fn + its context; keeps the device buffers alive."""

    def __init__(self, gk, name, ctx, keep):
        self.fn = ctypes.cast(getattr(gk._cdll, name), ctypes.c_void_p).value
        self.ctx = ctx
        self.ctx_ptr = ctypes.addressof(ctx)
        self.keep = keep

    def apply(self, b, x):
        """x = M^-1 b through the callback itself (what the solver drivers call); b, x: n x nrhs device tensors"""
        rc = APPLY_FN(self.fn)(self.ctx_ptr, torch.cuda.current_stream().cuda_stream, b.data_ptr(), x.data_ptr())
        if rc != 0:
            raise GkomiError("gkomi_apply_fn", rc, "preconditioner apply failed")
        return x


AUTODETECT = 0xff  # gko::precision_reduction::autodetect()


def jacobi_generate(gk, n, row_ptrs, col_idxs, vals, max_block_size=32, nrhs=1, storage_optimization=None,
                    accuracy=1e-1):
    """preconditioner::Jacobi::generate (core/preconditioner/jacobi.cpp:300-370):
    detect_blocks + generate, or extract/invert the diagonal for max_block_size 1.
    storage_optimization: None (fp64 blocks), a precision_reduction byte for all
    blocks (AUTODETECT = adaptive) or a sequence repeated over the blocks
    (jacobi::initialize_precisions, jacobi_kernels.cpp:485-493)."""
    dv = vals.device
    s = torch.cuda.current_stream().cuda_stream
    if max_block_size == 1:
        diag = torch.zeros(n, dtype=torch.float64, device=dv)
        gk.csr_extract_diagonal_f64_i32(s, n, row_ptrs, col_idxs, vals, diag)
        inv = torch.zeros_like(diag)
        gk.jacobi_invert_diagonal_f64(s, n, diag, inv)
        ctx = JacobiCtx(n, nrhs, n, 1, 0, 0, inv.data_ptr(), 0)
        return Preconditioner(gk, "gkomi_jacobi_apply_cb", ctx, (inv,))
    ptrs = torch.zeros(n + 1, dtype=torch.int32, device=dv)
    nbd = torch.zeros(1, dtype=torch.int64, device=dv)
    nws = gk.jacobi_find_blocks_workspace_bytes(n)
    ws = torch.empty(nws, dtype=torch.uint8, device=dv)
    hn = ctypes.c_int64(0)
    gk.jacobi_find_blocks_i32(s, n, row_ptrs, col_idxs, max_block_size, ptrs, nbd, ws, nws, ctypes.addressof(hn))
    nb = int(hn.value)
    blocks = torch.zeros(max(gk.jacobi_storage_elements(max_block_size, nb), 1), dtype=torch.float64, device=dv)
    prec = cond = None
    if storage_optimization is None:
        gk.jacobi_generate_f64_i32(s, n, row_ptrs, col_idxs, vals, nb, max_block_size, ptrs, None, blocks)
    else:
        src = np.atleast_1d(np.asarray(storage_optimization, np.uint8))
        prec = torch.from_numpy(np.resize(src, max(nb, 1))).to(dv)
        cond = torch.zeros(max(nb, 1), dtype=torch.float64, device=dv)
        gk.jacobi_generate_adaptive_f64_i32(s, n, row_ptrs, col_idxs, vals, nb, max_block_size, ptrs, accuracy,
                                            cond, prec, blocks)
    ctx = JacobiCtx(n, nrhs, nb, max_block_size, 0, ptrs.data_ptr(), blocks.data_ptr(),
                    prec.data_ptr() if prec is not None else 0)
    p = Preconditioner(gk, "gkomi_jacobi_apply_cb", ctx, (ptrs, blocks, prec, cond))
    p.num_blocks, p.block_ptrs, p.blocks, p.block_precisions, p.conditioning = nb, ptrs, blocks, prec, cond
    return p


def jacobi_transpose(gk, pre):
    """Jacobi::transpose (core/preconditioner/jacobi.cpp): the preconditioner of A^T,
    every stored block transposed in its storage precision."""
    if not hasattr(pre, "blocks"):
        return pre   # scalar Jacobi (a diagonal) is its own transpose
    s = torch.cuda.current_stream().cuda_stream
    out = torch.zeros_like(pre.blocks)
    c = pre.ctx
    gk.jacobi_transpose_f64_i32(s, pre.num_blocks, c.max_block_size, pre.block_ptrs, pre.block_precisions, pre.blocks, out)
    ctx = JacobiCtx(c.n, c.nrhs, c.num_blocks, c.max_block_size, 0, pre.block_ptrs.data_ptr(), out.data_ptr(),
                    pre.block_precisions.data_ptr() if pre.block_precisions is not None else 0)
    t = Preconditioner(gk, "gkomi_jacobi_apply_cb", ctx, (pre.block_ptrs, out, pre.block_precisions, pre.conditioning))
    t.num_blocks, t.block_ptrs, t.blocks, t.block_precisions, t.conditioning = (
        pre.num_blocks, pre.block_ptrs, out, pre.block_precisions, pre.conditioning)
    return t


class TrsPlan:
    """solver::LowerTrs / UpperTrs after generate(): the analysed factor
    (gkomi_trs_analyse_{symbolic,numeric}) and its solve."""

    def __init__(self, gk, n, row_ptrs, col_idxs, vals, lower):
        self.gk, self.n, self.lower = gk, int(n), bool(lower)
        self.row_ptrs, self.col_idxs = row_ptrs, col_idxs
        dv = vals.device
        s = torch.cuda.current_stream().cuda_stream
        nb = gk.trs_symbolic_workspace_bytes(n)
        self.symbolic = torch.empty(max(nb, 8), dtype=torch.uint8, device=dv)
        out = (ctypes.c_int64 * 4)()
        gk.trs_analyse_symbolic_i32(s, n, row_ptrs, col_idxs, int(self.lower), self.symbolic, nb, ctypes.addressof(out))
        self.nslices, self.entries, self.nlevels, self.max_deps = (int(v) for v in out)
        self.plan_bytes = gk.trs_plan_bytes(self.nslices, self.entries)
        self.plan = torch.empty(max(self.plan_bytes, 8), dtype=torch.uint8, device=dv)
        self.refresh(vals)

    def refresh(self, vals):
        """new values, same sparsity pattern: numeric phase only"""
        s = torch.cuda.current_stream().cuda_stream
        self.vals = vals
        self.gk.trs_analyse_numeric_f64_i32(s, self.n, self.row_ptrs, self.col_idxs, vals, int(self.lower),
                                            self.symbolic, self.nslices, self.entries, self.nlevels, self.plan,
                                            self.plan_bytes)

    def solve(self, b, x, unit_diag=False):
        s = torch.cuda.current_stream().cuda_stream
        b2, x2 = b.reshape(self.n, -1), x.reshape(self.n, -1)
        self.gk.trs_solve_plan_f64(s, self.n, b2.shape[1], self.plan, self.nslices, self.entries, self.max_deps, int(unit_diag),
                                   b2, b2.stride(0), x2, x2.stride(0))
        return x

    def overrun(self):
        flag = ctypes.c_int(0)
        self.gk.trs_plan_check_overrun(torch.cuda.current_stream().cuda_stream, self.plan, ctypes.addressof(flag))
        return bool(flag.value)


class TrsBricks:
    """solver::LowerTrs / UpperTrs after generate() for factors of grid problems: the brick
    plan (gkomi_trs_bricks_*, csrc/trs_bricks.hip).  Raises GkomiError(GKOMI_ENOTSUPPORTED)
    when the factor is not stencil-shaped; callers then keep TrsPlan."""

    def __init__(self, gk, n, row_ptrs, col_idxs, vals, lower, brick_rows=0, threads=0, mode=0, handle=None):
        self.gk, self.n, self.lower = gk, int(n), bool(lower)
        self.row_ptrs, self.col_idxs = row_ptrs, col_idxs
        self.handle = ctypes.c_void_p(0)
        s = torch.cuda.current_stream().cuda_stream
        if handle is not None:
            self.handle = ctypes.c_void_p(handle)
        else:
            gk.trs_bricks_create_i32(s, n, row_ptrs, col_idxs, int(self.lower), int(brick_rows), int(threads), int(mode),
                                     ctypes.addressof(self.handle))
        self.levels_estimate = int(gk.trs_bricks_levels_estimate(self.handle.value))
        info = (ctypes.c_int64 * 8)()
        gk.trs_bricks_info(self.handle.value, ctypes.addressof(info))
        (self.nbricks, self.coarse_levels, self.nsteps, self.critical_steps, self.lds_bytes, self.width,
         self.threads, self.mode) = (int(v) for v in info)
        self.plan_bytes = gk.trs_bricks_plan_bytes(self.handle.value)
        self.plan = torch.empty(max(self.plan_bytes, 8), dtype=torch.uint8, device=vals.device)
        self.refresh(vals)

    def estimate_us(self, nlevels):
        """critical path of the pipelined solve: one LDS step per level of the factor + a memory hand-off per brick level"""
        return TRS_BRICK_STEP_US * nlevels + TRS_BRICK_HOP_US * self.coarse_levels

    def refresh(self, vals):
        s = torch.cuda.current_stream().cuda_stream
        self.vals = vals
        self.gk.trs_bricks_numeric_f64_i32(s, self.handle.value, self.row_ptrs, self.col_idxs, vals, self.plan,
                                           self.plan_bytes)

    def solve(self, b, x, unit_diag=False):
        s = torch.cuda.current_stream().cuda_stream
        b2, x2 = b.reshape(self.n, -1), x.reshape(self.n, -1)
        self.gk.trs_bricks_solve_f64(s, self.handle.value, self.plan, b2.shape[1], int(unit_diag), b2, b2.stride(0),
                                     x2, x2.stride(0))
        return x

    def overrun(self):
        flag = ctypes.c_int(0)
        self.gk.trs_bricks_check_overrun(torch.cuda.current_stream().cuda_stream, self.plan, ctypes.addressof(flag))
        return bool(flag.value)

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h is not None and h.value:
            self.gk.trs_bricks_destroy(h.value)


# a level must hold this many rows on average for the level-scheduled solve to pay: below it
# (chains, narrow bands) the analysis-free kernel with its in-workgroup LDS hand-offs is faster
TRS_PLAN_MIN_ROWS_PER_LEVEL = 64


# per dependency level of the level plan / per level + per brick level of the pipelined brick plan (us,
# measured on the 108^3 and 1000^2 factors, profiles/r02_trs_bricks.md): what `ilu_from_factors` compares
TRS_LEVEL_US = 1.7
TRS_BRICK_STEP_US = 0.17
TRS_BRICK_HOP_US = 5.0


def ilu_from_factors(gk, n, L, U, nrhs=1, l_unit_diag=False, analyse=True, bricks=True, brick_rows=0):
    """preconditioner::Ilu over given CSR factors L = (row_ptrs, col_idxs, vals), U likewise.
    analyse: LowerTrs / UpperTrs::generate -- the dependency analysis of both factors (True / False / "force");
    a factor of a grid problem gets the brick plan (bricks=True; csrc/trs_bricks.hip), one whose levels are
    wide enough the level-scheduled kernel, a small one (<= 4096 rows) the single-workgroup solve of the same plan,
    anything else keeps the analysis-free solve.
    brick_rows: rows per brick of the brick plan (0: the library's default); bricks="force" takes the
    brick plan whenever the factor admits one, whatever the cost model says.
    The brick analysis runs on the device; a factor that takes the brick plan skips the level analysis (its
    level count is estimated from the box geometry the bricks found)."""
    dv = L[2].device
    inter = torch.zeros((n, nrhs), dtype=torch.float64, device=dv)
    nb = gk.trs_workspace_bytes()
    tws = torch.zeros(nb, dtype=torch.uint8, device=dv)
    plans = [None, None]
    brick_plans = [None, None]
    if analyse and n > 0:
        for i, (f, lower) in enumerate(((L, True), (U, False))):
            bk = None
            if bricks and n >= 2:
                try:
                    bk = TrsBricks(gk, n, f[0], f[1], f[2], lower, brick_rows=brick_rows)
                except GkomiError as e:
                    if e.code != GKOMI_ENOTSUPPORTED:
                        raise
            if bk is not None:
                nlevels = bk.levels_estimate
                # pipelined: about one step per level of the factor
                if nlevels > 16 and (bricks == "force" or gk.trs_prefer_bricks(n, nlevels, bk.coarse_levels)):
                    brick_plans[i] = bk
                    continue
                del bk
            plan = TrsPlan(gk, n, f[0], f[1], f[2], lower)
            # wide levels, or a small factor (one workgroup, x in LDS): gkomi_trs_use_plan, the rule of the shims and the mirror
            if analyse == "force" or gk.trs_use_plan(n, plan.nlevels, plan.max_deps):
                plans[i] = plan
    pl, pu = plans
    bl, bu = brick_plans
    ctx = IluCtx(n, nrhs, L[0].data_ptr(), L[1].data_ptr(), L[2].data_ptr(), U[0].data_ptr(), U[1].data_ptr(),
                 U[2].data_ptr(), inter.data_ptr(), tws.data_ptr(), nb, int(l_unit_diag), 0,
                 pl.plan.data_ptr() if pl else None, pl.nslices if pl else 0, pl.entries if pl else 0,
                 pl.max_deps if pl else -1,
                 pu.plan.data_ptr() if pu else None, pu.nslices if pu else 0, pu.entries if pu else 0,
                 pu.max_deps if pu else -1,
                 bl.handle.value if bl else None, bl.plan.data_ptr() if bl else None,
                 bu.handle.value if bu else None, bu.plan.data_ptr() if bu else None)
    p = Preconditioner(gk, "gkomi_ilu_apply_cb", ctx, (L, U, inter, tws, pl, pu, bl, bu))
    p.l_plan, p.u_plan, p.l_bricks, p.u_bricks = pl, pu, bl, bu
    return p


# ---- the pieces of a factorization's generate, each once -------------------------------------

_CSR = (torch.int32, torch.float64)


def _bytes(nbytes, dv):
    return torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=dv)


def _empty_csr(n, nnz, dv):
    return torch.zeros(nnz, dtype=torch.int32, device=dv), torch.zeros(nnz, dtype=torch.float64, device=dv)


def _count_then_fill(call, counts, dv, dtypes=_CSR, always=False):
    """The two-call idiom of the C ABI.  call(None, ...) writes the row pointers and `counts` (one ctypes.c_int64 per
    output matrix); then one array per dtype is allocated for every count and call(*arrays) fills them, where there is
    something to fill or `always`.  Returns the arrays."""
    call(*[None] * (len(counts) * len(dtypes)))
    arrays = [torch.zeros(int(c.value), dtype=t, device=dv) for c in counts for t in dtypes]
    if always or any(c.value for c in counts):
        call(*arrays)
    return arrays


def _sorted_copy(gk, n, row_ptrs, col_idxs, vals, skip_sorting):
    """working copies of col_idxs and vals, every row sorted by column index unless skipped"""
    ci, v = col_idxs.clone(), vals.clone()
    if not skip_sorting:
        s = torch.cuda.current_stream().cuda_stream
        sorted_flag = ctypes.c_int(0)
        fws = torch.zeros(8, dtype=torch.uint8, device=v.device)
        gk.csr_is_sorted_by_column_index_i32(s, n, row_ptrs, ci, fws, 8, ctypes.addressof(sorted_flag))
        if not sorted_flag.value:
            gk.csr_sort_by_column_index_f64_i32(s, n, row_ptrs, ci, v)
    return ci, v


def _split_l_u(gk, n, rp, ci, v):
    """factorization::initialize_row_ptrs_l_u + initialize_l_u -> (L, U), L with a unit diagonal"""
    s = torch.cuda.current_stream().cuda_stream
    dv = v.device
    lrp = torch.zeros(n + 1, dtype=torch.int32, device=dv)
    urp = torch.zeros(n + 1, dtype=torch.int32, device=dv)
    sb = gk.prefix_sum_workspace_bytes(n + 1)
    sws = _bytes(sb, dv)
    gk.factorization_initialize_row_ptrs_l_u_i32(s, n, rp, ci, lrp, urp, sws, sb)
    lc, lv = _empty_csr(n, int(lrp[n].item()), dv)
    uc, uv = _empty_csr(n, int(urp[n].item()), dv)
    gk.factorization_initialize_l_u_f64_i32(s, n, rp, ci, v, lrp, lc, lv, urp, uc, uv)
    return (lrp, lc, lv), (urp, uc, uv)


def _split_l(gk, n, rp, ci, v, diag_sqrt):
    """factorization::initialize_row_ptrs_l + initialize_l -> L; diag_sqrt: store the root of the diagonal"""
    s = torch.cuda.current_stream().cuda_stream
    dv = v.device
    lrp = torch.zeros(n + 1, dtype=torch.int32, device=dv)
    sb = gk.prefix_sum_workspace_bytes(n + 1)
    sws = _bytes(sb, dv)
    gk.factorization_initialize_row_ptrs_l_i32(s, n, rp, ci, lrp, sws, sb)
    lc, lv = _empty_csr(n, int(lrp[n].item()), dv)
    gk.factorization_initialize_l_f64_i32(s, n, rp, ci, v, lrp, lc, lv, int(diag_sqrt))
    return lrp, lc, lv


class _LevelAnalysis:
    """What FactorizationAnalysis, ParIlutSweep and ParIctSweep share: the workspace one gkomi_*_analyse_i32 call
    fills (.ws, .nbytes) and the six numbers it reports."""

    def _analyse(self, gk, n, dv, nbytes, analyse, *pattern):
        self.gk, self.n, self.nbytes = gk, n, nbytes
        self.ws = torch.zeros(max(nbytes, 8), dtype=torch.uint8, device=dv)
        out = (ctypes.c_int64 * 6)()
        analyse(torch.cuda.current_stream().cuda_stream, n, *pattern, self.ws, nbytes, ctypes.addressof(out))
        self.nlevels, self.longest_row, self.widest_level, self.launches, self.narrow_runs, self.nnz = (int(x) for x in out)


def _with_diagonal(gk, n, row_ptrs, col_idxs, vals):
    """factorization::add_diagonal_elements on a working copy (par_ilu.cpp:93-95)"""
    s = torch.cuda.current_stream().cuda_stream
    dv = vals.device
    rp = row_ptrs.clone()
    nb = gk.factorization_workspace_bytes(n)
    ws = torch.empty(nb, dtype=torch.uint8, device=dv)
    missing = ctypes.c_int64(0)
    gk.factorization_count_missing_diagonal_i32(s, n, n, rp, col_idxs, ws, nb, ctypes.addressof(missing))
    if not missing.value:
        return rp, col_idxs, vals
    nnz = int(vals.numel()) + missing.value
    nc = torch.zeros(nnz, dtype=torch.int32, device=dv)
    nv = torch.zeros(nnz, dtype=torch.float64, device=dv)
    gk.factorization_add_diagonal_elements_f64_i32(s, n, n, rp, col_idxs, vals, nc, nv, ws)
    return rp, nc, nv


def _transpose(gk, n, rp, ci, v):
    s = torch.cuda.current_stream().cuda_stream
    tb = gk.csr_transpose_workspace_bytes(n)
    tws = torch.empty(tb, dtype=torch.uint8, device=v.device)
    trp = torch.zeros(n + 1, dtype=torch.int32, device=v.device)
    tc, tv = torch.zeros_like(ci), torch.zeros_like(v)
    gk.csr_transpose_f64_i32(s, n, n, int(v.numel()), rp, ci, v, trp, tc, tv, tws, tb)
    return trp, tc, tv


def par_ilu_generate(gk, n, row_ptrs, col_idxs, vals, iterations=0, nrhs=1):
    """preconditioner::Ilu over factorization::ParIlu (core/factorization/par_ilu.cpp:74-163):
    returns the Preconditioner (L^-1 then U^-1); .L / .U hold the factors."""
    s = torch.cuda.current_stream().cuda_stream
    dv = vals.device
    rp, ci, v = _with_diagonal(gk, n, row_ptrs, col_idxs, vals)
    nnz = int(v.numel())
    L, U = _split_l_u(gk, n, rp, ci, v)
    utrp, utc, utv = _transpose(gk, n, *U)
    rows = torch.zeros(max(nnz, 1), dtype=torch.int32, device=dv)
    gk.convert_ptrs_to_idxs_i32(s, rp, n, rows)
    gk.par_ilu_compute_l_u_factors_f64_i32(s, iterations, nnz, rows, ci, v, *L, utrp, utc, utv)
    U = _transpose(gk, n, utrp, utc, utv)
    p = ilu_from_factors(gk, n, L, U, nrhs=nrhs)
    p.L, p.U = L, U
    return p


def par_ic_generate(gk, n, row_ptrs, col_idxs, vals, iterations=0, nrhs=1):
    """preconditioner::Ic over factorization::ParIc (core/factorization/par_ic.cpp:70-145):
    L^-1 then L^-T through the triangular solves; .L / .Lt hold the factors."""
    s = torch.cuda.current_stream().cuda_stream
    dv = vals.device
    lrp, lc, lv = _split_l(gk, n, *_with_diagonal(gk, n, row_ptrs, col_idxs, vals), diag_sqrt=False)
    lnnz = int(lv.numel())
    a_vals = lv.clone()
    rows = torch.zeros(max(lnnz, 1), dtype=torch.int32, device=dv)
    gk.convert_ptrs_to_idxs_i32(s, lrp, n, rows)
    gk.par_ic_init_factor_f64_i32(s, n, lrp, lc, lv)
    gk.par_ic_compute_factor_f64_i32(s, iterations, lnnz, rows, a_vals, lrp, lc, lv)
    Lt = _transpose(gk, n, lrp, lc, lv)
    p = ilu_from_factors(gk, n, (lrp, lc, lv), Lt, nrhs=nrhs)
    p.L, p.Lt = (lrp, lc, lv), Lt
    return p


# ---- ParILUT (core/factorization/par_ilut.cpp:190-344) -----------------------------------------------------

def par_ilut_spgemm(gk, n, a, b):
    """csr::spgemm of two n x n matrices (row_ptrs, col_idxs, vals)"""
    s = torch.cuda.current_stream().cuda_stream
    dv = a[2].device
    nb = gk.csr_spgemm_workspace_bytes(n, n)
    ws = _bytes(nb, dv)
    crp = torch.zeros(n + 1, dtype=torch.int32, device=dv)
    cnnz = ctypes.c_int64(0)

    def call(cc, cv):
        gk.csr_spgemm_f64_i32(s, n, n, int(a[2].numel()), a[0], a[1], a[2], n, n, int(b[2].numel()), b[0], b[1], b[2],
                              None, None, 0, 0, 0, None, None, None, crp, cc, cv, ctypes.addressof(cnnz), ws, nb)
    return (crp, *_count_then_fill(call, [cnnz], dv))


def par_ilut_add_candidates(gk, n, lu, a, l, u):
    """par_ilut_factorization::add_candidates -> (L', U')"""
    s = torch.cuda.current_stream().cuda_stream
    dv = a[2].device
    nb = gk.par_ilut_add_candidates_workspace_bytes(n)
    ws = _bytes(nb, dv)
    lrp = torch.zeros(n + 1, dtype=torch.int32, device=dv)
    urp = torch.zeros(n + 1, dtype=torch.int32, device=dv)
    lnnz, unnz = ctypes.c_int64(0), ctypes.c_int64(0)

    def call(lc, lv, uc, uv):
        gk.par_ilut_add_candidates_f64_i32(s, n, *lu, *a, *l, *u, lrp, lc, lv, urp, uc, uv, ctypes.addressof(lnnz),
                                           ctypes.addressof(unnz), ws, nb)
    lc, lv, uc, uv = _count_then_fill(call, [lnnz, unnz], dv, always=n > 0)
    return (lrp, lc, lv), (urp, uc, uv)


def par_ilut_threshold_select(gk, vals, rank):
    """par_ilut_factorization::threshold_select: the magnitude of rank `rank` among vals"""
    nnz = int(vals.numel())
    nb = gk.par_ilut_select_workspace_bytes(nnz)
    ws = _bytes(nb, vals.device)
    out = ctypes.c_double(0.0)
    gk.par_ilut_threshold_select_f64(torch.cuda.current_stream().cuda_stream, nnz, vals, rank, ws, nb, ctypes.addressof(out))
    return out.value


def par_ilut_threshold_approx(gk, vals, rank):
    """the threshold of par_ilut_factorization::threshold_filter_approx"""
    nnz = int(vals.numel())
    nb = gk.par_ilut_approx_workspace_bytes()
    ws = _bytes(nb, vals.device)
    out = ctypes.c_double(0.0)
    gk.par_ilut_threshold_approx_f64(torch.cuda.current_stream().cuda_stream, nnz, vals, rank, ws, nb, ctypes.addressof(out))
    return out.value


def _threshold(gk, vals, nnz_limit, approximate_select):
    """the magnitude below which entries of a candidate factor are dropped so that about nnz_limit remain"""
    rank = max(0, int(vals.numel()) - nnz_limit - 1)
    return (par_ilut_threshold_approx if approximate_select else par_ilut_threshold_select)(gk, vals, rank)


def par_ilut_threshold_filter(gk, n, m, threshold, with_coo=False):
    """par_ilut_factorization::threshold_filter -> (row_ptrs, col_idxs, vals) [, COO row indices]"""
    s = torch.cuda.current_stream().cuda_stream
    dv = m[2].device
    nb = gk.par_ilut_filter_workspace_bytes(n)
    ws = _bytes(nb, dv)
    nrp = torch.zeros(n + 1, dtype=torch.int32, device=dv)
    nnz = ctypes.c_int64(0)

    def call(nc, nv, rows=None):
        gk.par_ilut_threshold_filter_f64_i32(s, n, *m, threshold, nrp, nc, nv, rows, ctypes.addressof(nnz), ws, nb)
    nc, nv, *rows = _count_then_fill(call, [nnz], dv, dtypes=_CSR + (torch.int32,) if with_coo else _CSR)
    return ((nrp, nc, nv), rows[0]) if with_coo else (nrp, nc, nv)


class ParIlutSweep(_LevelAnalysis):
    """gkomi_par_ilut_analyse_i32 of one pair of patterns (L', U'); .compute runs the exact sweep
    (par_ilut_factorization::compute_l_u_factors with the reference executor's result) in place."""

    def __init__(self, gk, n, l, u):
        self.l, self.u = l, u
        self.l_nnz, self.u_nnz = int(l[2].numel()), int(u[2].numel())
        self._analyse(gk, n, l[2].device, gk.par_ilut_sweep_workspace_bytes(n, self.l_nnz, self.u_nnz),
                      gk.par_ilut_analyse_i32, self.l_nnz, l[0], l[1], self.u_nnz, u[0], u[1])

    def compute(self, a, u_csc=None):
        """u_csc: the CSC copy of U, whose values are brought up to date"""
        ut = u_csc if u_csc is not None else (None, None, None)
        self.gk.par_ilut_compute_l_u_factors_f64_i32(torch.cuda.current_stream().cuda_stream, self.n, *a, self.l_nnz, *self.l,
                                                     self.u_nnz, *self.u, *ut, self.ws, self.nbytes)


def _check_threshold_generate(who, n, row_ptrs, ncols, fill_in_limit):
    """GKO_ASSERT_IS_SQUARE_MATRIX and the fill_in_limit check, before anything reaches the device"""
    if ncols is not None and ncols != n:
        raise ValueError(f"{who} needs a square matrix, got {n} x {ncols}")
    if int(row_ptrs.numel()) != n + 1:
        raise ValueError(f"{who} needs a square matrix: {int(row_ptrs.numel()) - 1} rows of row pointers for n = {n}")
    if not fill_in_limit > 0.0:
        raise ValueError(f"fill_in_limit must be positive, got {fill_in_limit}")


def par_ilut_generate(gk, n, row_ptrs, col_idxs, vals, iterations=5, fill_in_limit=2.0, approximate_select=True,
                      skip_sorting=False, nrhs=1, ncols=None):
    """preconditioner::Ilu over factorization::ParIlut (core/factorization/par_ilut.cpp:190-344), with the factors of the
    reference executor bit for bit: sort, initialize_l_u, then per iteration spgemm, add_candidates, transpose, sweep,
    threshold selection and filters, sweep.  Returns the Preconditioner; .L / .U hold the factors, .levels the number of
    dependency levels of every sweep.
    The CSC copy of U' exists only where its order matters: the approximate selection samples it.  The exact
    selection does not depend on the order of the values, and the second sweep reads U by rows."""
    _check_threshold_generate("ParIlut", n, row_ptrs, ncols, fill_in_limit)
    a = (row_ptrs, *_sorted_copy(gk, n, row_ptrs, col_idxs, vals, skip_sorting))
    l, u = _split_l_u(gk, n, *a)
    l_nnz_limit, u_nnz_limit = int(int(l[2].numel()) * fill_in_limit), int(int(u[2].numel()) * fill_in_limit)
    levels = []
    for _ in range(iterations):
        lu = par_ilut_spgemm(gk, n, l, u)
        l_new, u_new = par_ilut_add_candidates(gk, n, lu, a, l, u)
        u_new_csc = _transpose(gk, n, *u_new) if approximate_select else None
        sweep = ParIlutSweep(gk, n, l_new, u_new)
        sweep.compute(a, u_new_csc)
        levels.append(sweep.nlevels)
        l_threshold = _threshold(gk, l_new[2], l_nnz_limit, approximate_select)
        u_threshold = _threshold(gk, (u_new_csc if approximate_select else u_new)[2], u_nnz_limit, approximate_select)
        l = par_ilut_threshold_filter(gk, n, l_new, l_threshold)
        u = par_ilut_threshold_filter(gk, n, u_new, u_threshold)
        sweep = ParIlutSweep(gk, n, l, u)
        sweep.compute(a)
        levels.append(sweep.nlevels)
    p = ilu_from_factors(gk, n, l, u, nrhs=nrhs)
    p.L, p.U, p.levels = l, u, levels
    return p


# ---- ParICT (core/factorization/par_ict.cpp:174-292) --------------------------------------------------------

def par_ict_add_candidates(gk, n, llh, a, l):
    """par_ict_factorization::add_candidates -> L'"""
    s = torch.cuda.current_stream().cuda_stream
    dv = a[2].device
    nb = gk.par_ict_add_candidates_workspace_bytes(n)
    ws = _bytes(nb, dv)
    lrp = torch.zeros(n + 1, dtype=torch.int32, device=dv)
    lnnz = ctypes.c_int64(0)

    def call(lc, lv):
        gk.par_ict_add_candidates_f64_i32(s, n, *llh, *a, *l, lrp, lc, lv, ctypes.addressof(lnnz), ws, nb)
    return (lrp, *_count_then_fill(call, [lnnz], dv, always=n > 0))


class ParIctSweep(_LevelAnalysis):
    """gkomi_par_ict_analyse_i32 of one pattern L'; .compute runs the exact sweep
    (par_ict_factorization::compute_factor with the reference executor's result) in place."""

    def __init__(self, gk, n, l):
        self.l = l
        self.l_nnz = int(l[2].numel())
        self._analyse(gk, n, l[2].device, gk.par_ict_sweep_workspace_bytes(n, self.l_nnz), gk.par_ict_analyse_i32,
                      self.l_nnz, l[0], l[1])

    def compute(self, a):
        self.gk.par_ict_compute_factor_f64_i32(torch.cuda.current_stream().cuda_stream, self.n, *a, self.l_nnz, *self.l,
                                               self.ws, self.nbytes)


def par_ict_generate(gk, n, row_ptrs, col_idxs, vals, iterations=5, fill_in_limit=2.0, approximate_select=True,
                     skip_sorting=False, nrhs=1, ncols=None):
    """preconditioner::Ic over factorization::ParIct (core/factorization/par_ict.cpp:174-292), with the factor of the
    reference executor bit for bit: sort, initialize_l with the root of the diagonal, then per iteration spgemm(L, L^T),
    add_candidates, sweep, threshold selection on L' in CSR order and filter, sweep, transpose.  Returns the
    Preconditioner (L^-1 then L^-T); .L / .Lt hold the factors, .levels the number of dependency levels of every sweep."""
    _check_threshold_generate("ParIct", n, row_ptrs, ncols, fill_in_limit)
    a = (row_ptrs, *_sorted_copy(gk, n, row_ptrs, col_idxs, vals, skip_sorting))
    l = _split_l(gk, n, *a, diag_sqrt=True)
    lt = _transpose(gk, n, *l)
    l_nnz_limit = int(int(l[2].numel()) * fill_in_limit)
    levels = []
    for _ in range(iterations):
        llh = par_ilut_spgemm(gk, n, l, lt)
        l_new = par_ict_add_candidates(gk, n, llh, a, l)
        sweep = ParIctSweep(gk, n, l_new)
        sweep.compute(a)
        levels.append(sweep.nlevels)
        l = par_ilut_threshold_filter(gk, n, l_new, _threshold(gk, l_new[2], l_nnz_limit, approximate_select))
        sweep = ParIctSweep(gk, n, l)
        sweep.compute(a)
        levels.append(sweep.nlevels)
        lt = _transpose(gk, n, *l)
    p = ilu_from_factors(gk, n, l, lt, nrhs=nrhs)
    p.L, p.Lt, p.levels = l, lt, levels
    return p


class FactorizationAnalysis(_LevelAnalysis):
    """gkomi_ilu_analyse_i32: diagonal positions, dependency levels and the launch list of the exact ILU(0) / IC(0)
    of one sparsity pattern (sorted rows, diagonal stored); reusable for any number of numeric calls."""

    def __init__(self, gk, n, row_ptrs, col_idxs):
        self._analyse(gk, n, row_ptrs.device, gk.ilu_analysis_workspace_bytes(n), gk.ilu_analyse_i32, row_ptrs, col_idxs)

    def compute_lu(self, row_ptrs, col_idxs, vals):
        self.gk.ilu_compute_lu_f64_i32(torch.cuda.current_stream().cuda_stream, self.n, row_ptrs, col_idxs, vals,
                                       self.ws, self.nbytes)

    def ic_compute(self, row_ptrs, col_idxs, vals):
        self.gk.ic_compute_f64_i32(torch.cuda.current_stream().cuda_stream, self.n, row_ptrs, col_idxs, vals, self.ws,
                                   self.nbytes)


def _exact_working_copy(gk, n, row_ptrs, col_idxs, vals, skip_sorting):
    """sort_by_column_index unless skipped, then add_diagonal_elements, on a working copy (core/factorization/ilu.cpp:80-86),
    and its level analysis"""
    rp, ci, v = _with_diagonal(gk, n, row_ptrs, *_sorted_copy(gk, n, row_ptrs, col_idxs, vals, skip_sorting))
    return rp, ci, v, FactorizationAnalysis(gk, n, rp, ci)


def ilu_generate(gk, n, row_ptrs, col_idxs, vals, nrhs=1, skip_sorting=False):
    """preconditioner::Ilu over factorization::Ilu, the exact ILU(0) (core/factorization/ilu.cpp:67-124): sort,
    add_diagonal_elements, compute_lu, initialize_l_u.  .L / .U hold the factors, .analysis the level analysis."""
    rp, ci, v, an = _exact_working_copy(gk, n, row_ptrs, col_idxs, vals, skip_sorting)
    an.compute_lu(rp, ci, v)
    L, U = _split_l_u(gk, n, rp, ci, v)
    p = ilu_from_factors(gk, n, L, U, nrhs=nrhs)
    p.L, p.U, p.analysis = L, U, an
    return p


def ic_generate(gk, n, row_ptrs, col_idxs, vals, nrhs=1, skip_sorting=False):
    """preconditioner::Ic over factorization::Ic, the exact IC(0) (core/factorization/ic.cpp:67-120): sort,
    add_diagonal_elements, compute, initialize_l, L^T.  .L / .Lt hold the factors."""
    rp, ci, v, an = _exact_working_copy(gk, n, row_ptrs, col_idxs, vals, skip_sorting)
    an.ic_compute(rp, ci, v)
    L = _split_l(gk, n, rp, ci, v, diag_sqrt=False)
    Lt = _transpose(gk, n, *L)
    p = ilu_from_factors(gk, n, L, Lt, nrhs=nrhs)
    p.L, p.Lt, p.analysis = L, Lt, an
    return p


# ---- ISAI (core/preconditioner/isai.cpp:87-265) ----------------------------------------------------------------

ISAI_KINDS = ("lower", "upper", "general", "spd")


class IsaiCtx(ctypes.Structure):
    """gkomi_isai_ctx (include/gkomi.h)."""
    _fields_ = [("n", ctypes.c_int64), ("nrhs", ctypes.c_int64), ("num_matrices", ctypes.c_int64),
                ("first", CsrCtx), ("second", CsrCtx), ("intermediate", ctypes.c_void_p)]


def _check_isai(kind, n, row_ptrs, ncols, sparsity_power, excess_limit):
    """GKO_ASSERT_IS_SQUARE_MATRIX and the parameter checks, before anything reaches the device"""
    if kind not in ISAI_KINDS:
        raise ValueError(f"unknown isai kind {kind!r}: one of {', '.join(ISAI_KINDS)}")
    if int(sparsity_power) != sparsity_power or sparsity_power < 1:
        raise ValueError(f"sparsity_power must be an integer >= 1, got {sparsity_power}")
    if int(excess_limit) != excess_limit or excess_limit < 0:
        raise ValueError(f"excess_limit must be an integer >= 0, got {excess_limit}")
    if ncols is not None and ncols != n:
        raise ValueError(f"Isai needs a square matrix, got {n} x {ncols}")
    if int(row_ptrs.numel()) != n + 1:
        raise ValueError(f"Isai needs a square matrix: {int(row_ptrs.numel()) - 1} rows of row pointers for n = {n}")


def isai_extend_sparsity(gk, n, m, power):
    """extend_sparsity (isai.cpp:87-118): m^power by square-and-multiply through csr::spgemm, as it is written there"""
    if power == 1:
        return m[0].clone(), m[1].clone(), m[2].clone()
    id_power, acc = m, m
    i = power - 1
    while i > 1:
        if i % 2 != 0:
            acc = par_ilut_spgemm(gk, n, id_power, acc)
            i -= 1
        id_power = par_ilut_spgemm(gk, n, id_power, id_power)
        i //= 2
    return par_ilut_spgemm(gk, n, id_power, acc)


def isai_generate_kernel(gk, kind, n, m, inverse):
    """isai::generate_tri_inverse / generate_general_inverse on a pattern: fills the values of the short rows of
    `inverse` in place -> (excess_rhs_ptrs, excess_nz_ptrs), device int32 arrays of n + 1 entries"""
    s = torch.cuda.current_stream().cuda_stream
    dv = m[2].device
    rhs_ptrs = torch.zeros(n + 1, dtype=torch.int32, device=dv)
    nz_ptrs = torch.zeros(n + 1, dtype=torch.int32, device=dv)
    nb = gk.isai_generate_workspace_bytes(n)
    ws = _bytes(nb, dv)
    if kind in ("lower", "upper"):
        gk.isai_generate_tri_inverse_f64_i32(s, n, *m, *inverse, rhs_ptrs, nz_ptrs, int(kind == "lower"), ws, nb)
    else:
        gk.isai_generate_general_inverse_f64_i32(s, n, *m, *inverse, rhs_ptrs, nz_ptrs, int(kind == "spd"), ws, nb)
    return rhs_ptrs, nz_ptrs


def isai_excess_system(gk, n, m, inverse, rhs_ptrs, nz_ptrs, e_dim, e_nnz, e_start, e_end):
    """isai::generate_excess_system -> ((row_ptrs, col_idxs, vals), rhs)"""
    s = torch.cuda.current_stream().cuda_stream
    dv = m[2].device
    erp = torch.zeros(e_dim + 1, dtype=torch.int32, device=dv)
    ec, ev = _empty_csr(e_dim, e_nnz, dv)
    rhs = torch.zeros(e_dim, dtype=torch.float64, device=dv)
    gk.isai_generate_excess_system_f64_i32(s, n, *m, inverse[0], inverse[1], rhs_ptrs, nz_ptrs, e_dim, e_nnz, erp, ec, ev,
                                           rhs, e_start, e_end)
    return (erp, ec, ev), rhs


def isai_gmres_excess_solver(gk, e_dim, system, rhs, x):
    """The reference's default for general and spd (isai.cpp:230-244): GMRES with block-Jacobi(32), at most e_dim
    iterations, residual reduction 1e-6 against the norm of the rhs; x comes in as the initial guess."""
    pre = jacobi_generate(gk, e_dim, *system, max_block_size=32)
    gmres_solve(gk, e_dim, *system, rhs, x=x, max_iters=e_dim, reduction=1e-6, baseline="rhs_norm", precond=pre)
    return x


def _isai_trs_excess_solver(lower):
    def solve(gk, e_dim, system, rhs, x):
        s = torch.cuda.current_stream().cuda_stream
        nb = gk.trs_workspace_bytes()
        ws = torch.zeros(nb, dtype=torch.uint8, device=rhs.device)
        (gk.lower_trs_solve_f64_i32 if lower else gk.upper_trs_solve_f64_i32)(s, e_dim, 1, *system, 0, rhs, 1, x, 1, ws, nb)
        return x
    return solve


def isai_generate(gk, kind, n, row_ptrs, col_idxs, vals, sparsity_power=1, excess_limit=0, skip_sorting=False,
                  excess_solver=None, ncols=None, trace=None):
    """Isai::generate_inverse (core/preconditioner/isai.cpp:121-265) for kind in "lower", "upper", "general", "spd":
    a sorted copy, for spd its lower part (initialize_l, diag_sqrt = false), the sparsity power, the generate kernel,
    then the long rows block by block over excess_limit (0: one block): excess system, transpose, solve -- UpperTrs for
    lower, LowerTrs for upper, GMRES with block-Jacobi(32) for general and spd, or excess_solver(gk, dim, system, rhs,
    x) -- scale (spd) and scatter.  Returns the inverse as CSR; for spd (L, L^T).
    trace: a dict that receives the prefix arrays (host) and the (start, end) of every block."""
    _check_isai(kind, n, row_ptrs, ncols, sparsity_power, excess_limit)
    s = torch.cuda.current_stream().cuda_stream
    to_invert = (row_ptrs, *_sorted_copy(gk, n, row_ptrs, col_idxs, vals, skip_sorting))
    if kind != "spd":
        inverted = isai_extend_sparsity(gk, n, to_invert, sparsity_power)
    else:
        base = _split_l(gk, n, *to_invert, diag_sqrt=False)
        inverted = base if sparsity_power == 1 else isai_extend_sparsity(gk, n, base, sparsity_power)
    rhs_ptrs, nz_ptrs = isai_generate_kernel(gk, kind, n, to_invert, inverted)
    host_rhs_ptrs, host_nz_ptrs = rhs_ptrs.cpu().numpy(), nz_ptrs.cpu().numpy()
    total = int(host_rhs_ptrs[n])
    lim = total if excess_limit == 0 else int(excess_limit)
    if trace is not None:
        trace.update(excess_rhs_ptrs=host_rhs_ptrs, excess_nz_ptrs=host_nz_ptrs, blocks=[])
    if excess_solver is None:
        excess_solver = (isai_gmres_excess_solver if kind in ("general", "spd") else _isai_trs_excess_solver(kind == "upper"))
    block = 0
    while total > 0 and block < n:
        start = block
        e_dim = 0
        while e_dim < lim and block < n:
            block += 1
            e_dim = int(host_rhs_ptrs[block] - host_rhs_ptrs[start])
        if e_dim == 0:
            break
        e_nnz = int(host_nz_ptrs[block] - host_nz_ptrs[start])
        system, rhs = isai_excess_system(gk, n, to_invert, inverted, rhs_ptrs, nz_ptrs, e_dim, e_nnz, start, block)
        tws = _bytes(gk.csr_transpose_workspace_bytes(e_dim), rhs.device)
        trp = torch.zeros(e_dim + 1, dtype=torch.int32, device=rhs.device)
        tc, tv = torch.zeros_like(system[1]), torch.zeros_like(system[2])
        gk.csr_transpose_f64_i32(s, e_dim, e_dim, e_nnz, *system, trp, tc, tv, tws, int(tws.numel()))
        solution = excess_solver(gk, e_dim, (trp, tc, tv), rhs, rhs.clone())
        if kind == "spd":
            gk.isai_scale_excess_solution_f64_i32(s, n, rhs_ptrs, solution, start, block)
        gk.isai_scatter_excess_solution_f64_i32(s, n, rhs_ptrs, solution, inverted[0], inverted[2], start, block)
        if trace is not None:
            trace["blocks"].append((start, block))
    if kind == "spd":
        return inverted, _transpose(gk, n, *inverted)
    return inverted


def _isai_csr_ctx(gk, n, m, keep):
    """the gkomi_csr_ctx of an inverse, with its srow and its longest row"""
    c = Csr(gk, n, n, *m)
    keep.append(c)
    return c.callback().ctx


def isai_from_inverses(gk, n, first, second=None, nrhs=1):
    """The Preconditioner over gkomi_isai_apply_cb: x = first b, or x = second (first b)."""
    keep = [first, second]
    c1 = _isai_csr_ctx(gk, n, first, keep)
    c2 = _isai_csr_ctx(gk, n, second, keep) if second is not None else type(c1)()
    inter = torch.zeros((n, nrhs), dtype=torch.float64, device=first[2].device) if second is not None else None
    keep.append(inter)
    ctx = IsaiCtx(n, nrhs, 1 if second is None else 2, c1, c2, inter.data_ptr() if inter is not None else None)
    p = Preconditioner(gk, "gkomi_isai_apply_cb", ctx, keep)
    p.inverses = (first,) if second is None else (first, second)
    return p


def isai_preconditioner(gk, kind, n, row_ptrs, col_idxs, vals, sparsity_power=1, excess_limit=0, skip_sorting=False,
                        nrhs=1, excess_solver=None):
    """preconditioner::Isai<kind>::generate: LowerIsai / UpperIsai / GeneralIsai apply one SpMV, SpdIsai two (L, L^T)"""
    inv = isai_generate(gk, kind, n, row_ptrs, col_idxs, vals, sparsity_power, excess_limit, skip_sorting, excess_solver)
    return isai_from_inverses(gk, n, *inv, nrhs=nrhs) if kind == "spd" else isai_from_inverses(gk, n, inv, nrhs=nrhs)


def ilu_isai_from_factors(gk, n, L, U, sparsity_power=1, excess_limit=0, skip_sorting=False, nrhs=1):
    """preconditioner::Ilu (or Ic, with U = L^T) with LowerIsai and UpperIsai as its solvers: x = U^-1 (L^-1 b) as two
    SpMVs.  .l_inverse / .u_inverse hold the approximate inverses."""
    for f in (L, U):
        _check_isai("lower", n, f[0], None, sparsity_power, excess_limit)
    li = isai_generate(gk, "lower", n, *L, sparsity_power, excess_limit, skip_sorting)
    ui = isai_generate(gk, "upper", n, *U, sparsity_power, excess_limit, skip_sorting)
    p = isai_from_inverses(gk, n, li, ui, nrhs=nrhs)
    p.l_inverse, p.u_inverse = li, ui
    return p


def ic_isai_from_factor(gk, n, L, sparsity_power=1, excess_limit=0, skip_sorting=False, nrhs=1):
    """preconditioner::Ic with LowerIsai as its solver: the second solver is the transpose of the first (ic.hpp:327-328),
    not an UpperIsai of L^T -- the two differ, and only this one keeps the preconditioner symmetric for CG.
    .l_inverse / .u_inverse hold the approximate inverse and its transpose."""
    _check_isai("lower", n, L[0], None, sparsity_power, excess_limit)
    li = isai_generate(gk, "lower", n, *L, sparsity_power, excess_limit, skip_sorting)
    ui = _transpose(gk, n, *li)
    p = isai_from_inverses(gk, n, li, ui, nrhs=nrhs)
    p.l_inverse, p.u_inverse = li, ui
    return p


# ---- sparse direct solver: symbolic Cholesky, Lu, Direct ------------------------------------------------

FOREST_FIELDS = ("parents", "child_ptrs", "children", "postorder", "inv_postorder", "postorder_parents")


def elimination_forest(gk, n, row_ptrs, col_idxs):
    """factorization::compute_elim_forest (core/factorization/elimination_forest.cpp:183-207) of a device CSR pattern:
    dict of the six int32 device arrays (child_ptrs has n + 2 entries, the pseudo-root is n).  Host work, blocking."""
    dv = row_ptrs.device
    out = {k: torch.zeros(n + 2 if k == "child_ptrs" else max(n, 1), dtype=torch.int32, device=dv) for k in FOREST_FIELDS}
    gk.elimination_forest_i32(torch.cuda.current_stream().cuda_stream, n, row_ptrs, col_idxs,
                              *(out[k] for k in FOREST_FIELDS))
    return {k: (v if k == "child_ptrs" else v[:n]) for k, v in out.items()}


def symbolic_cholesky(gk, n, row_ptrs, col_idxs, forest=None):
    """factorization::symbolic_cholesky (core/factorization/symbolic.cpp:66-93): count, prefix sum, factorize, sort,
    transpose, spgeam.  Returns (L, combined), each (row_ptrs, col_idxs, vals): the sorted pattern of the Cholesky
    factor and the pattern of L + L^T; the values these steps drag along are zeros."""
    s = torch.cuda.current_stream().cuda_stream
    dv = row_ptrs.device
    nnz = int(col_idxs.numel())
    if forest is None:
        forest = elimination_forest(gk, n, row_ptrs, col_idxs)
    nb = gk.cholesky_symbolic_workspace_bytes(n, nnz)
    ws = torch.empty(max(nb, 8), dtype=torch.uint8, device=dv)
    lrp = torch.zeros(n + 1, dtype=torch.int32, device=dv)
    factor_nnz = ctypes.c_int64(0)
    gk.cholesky_symbolic_count_i32(s, n, nnz, row_ptrs, col_idxs, forest["inv_postorder"], forest["postorder_parents"],
                                   lrp, ws, nb, ctypes.addressof(factor_nnz))
    sb = gk.prefix_sum_workspace_bytes(n + 1)
    sws = torch.empty(max(sb, 8), dtype=torch.uint8, device=dv)
    gk.prefix_sum_i32(s, lrp, n + 1, sws, sb)
    lnnz = int(factor_nnz.value)
    lc = torch.zeros(lnnz, dtype=torch.int32, device=dv)
    lv = torch.zeros(lnnz, dtype=torch.float64, device=dv)
    gk.cholesky_symbolic_factorize_i32(s, n, nnz, row_ptrs, col_idxs, forest["postorder"], forest["inv_postorder"],
                                       forest["postorder_parents"], lrp, lc, ws, nb)
    gk.csr_sort_by_column_index_f64_i32(s, n, lrp, lc, lv)
    trp, tc, tv = _transpose(gk, n, lrp, lc, lv)
    # L^T->apply(one, Identity, one, L): L becomes 1 * L^T + 1 * L
    one = torch.ones(1, dtype=torch.float64, device=dv)
    gb = gk.csr_spgeam_workspace_bytes(n)
    gws = torch.empty(max(gb, 8), dtype=torch.uint8, device=dv)
    crp = torch.zeros(n + 1, dtype=torch.int32, device=dv)
    cnnz = ctypes.c_int64(0)

    def spgeam(cc, cv):
        gk.csr_spgeam_f64_i32(s, n, n, one, lnnz, trp, tc, tv, one, n, n, lnnz, lrp, lc, lv, crp, cc, cv,
                              ctypes.addressof(cnnz), gws, gb)
    cc, cv = _count_then_fill(spgeam, [cnnz], dv)
    return (lrp, lc, lv), (crp, cc, cv)


class LuFactorization:
    """experimental::factorization::Factorization in its combined_lu storage (what Lu::generate returns,
    core/factorization/lu.cpp:144): .combined = (row_ptrs, col_idxs, vals) holds L below the diagonal (its unit
    diagonal is not stored) and U on and above it, .diag_idxs the position of every diagonal, .analysis the
    FactorizationAnalysis of the pattern."""

    def __init__(self, gk, n, a_row_ptrs, a_col_idxs, pattern):
        self.gk, self.n = gk, int(n)
        self.a_row_ptrs, self.a_col_idxs = a_row_ptrs, a_col_idxs
        frp, fc = pattern
        dv = frp.device
        self.combined = (frp, fc, torch.zeros(int(fc.numel()), dtype=torch.float64, device=dv))
        self.diag_idxs = torch.zeros(max(self.n, 1), dtype=torch.int32, device=dv)[:self.n]
        self._flag = torch.zeros(8, dtype=torch.uint8, device=dv)
        # rejects rows that are not strictly ascending or lack their diagonal before anything searches them
        self.analysis = FactorizationAnalysis(gk, self.n, frp, fc)

    def refactorize(self, vals):
        """new values of A on the same pattern: lu_factorization::initialize, then factorize on the kept analysis"""
        s = torch.cuda.current_stream().cuda_stream
        frp, fc, fv = self.combined
        self.gk.lu_initialize_f64_i32(s, self.n, self.a_row_ptrs, self.a_col_idxs, vals, int(fc.numel()), frp, fc, fv,
                                      self.diag_idxs, self._flag, 8)
        self.gk.lu_factorize_f64_i32(s, self.n, frp, fc, fv, self.analysis.ws, self.analysis.nbytes)
        return self


def lu_generate(gk, n, row_ptrs, col_idxs, vals, symbolic=None, symmetric_sparsity=False):
    """experimental::factorization::Lu::generate (core/factorization/lu.cpp:85-145).  symbolic: (row_ptrs, col_idxs)
    of the factor's pattern (sorted rows, diagonal stored, closed under fill), copied; without one,
    symmetric_sparsity=True takes symbolic_cholesky of the matrix and anything else raises
    GkomiError(GKOMI_ENOTSUPPORTED) like lu.cpp:94-99."""
    gk.lu_symbolic_supported(int(symbolic is not None), int(bool(symmetric_sparsity)))
    if symbolic is not None:
        pattern = (symbolic[0].clone(), symbolic[1].clone())
    else:
        pattern = symbolic_cholesky(gk, n, row_ptrs, col_idxs)[1][:2]
    return LuFactorization(gk, n, row_ptrs, col_idxs, pattern).refactorize(vals)


class Direct:
    """experimental::solver::Direct over a combined_lu factorization (core/solver/direct.cpp:131-227):
    LowerTrs(unit_diagonal) then UpperTrs on the combined matrix through one intermediate vector.  Both solves are the
    analysis-free kernels (csrc/trs.hip), which skip the entries of the other triangle; the level plan and the brick
    plan are not handed a two-sided matrix."""

    def __init__(self, gk, lu, nrhs=1):
        self.gk, self.lu, self.n, self.nrhs = gk, lu, lu.n, int(nrhs)
        dv = lu.combined[2].device
        self.intermediate = torch.zeros((self.n, self.nrhs), dtype=torch.float64, device=dv)
        self.trs_bytes = gk.trs_workspace_bytes()
        self.trs_workspace = torch.zeros(self.trs_bytes, dtype=torch.uint8, device=dv)

    def _solve(self, b, x):
        s = torch.cuda.current_stream().cuda_stream
        rp, ci, v = self.lu.combined
        y = self.intermediate
        self.gk.lower_trs_solve_f64_i32(s, self.n, self.nrhs, rp, ci, v, 1, b, b.stride(0), y, y.stride(0),
                                        self.trs_workspace, self.trs_bytes)
        self.gk.upper_trs_solve_f64_i32(s, self.n, self.nrhs, rp, ci, v, 0, y, y.stride(0), x, x.stride(0),
                                        self.trs_workspace, self.trs_bytes)

    def apply(self, *args):
        """apply(b, x): x = A^-1 b.  apply(alpha, b, beta, x): x = alpha A^-1 b + beta x, as the upper solver's advanced
        apply composes it (scale, then add_scaled).  b, x: n x nrhs device tensors, row stride >= nrhs."""
        if len(args) == 2:
            b, x = args
            assert b.shape == (self.n, self.nrhs) and x.shape == (self.n, self.nrhs)
            if self.n > 0:
                self._solve(b, x)
            return x
        alpha, b, beta, x = args
        assert b.shape == (self.n, self.nrhs) and x.shape == (self.n, self.nrhs)
        if self.n == 0:
            return x
        s = torch.cuda.current_stream().cuda_stream
        dv = x.device
        al = alpha if torch.is_tensor(alpha) else torch.tensor([float(alpha)], dtype=torch.float64, device=dv)
        be = beta if torch.is_tensor(beta) else torch.tensor([float(beta)], dtype=torch.float64, device=dv)
        plain = torch.zeros((self.n, self.nrhs), dtype=torch.float64, device=dv)
        self._solve(b, plain)
        self.gk.dense_scale_f64(s, self.n, self.nrhs, be, 1, x, x.stride(0))
        self.gk.dense_add_scaled_f64(s, self.n, self.nrhs, al, 1, plain, plain.stride(0), x, x.stride(0))
        return x

    def overrun(self):
        flag = ctypes.c_int(0)
        self.gk.trs_check_overrun(torch.cuda.current_stream().cuda_stream, self.trs_workspace, ctypes.addressof(flag))
        return bool(flag.value)


# ---- Multigrid ---------------------------------------------------------------------------------------------------
# solver::Multigrid over multigrid::MultigridLevel objects (core/solver/multigrid.cpp), multigrid::FixedCoarsening
# (core/multigrid/fixed_coarsening.cpp) and the smoother build_smoother makes (include/ginkgo/core/solver/ir.hpp:314-350).
# The recursion runs on the host and only queues work; the one look at the device is the residual norm of a
# ResidualNorm criterion between two cycles.

CSR_SPLIT = 4            # GKOMI_CSR_SPLIT: the bit-exact nonzero-split SpMV
MG_CYCLES = ("v", "f", "w")
MG_MID_CASES = ("both", "post_smoother", "pre_smoother", "standalone")
INITIAL_GUESS_MODES = ("zero", "rhs", "provided")


# The fused sweep walks a row with one lane.  profiles/multigrid_probe.md: at least as fast as the three-call sequence up
# to the Galerkin coarse matrix of the 1024 x 1024 Poisson problem (524 288 rows, 1 571 840 nonzeros: 13.4 against 24.2 us),
# slower on the 1024 x 1024 matrix itself (5 238 784 nonzeros: 34.9 against 29.0 us).  No size in between was measured,
# so the default takes the fused path up to the largest size at which it was seen to win.
MG_FUSED_MAX_NNZ = 1571840


def _mg_fused(fused, nnz):
    """fused: True / False as given; None: GKOMI_MG_FUSED=0 turns the fused Jacobi sweep off and =1 on for every size
    (A/B runs), otherwise the measured size rule.  Either path gives the same bits."""
    import os
    if fused is not None:
        return bool(fused)
    env = os.environ.get("GKOMI_MG_FUSED", "")
    if env in ("0", "1"):
        return env == "1"
    return nnz <= MG_FUSED_MAX_NNZ


class _Scalars:
    """the 1 x 1 device scalars a cycle needs (the reference's one_list / neg_one_list), made once"""

    def __init__(self, dv):
        self.dv = dv
        self._vals = {}

    def get(self, value):
        value = float(value)
        if value not in self._vals:
            self._vals[value] = torch.tensor([value], dtype=torch.float64, device=self.dv)
        return self._vals[value]


def _csr_apply(a, b, x, alpha=None, beta=None):
    """x = A b, or x = alpha A b + beta x with device scalars, through the matrix's own strategy and srow; unlike
    Csr.apply nothing is uploaded per call"""
    s = torch.cuda.current_stream().cuda_stream
    strategy, srow = a.strategy & ~(3 << 29), a.srow()
    if srow is None and (strategy & 0xff) == CSR_SPLIT:
        strategy = (strategy & ~0xff) | 1    # no srow (fewer than two nonzeros): the row-cut streaming kernel, bit-exact too
    a.gk.csr_spmv_srow_f64_i32(s, a.nrows, a.ncols, b.shape[1], a.nnz, a.row_ptrs, a.col_idxs, a.vals, b, b.stride(0), x,
                               x.stride(0), alpha, beta, strategy | a.gather_flags(), a.max_row_nnz(), srow, a.srow_tile)
    return x


class MultigridLevel:
    """multigrid::MultigridLevel (include/ginkgo/core/multigrid/multigrid_level.hpp): the fine, restrict, coarse and
    prolong operators of one level, each a gkomi.formats.Csr (.triple(op) gives (row_ptrs, col_idxs, vals)); as a
    LinOp it is their composition: apply(b, x[, alpha, beta])."""

    def __init__(self, fine, restrict, coarse, prolong):
        self.fine, self.restrict, self.coarse, self.prolong = fine, restrict, coarse, prolong

    def get_fine_op(self):
        return self.fine

    def get_restrict_op(self):
        return self.restrict

    def get_coarse_op(self):
        return self.coarse

    def get_prolong_op(self):
        return self.prolong

    @staticmethod
    def triple(op):
        return op.row_ptrs, op.col_idxs, op.vals

    def apply(self, b, x, alpha=None, beta=None):
        """the level as a LinOp is its composition prolong(coarse(restrict(b)))
        (include/ginkgo/core/multigrid/multigrid_level.hpp:101-105); alpha and beta act on the last factor"""
        dv, nrhs = b.device, b.shape[1]
        t1 = torch.zeros((self.restrict.nrows, nrhs), dtype=torch.float64, device=dv)
        t2 = torch.zeros_like(t1)
        self.restrict.apply(b, t1)
        self.coarse.apply(t1, t2)
        return self.prolong.apply(t2, x, alpha, beta)


def fixed_coarsening(gk, n, row_ptrs, col_idxs, vals, coarse_rows, skip_sorting=False, strategy=0):
    """multigrid::FixedCoarsening::generate (core/multigrid/fixed_coarsening.cpp:69-118): the fine matrix sorted unless
    skipped, R = the selection matrix of coarse_rows (values 1, col_idxs = coarse_rows, row_ptrs = 0..m), P = R^T by
    csr::transpose, A_c = R (A P) by two csr::spgemm; all four carry `strategy` as the reference hands the fine
    matrix's strategy on.  coarse_rows: an int32 device tensor or a sequence.  -> MultigridLevel"""
    dv = vals.device
    s = torch.cuda.current_stream().cuda_stream
    n = int(n)
    if not torch.is_tensor(coarse_rows):
        coarse_rows = torch.from_numpy(np.ascontiguousarray(coarse_rows, dtype=np.int32)).to(dv)
    m = int(coarse_rows.numel())
    if m <= 0:
        raise ValueError("coarse_rows must hold at least one row")
    ci, v = _sorted_copy(gk, n, row_ptrs, col_idxs, vals, skip_sorting)
    fine = Csr(gk, n, n, row_ptrs, ci, v, strategy)
    restrict = Csr(gk, m, n, torch.arange(m + 1, dtype=torch.int32, device=dv),
                   coarse_rows.to(device=dv, dtype=torch.int32).clone(), torch.ones(m, dtype=torch.float64, device=dv),
                   strategy)
    tb = gk.csr_transpose_workspace_bytes(n)
    prp = torch.zeros(n + 1, dtype=torch.int32, device=dv)
    pc, pv = _empty_csr(n, m, dv)
    gk.csr_transpose_f64_i32(s, m, n, m, restrict.row_ptrs, restrict.col_idxs, restrict.vals, prp, pc, pv, _bytes(tb, dv), tb)
    prolong = Csr(gk, n, m, prp, pc, pv, strategy)
    coarse = restrict.spgemm(fine.spgemm(prolong))
    return MultigridLevel(fine, restrict, coarse, prolong)


class JacobiSmoother:
    """build_smoother(Jacobi with max_block_size 1, iterations, relaxation) generated on a Csr: `iterations` sweeps
    x <- 1 x + (relaxation (b - A x)) inv_diag of Ir with an Iteration criterion.  One right-hand side with unit
    stride goes through gkomi_multigrid_jacobi_sweeps_f64_i32 (one launch per sweep) where _mg_fused says so (fused
    True / False, GKOMI_MG_FUSED, or the measured size rule); anything else through copy + csr::advanced_spmv +
    jacobi::scalar_apply.
    Both give the same bits.  apply(b, x, zero=False): zero = initial_guess_mode::zero."""
    uses_initial_guess = True
    accepts_zero_guess = True

    def __init__(self, gk, matrix, iterations=1, relaxation=0.9, fused=None, inv_diag=None):
        self.gk, self.matrix, self.iterations, self.relaxation = gk, matrix, int(iterations), float(relaxation)
        self.fused = _mg_fused(fused, matrix.nnz)
        dv = matrix.vals.device
        s = torch.cuda.current_stream().cuda_stream
        n = matrix.nrows
        if inv_diag is None:    # else: the inverted diagonal of a generated scalar Jacobi
            diag = torch.zeros(max(n, 1), dtype=torch.float64, device=dv)[:n]
            inv_diag = torch.zeros_like(diag)
            gk.csr_extract_diagonal_f64_i32(s, n, matrix.row_ptrs, matrix.col_idxs, matrix.vals, diag)
            gk.jacobi_invert_diagonal_f64(s, n, diag, inv_diag)
        self.inv_diag = inv_diag
        self.ws_bytes = int(gk.multigrid_jacobi_sweeps_workspace_bytes(n))
        self.ws = _bytes(self.ws_bytes, dv)
        self.scalars = _Scalars(dv)
        self._residual = None

    def apply(self, b, x, zero=False):
        gk, a, n = self.gk, self.matrix, self.matrix.nrows
        s = torch.cuda.current_stream().cuda_stream
        if self.fused and b.shape[1] == 1 and b.stride(0) == 1 and x.stride(0) == 1:
            gk.multigrid_jacobi_sweeps_f64_i32(s, n, 1, a.nnz, a.row_ptrs, a.col_idxs, a.vals, self.inv_diag, self.relaxation,
                                               b, x, self.iterations, int(bool(zero)), self.ws, self.ws_bytes)
            return x
        nrhs = b.shape[1]
        if zero:
            gk.dense_fill_f64(s, n, nrhs, x, x.stride(0), 0.0)
        if self._residual is None or self._residual.shape != (n, nrhs):
            self._residual = torch.zeros((n, nrhs), dtype=torch.float64, device=b.device)
        r = self._residual
        one, neg_one, relax = self.scalars.get(1.0), self.scalars.get(-1.0), self.scalars.get(self.relaxation)
        for it in range(self.iterations):
            src = b
            if not (it == 0 and zero):
                gk.dense_copy_f64(s, n, nrhs, b, b.stride(0), r, r.stride(0))
                _csr_apply(a, x, r, neg_one, one)
                src = r
            gk.jacobi_scalar_apply_f64(s, n, nrhs, self.inv_diag, relax, src, src.stride(0), one, x, x.stride(0))
        return x


def jacobi_smoother(gk, matrix, iterations=1, relaxation=0.9, fused=None):
    """a factory product: the JacobiSmoother of a gkomi.formats.Csr"""
    return JacobiSmoother(gk, matrix, iterations, relaxation, fused)


class _IrSmoother:
    """build_smoother around a solver that takes no initial guess (multigrid.cpp:148-155): Ir with an Iteration
    criterion; per iteration r = b - A x, then x = 1 x + relaxation solver(r) as the advanced apply of a solver
    composes it: the solve into a temporary, then add_scaled.  (A scalar Jacobi, whose advanced apply rounds
    differently, never gets here: Multigrid hands it to JacobiSmoother.)"""
    uses_initial_guess = True
    accepts_zero_guess = True

    def __init__(self, gk, matrix, inner, iterations, relaxation):
        self.gk, self.matrix, self.inner, self.iterations = gk, matrix, inner, int(iterations)
        self.scalars = _Scalars(matrix.vals.device)
        self.relaxation = float(relaxation)
        self._r = self._z = None

    def apply(self, b, x, zero=False):
        gk, a, n, nrhs = self.gk, self.matrix, self.matrix.nrows, b.shape[1]
        s = torch.cuda.current_stream().cuda_stream
        if zero:
            gk.dense_fill_f64(s, n, nrhs, x, x.stride(0), 0.0)
        if self._r is None or self._r.shape != (n, nrhs):
            self._r = torch.zeros((n, nrhs), dtype=torch.float64, device=b.device)
            self._z = torch.zeros_like(self._r)
        one, neg_one, relax = self.scalars.get(1.0), self.scalars.get(-1.0), self.scalars.get(self.relaxation)
        for it in range(self.iterations):
            src = b
            if not (it == 0 and zero):
                gk.dense_copy_f64(s, n, nrhs, b, b.stride(0), self._r, nrhs)
                _csr_apply(a, x, self._r, neg_one, one)
                src = self._r
            _apply_op(self.inner, src, self._z)
            gk.dense_add_scaled_f64(s, n, nrhs, relax, 1, self._z, nrhs, x, x.stride(0))
        return x


def _apply_op(op, b, x):
    """a smoother / solver slot holds an object with apply(b, x) or a callable (b, x)"""
    return op.apply(b, x) if hasattr(op, "apply") else op(b, x)


class _PythonCallback:
    """a gkomi_apply_fn whose body is a Python apply(b, x): what makes a Multigrid usable as precond= of the solver
    drivers (they call it with device pointers to contiguous n x nrhs vectors on the stream they run on)"""

    class _View:
        def __init__(self, ptr, n, nrhs):
            self.__cuda_array_interface__ = {"shape": (n, nrhs), "typestr": "<f8", "data": (int(ptr), False),
                                             "version": 2, "strides": None}

    class _Record(ctypes.Structure):
        """what _check_precond reads: a Python callback sees bare pointers, so it serves the one column count it
        was made for and a solve with another is refused before any launch"""
        _fields_ = [("nrhs", ctypes.c_int64)]

    def __init__(self, apply, n, nrhs=1):
        self.n, self.nrhs = int(n), int(nrhs)
        self.ctx = self._Record(self.nrhs)
        self.error = None

        def call(ctx, stream, in_ptr, out_ptr):
            try:
                b = torch.as_tensor(self._View(in_ptr, self.n, self.nrhs), device="cuda")
                x = torch.as_tensor(self._View(out_ptr, self.n, self.nrhs), device="cuda")
                apply(b, x)
                return 0
            except Exception as e:  # noqa: BLE001 - must not unwind through the C driver; the solve fails with EINVAL
                import traceback
                traceback.print_exc()
                self.error = e
                return -1
        self._keep = APPLY_FN(call)
        self.fn = ctypes.cast(self._keep, ctypes.c_void_p).value
        self.ctx_ptr = None


class Multigrid:
    """solver::Multigrid with the reference's factory parameters (include/ginkgo/core/solver/multigrid.hpp:218-400),
    generated on a gkomi.formats.Csr.

    mg_level: callables matrix -> MultigridLevel (fixed_coarsening_factory below), chosen per level by level_selector
    (default: the only one, or the level's index).  pre_ / mid_ / post_smoother: lists of length 0 (no smoother), 1
    (for all levels) or len(mg_level) of callables matrix -> smoother, None = no smoother at that level; a product
    whose uses_initial_guess is not True is wrapped like build_smoother does, with smoother_iters and smoother_relax.
    coarsest_solver: list of callables matrix -> solver (apply(b, x) or a callable (b, x)); empty or None: Identity.
    criteria: max_iters cycles and, with reduction, ResidualNorm(reduction, baseline) checked before each cycle.
    fused: False sends a scalar-Jacobi smoother through the three-call sequence instead of the fused sweep, True the
    other way at every size (None: GKOMI_MG_FUSED, else the measured size rule of MG_FUSED_MAX_NNZ); trace: a list that receives (what, level) for every smoother, restriction, prolongation
    and coarsest solve, in call order.

    apply(b, x, initial_guess=None) -> dict(x, iterations, converged, residual_norm, baseline_norm);
    apply_advanced(alpha, b, beta, x): x = alpha MG(b) + beta x on a clone (multigrid.cpp:615-643); solve = apply.
    As precond= of cg_solve, krylov_solve, gmres_solve and solve_op it is applied through callback()."""

    def __init__(self, gk, matrix, mg_level, pre_smoother=(), mid_smoother=(), post_smoother=(), post_uses_pre=True,
                 mid_case="standalone", max_levels=10, min_coarse_rows=64, coarsest_solver=(), cycle="v",
                 smoother_relax=0.9, smoother_iters=1, default_initial_guess="provided", max_iters=1, reduction=None,
                 baseline="rhs_norm", level_selector=None, solver_selector=None, fused=None, trace=None):
        self.fused = fused
        if cycle not in MG_CYCLES or mid_case not in MG_MID_CASES or default_initial_guess not in INITIAL_GUESS_MODES:
            raise ValueError("cycle, mid_case or default_initial_guess")
        mg_level, coarsest_solver = list(mg_level), list(coarsest_solver)
        pre_smoother, mid_smoother, post_smoother = list(pre_smoother), list(mid_smoother), list(post_smoother)
        # validate (multigrid.cpp:711-748)
        if len(mg_level) == 0 or any(f is None for f in mg_level):
            raise ValueError("mg_level needs at least one factory and no null entry")
        for checked, lst, what in ((True, pre_smoother, "pre_smoother"), (not post_uses_pre, post_smoother, "post_smoother"),
                                   (mid_case == "standalone", mid_smoother, "mid_smoother")):
            if checked and len(lst) > 1 and len(lst) != len(mg_level):
                raise ValueError(f"{what}: {len(lst)} entries for {len(mg_level)} mg_level entries (0, 1 or as many)")
        self.gk, self.matrix, self.mid_case, self.trace = gk, matrix, mid_case, trace
        self.max_iters, self.reduction, self.baseline = int(max_iters), reduction, baseline
        self.default_initial_guess = default_initial_guess
        self.smoother_relax, self.smoother_iters = smoother_relax, smoother_iters
        self._cycle = cycle
        if level_selector is None:
            level_selector = (lambda level, m: 0) if len(mg_level) == 1 else (lambda level, m: level)
        if solver_selector is None:
            solver_selector = lambda level, m: 0
        # generate (multigrid.cpp:491-574)
        self.mg_level_list, self.pre_smoother_list, self.mid_smoother_list, self.post_smoother_list = [], [], [], []
        m, level = matrix, 0
        while level < max_levels and m.nrows > min_coarse_rows:
            index = level_selector(level, m)
            lvl = mg_level[index](m)
            if lvl.get_coarse_op().nrows == m.nrows:
                break    # the level does not reduce the dimension
            self._handle_list(index, lvl.get_fine_op(), pre_smoother, self.pre_smoother_list)
            if mid_case == "standalone":
                self._handle_list(index, lvl.get_fine_op(), mid_smoother, self.mid_smoother_list)
            if not post_uses_pre:
                self._handle_list(index, lvl.get_fine_op(), post_smoother, self.post_smoother_list)
            self.mg_level_list.append(lvl)
            m = lvl.get_coarse_op()
            level += 1
        if post_uses_pre:
            self.post_smoother_list = self.pre_smoother_list
        if level == 0:
            raise ValueError("Multigrid generated no level: the matrix has no more than min_coarse_rows rows, "
                             "max_levels is 0 or the first level does not reduce the dimension")
        factory = coarsest_solver[solver_selector(level, m)] if coarsest_solver else None
        self.coarsest_solver = None if factory is None else factory(m)     # None: Identity
        self.scalars = _Scalars(matrix.vals.device)
        self._state_nrhs = None
        self._callback = None

    def _handle_list(self, index, m, factories, out):
        f = factories[0 if len(factories) == 1 else index] if factories else None
        if f is None:
            out.append(None)
            return
        s = f(m)
        if getattr(s, "uses_initial_guess", False) is True:
            out.append(s)
        elif isinstance(s, Preconditioner) and isinstance(s.ctx, JacobiCtx) and s.ctx.max_block_size == 1 and isinstance(m, Csr):
            # Ir over a generated scalar Jacobi with an Iteration criterion: the fused sweep (or its three-call twin)
            out.append(JacobiSmoother(self.gk, m, self.smoother_iters, self.smoother_relax, self.fused, inv_diag=s.keep[0]))
        else:
            out.append(_IrSmoother(self.gk, m, s, self.smoother_iters, self.smoother_relax))

    # accessors of the reference
    def get_mg_level_list(self):
        return self.mg_level_list

    def get_pre_smoother_list(self):
        return self.pre_smoother_list

    def get_mid_smoother_list(self):
        return self.mid_smoother_list

    def get_post_smoother_list(self):
        return self.post_smoother_list

    def get_coarsest_solver(self):
        return self.coarsest_solver

    def get_cycle(self):
        return self._cycle

    def set_cycle(self, cycle):
        if cycle not in MG_CYCLES:
            raise ValueError("cycle")
        self._cycle = cycle

    def _note(self, what, level):
        if self.trace is not None:
            self.trace.append((what, level))

    def _allocate(self, nrhs, dv):
        """MultigridState::generate: r of every level's rows, g and e of the next level's, once per nrhs"""
        if self._state_nrhs == nrhs:
            return
        vec = lambda rows: torch.zeros((max(rows, 1), nrhs), dtype=torch.float64, device=dv)[:rows]
        self._r = [vec(lvl.get_fine_op().nrows) for lvl in self.mg_level_list]
        self._g = [vec(lvl.get_coarse_op().nrows) for lvl in self.mg_level_list]
        self._e = [vec(lvl.get_coarse_op().nrows) for lvl in self.mg_level_list]
        self._state_nrhs = nrhs

    def _smooth(self, smoother, b, x, zero=False, level=0):
        if zero and getattr(smoother, "accepts_zero_guess", False):
            return smoother.apply(b, x, zero=True)
        if zero and level != 0:
            # no initial-guess interface: fill, then apply; x of the first level is zero already (multigrid.cpp:413-419)
            self.gk.dense_fill_f64(torch.cuda.current_stream().cuda_stream, x.shape[0], x.shape[1], x, x.stride(0), 0.0)
        return _apply_op(smoother, b, x)

    def _run_cycle(self, cycle, level, m, b, x, x_is_zero, first, end):
        """MultigridState::run_cycle (multigrid.cpp:377-485); queues work only"""
        gk = self.gk
        s = torch.cuda.current_stream().cuda_stream
        total = len(self.mg_level_list)
        nrhs = b.shape[1]
        if level == total:
            if self.coarsest_solver is None:
                gk.dense_copy_f64(s, b.shape[0], nrhs, b, b.stride(0), x, x.stride(0))
            else:
                self._note("coarsest", level)
                _apply_op(self.coarsest_solver, b, x)
            return
        lvl = self.mg_level_list[level]
        pre, post = self.pre_smoother_list[level], self.post_smoother_list[level]
        mid = self.mid_smoother_list[level] if self.mid_case == "standalone" else None
        one, neg_one = self.scalars.get(1.0), self.scalars.get(-1.0)
        if (first or self.mid_case in ("both", "pre_smoother")) and pre is not None:
            self._note("pre", level)
            self._smooth(pre, b, x, zero=x_is_zero, level=level)
        r, g, e = self._r[level], self._g[level], self._e[level]
        gk.dense_copy_f64(s, m.nrows, nrhs, b, b.stride(0), r, r.stride(0))
        _csr_apply(m, x, r, neg_one, one)
        self._note("restrict", level)
        _csr_apply(lvl.get_restrict_op(), r, g)
        if level + 1 == total:
            gk.dense_fill_f64(s, e.shape[0], nrhs, e, e.stride(0), 0.0)
        nxt = self.mg_level_list[level + 1].get_fine_op() if level + 1 < total else lvl.get_coarse_op()
        self._run_cycle(cycle, level + 1, nxt, g, e, True, True, cycle == "v")
        if level < total - 1:
            if cycle == "f":
                self._run_cycle("v", level + 1, nxt, g, e, False, False, True)
            elif cycle == "w":
                self._run_cycle(cycle, level + 1, nxt, g, e, False, False, True)
        self._note("prolong", level)
        _csr_apply(lvl.get_prolong_op(), e, x, one, one)
        if (end or self.mid_case in ("both", "post_smoother")) and post is not None:
            self._note("post", level)
            self._smooth(post, b, x)
        if cycle in ("w", "f") and not end and self.mid_case == "standalone" and mid is not None:
            self._note("mid", level)
            self._smooth(mid, b, x)

    def _residual_norm(self, b, x):
        """the look of a ResidualNorm criterion: || b - A x || per column, on the host"""
        gk, n, nrhs = self.gk, self.matrix.nrows, b.shape[1]
        s = torch.cuda.current_stream().cuda_stream
        r = self._r[0]
        gk.dense_copy_f64(s, n, nrhs, b, b.stride(0), r, r.stride(0))
        _csr_apply(self.matrix, x, r, self.scalars.get(-1.0), self.scalars.get(1.0))
        return self._norm2(r)

    def _norm2(self, v):
        gk, (n, nrhs) = self.gk, v.shape
        nb = int(gk.dense_reduction_workspace_bytes(n, nrhs))
        out = torch.zeros(nrhs, dtype=torch.float64, device=v.device)
        gk.dense_compute_norm2_f64(torch.cuda.current_stream().cuda_stream, n, nrhs, v, v.stride(0), out,
                                   _bytes(nb, v.device), nb)
        return out.cpu().numpy()

    def apply(self, b, x, initial_guess=None):
        guess = initial_guess or self.default_initial_guess
        if guess not in INITIAL_GUESS_MODES:
            raise ValueError("initial_guess")
        n = self.matrix.nrows
        b2, x2, nrhs = _operands(n, b, x)
        gk = self.gk
        s = torch.cuda.current_stream().cuda_stream
        if guess == "zero":
            gk.dense_fill_f64(s, n, nrhs, x2, x2.stride(0), 0.0)
        elif guess == "rhs":
            gk.dense_copy_f64(s, n, nrhs, b2, b2.stride(0), x2, x2.stride(0))
        self._allocate(nrhs, b2.device)
        it, converged = 0, False
        res = base = None
        while True:
            if it >= self.max_iters:     # Iteration is asked first, as by the drivers and the restatement
                break
            if self.reduction is not None:
                res = self._residual_norm(b2, x2)
                if base is None:
                    base = {"rhs_norm": lambda: self._norm2(b2), "initial_resnorm": lambda: res.copy(),
                            "absolute": lambda: np.ones(nrhs)}[self.baseline]()
                if np.all(res <= self.reduction * base):
                    converged = True
                    break
            self._run_cycle(self._cycle, 0, self.matrix, b2, x2, it == 0 and guess == "zero", True, True)
            it += 1
        return {"x": x2 if b.dim() > 1 else x2.reshape(n), "iterations": it, "converged": converged, "residual_norm": res,
                "baseline_norm": base}

    solve = apply

    def apply_advanced(self, alpha, b, beta, x, initial_guess=None):
        guess = initial_guess or self.default_initial_guess
        n = self.matrix.nrows
        b2, x2, nrhs = _operands(n, b, x)
        gk = self.gk
        s = torch.cuda.current_stream().cuda_stream
        if guess == "zero":
            gk.dense_fill_f64(s, n, nrhs, x2, x2.stride(0), 0.0)
        elif guess == "rhs":
            gk.dense_copy_f64(s, n, nrhs, b2, b2.stride(0), x2, x2.stride(0))
        clone = x2.clone()
        out = self.apply(b2, clone, initial_guess="provided" if guess != "zero" else "zero")
        gk.dense_scale_f64(s, n, nrhs, self.scalars.get(beta), 1, x2, x2.stride(0))
        gk.dense_add_scaled_f64(s, n, nrhs, self.scalars.get(alpha), 1, clone, clone.stride(0), x2, x2.stride(0))
        out["x"] = x2 if b.dim() > 1 else x2.reshape(n)
        return out

    def callback(self):
        """(fn, ctx_ptr) holder for the solver drivers: one application with the default initial guess"""
        if self._callback is None:
            self._callback = _PythonCallback(lambda b, x: self.apply(b, x), self.matrix.nrows)
        return self._callback

    # what _callback(precond) of the solve functions reads
    @property
    def fn(self):
        return self.callback().fn

    @property
    def ctx_ptr(self):
        return None

    @property
    def ctx(self):
        return self.callback().ctx


class OrderedCg:
    """solver::Cg with an Iteration criterion and no preconditioner as the reference's kernel sequence (core/solver/cg.cpp:
    cg::initialize, step_1, step_2, the SpMV of the matrix's strategy), with both dot products formed in the reference
    executor's order: a 1 x n by n x 1 product of gkomi_dense_gemm_f64 in its ordered mode, one chain from +0.0.  With a
    bit-exact SpMV strategy x is the reference executor's bit for bit, which the native Cg drivers (re-ordered
    reductions) cannot give.  One chain per dot product: for small systems such as the coarsest level of a Multigrid.
    apply(b, x) takes x as the initial guess; one right-hand side; nothing blocks.

    This is not a general Cg: it exists to reproduce the reference executor's bits where a test pins them, and its serial
    dot products make it slow on anything large.  Use cg_solve to solve a system."""

    def __init__(self, gk, matrix, max_iters):
        self.gk, self.matrix, self.max_iters = gk, matrix, int(max_iters)
        n, dv = matrix.nrows, matrix.vals.device
        vec = lambda: torch.zeros((max(n, 1), 1), dtype=torch.float64, device=dv)[:n]
        self.r, self.z, self.p, self.q = vec(), vec(), vec(), vec()
        self.scalars = torch.zeros(3, dtype=torch.float64, device=dv)      # prev_rho, rho, beta
        self.status = torch.zeros(8, dtype=torch.uint8, device=dv)
        self.one_minus = _Scalars(dv)

    def _dot(self, a, b, out):
        n = self.matrix.nrows
        self.gk.dense_gemm_f64(torch.cuda.current_stream().cuda_stream, 1, 1, n, a, max(n, 1), b, 1, out, 1, None, None, 1, None, 0)

    def apply(self, b, x):
        gk, a, n = self.gk, self.matrix, self.matrix.nrows
        if b.shape[1] != 1:
            raise ValueError("OrderedCg takes one right-hand side")
        s = torch.cuda.current_stream().cuda_stream
        r, z, p, q = self.r, self.z, self.p, self.q
        prev_rho, rho, beta = self.scalars[0:1], self.scalars[1:2], self.scalars[2:3]
        gk.cg_initialize_f64(s, n, 1, b, b.stride(0), r, 1, z, 1, p, 1, q, 1, prev_rho, rho, self.status)
        _csr_apply(a, x, r, self.one_minus.get(-1.0), self.one_minus.get(1.0))
        for _ in range(self.max_iters):
            gk.dense_copy_f64(s, n, 1, r, 1, z, 1)          # the Identity preconditioner
            self._dot(r, z, rho)
            gk.cg_step_1_f64(s, n, 1, p, 1, z, 1, rho, prev_rho, self.status)
            _csr_apply(a, p, q)
            self._dot(p, q, beta)
            gk.cg_step_2_f64(s, n, 1, x, x.stride(0), r, 1, p, 1, q, 1, beta, rho, self.status)
            prev_rho, rho = rho, prev_rho
        return x


def fixed_coarsening_factory(gk, select, skip_sorting=False):
    """an mg_level entry: select(matrix) -> the coarse rows of that matrix"""
    return lambda m: fixed_coarsening(gk, m.nrows, m.row_ptrs, m.col_idxs, m.vals, select(m), skip_sorting, m.strategy)


PGM_EXITS = ("nothing left", "no new match", "ratio", "max_iterations")


def pgm(gk, n, row_ptrs, col_idxs, vals, max_iterations=15, max_unassigned_ratio=0.05, deterministic=False,
        skip_sorting=False, strategy=0):
    """multigrid::Pgm::generate (core/multigrid/pgm.cpp:147-236) through gkomi_pgm_generate_f64_i32, all of it on the
    device: the fine matrix sorted unless skipped (with skip_sorting the caller's arrays are the fine operator), the
    aggregates, the restriction and the coarse matrix with the reference executor's integers and bits.  The restriction
    (num_agg x n, sorted rows) and the prolongation (one entry per row at column agg[i]) are unit-valued Csr matrices:
    their applies add what SparsityCsr's and RowGatherer's add, in the same order.  -> MultigridLevel with .agg (int32,
    n), .num_agg and .info = dict(iterations, left, exit, jump_rounds)"""
    n, max_iterations = int(n), int(max_iterations)
    if n <= 0:
        raise ValueError("Pgm needs a matrix with at least one row")
    if max_iterations < 0 or not 0.0 <= float(max_unassigned_ratio) <= 1.0:
        raise ValueError("max_iterations must not be negative and max_unassigned_ratio must lie in [0, 1]")
    if row_ptrs.numel() != n + 1 or col_idxs.numel() != vals.numel():
        raise ValueError("row_ptrs needs n + 1 entries, col_idxs as many as vals")
    dv = vals.device
    s = torch.cuda.current_stream().cuda_stream
    nnz = int(vals.numel())
    i32 = lambda k: torch.zeros(k, dtype=torch.int32, device=dv)
    if skip_sorting:
        fci, fv = col_idxs, vals
    else:
        fci, fv = _empty_csr(n, nnz, dv)
    agg, rrp, rci, crp = i32(n), i32(n + 1), i32(n), i32(n + 1)
    nb = gk.pgm_generate_workspace_bytes(n, nnz)
    ws = _bytes(nb, dv)
    num_agg, cnnz, info = ctypes.c_int64(0), ctypes.c_int64(0), (ctypes.c_int64 * 4)()

    def call(cc, cv):
        gk.pgm_generate_f64_i32(s, n, nnz, row_ptrs, col_idxs, vals, max_iterations, float(max_unassigned_ratio),
                                int(bool(deterministic)), int(bool(skip_sorting)), None if skip_sorting else fci,
                                None if skip_sorting else fv, agg, rrp, rci, crp, cc, cv, ctypes.addressof(num_agg),
                                ctypes.addressof(cnnz), ctypes.addressof(info), ws, nb)
    cc, cv = _count_then_fill(call, [cnnz], dv)
    m = int(num_agg.value)
    fine = Csr(gk, n, n, row_ptrs, fci, fv, strategy)
    restrict = Csr(gk, m, n, rrp[:m + 1].clone(), rci, torch.ones(n, dtype=torch.float64, device=dv), strategy)
    prolong = Csr(gk, n, m, torch.arange(n + 1, dtype=torch.int32, device=dv), agg.clone(),
                  torch.ones(n, dtype=torch.float64, device=dv), strategy)
    coarse = Csr(gk, m, m, crp[:m + 1].clone(), cc, cv, strategy)
    lvl = MultigridLevel(fine, restrict, coarse, prolong)
    lvl.agg, lvl.num_agg = agg, m
    lvl.info = dict(iterations=int(info[0]), left=int(info[1]), exit=PGM_EXITS[int(info[2])], jump_rounds=int(info[3]))
    return lvl


def pgm_factory(gk, **parameters):
    """an mg_level entry: Pgm with these parameters on whatever matrix the hierarchy hands it"""
    return lambda m: pgm(gk, m.nrows, m.row_ptrs, m.col_idxs, m.vals, strategy=m.strategy, **parameters)
