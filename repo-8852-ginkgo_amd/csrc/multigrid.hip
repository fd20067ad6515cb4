// Multigrid kernels for gfx950.
//
// 1. gko::kernels::hip::multigrid::{kcycle_step_1, kcycle_step_2, kcycle_check_stop}
//    (core/solver/multigrid_kernels.hpp); semantics = reference/solver/multigrid_kernels.cpp:53-119.
//    Elementwise over nrows x nrhs, every scalar expression in the reference's order, so bit-exact.
//
// 2. The smoother of a multigrid cycle in one launch per sweep: `sweeps` iterations of solver::Ir
//    (core/solver/ir.cpp:186-276) over a scalar preconditioner::Jacobi with an Iteration criterion on a
//    Csr<double, int32> and one right-hand side,
//        x <- 1 x + (relax (b - A x)) inv_diag.
//    Through the separate entry points one sweep is a copy (r = b), an advanced SpMV (r = -1 A x + 1 r) and a
//    scalar_apply (x = 1 x + relax r inv_diag): three launches, five passes over vectors, and on the coarse levels of
//    a hierarchy nothing but launch latency.  Here one lane owns one row and walks it in stored order:
//        t = b_i;  t += (-1 val_k) x[col_k]  for k left to right   (reference/matrix/csr_kernels.cpp:115-127)
//        x_i' = 1 x_i + (relax t) inv_diag_i                        (reference/preconditioner/jacobi_kernels.cpp:573-578)
//    every product and sum rounded once (the library is built with -ffp-contract=off), which is the order the
//    reference executor and the nonzero-split SpMV add in -- bit-identical for any row length.
//    A sweep reads the old x everywhere, so it writes to a second buffer and the buffers swap; sweeps are ordered on
//    the stream, no kernel waits for another workgroup and the host never looks.
#include "internal.hpp"

namespace gkomi {
namespace {

constexpr int block = 256;

__device__ __forceinline__ bool is_finite(double v) { return fabs(v) < __builtin_huge_val(); }

__global__ __launch_bounds__(block) void kcycle_step_1_kernel(
    int64_t nrows, int64_t nrhs, const double* __restrict__ alpha, const double* __restrict__ rho,
    const double* __restrict__ v, int64_t v_stride, double* __restrict__ g, int64_t g_stride,
    double* __restrict__ d, int64_t d_stride, double* __restrict__ e, int64_t e_stride)
{
    const int64_t total = nrows * nrhs;
    for (int64_t idx = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; idx < total;
         idx += static_cast<int64_t>(gridDim.x) * block) {
        const int64_t j = idx / nrhs, i = idx % nrhs;
        const double temp = alpha[i] / rho[i];
        double ev = e[j * e_stride + i];
        if (is_finite(temp)) {
            g[j * g_stride + i] -= temp * v[j * v_stride + i];
            ev *= temp;
            e[j * e_stride + i] = ev;
        }
        d[j * d_stride + i] = ev;
    }
}

__global__ __launch_bounds__(block) void kcycle_step_2_kernel(
    int64_t nrows, int64_t nrhs, const double* __restrict__ alpha, const double* __restrict__ rho,
    const double* __restrict__ gamma, const double* __restrict__ beta, const double* __restrict__ zeta,
    const double* __restrict__ d, int64_t d_stride, double* __restrict__ e, int64_t e_stride)
{
    const int64_t total = nrows * nrhs;
    for (int64_t idx = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; idx < total;
         idx += static_cast<int64_t>(gridDim.x) * block) {
        const int64_t j = idx / nrhs, i = idx % nrhs;
        const double scalar_d = zeta[i] / (beta[i] - gamma[i] * gamma[i] / rho[i]);
        const double scalar_e = 1.0 - gamma[i] / alpha[i] * scalar_d;
        if (is_finite(scalar_d) && is_finite(scalar_e)) {
            e[j * e_stride + i] = scalar_e * e[j * e_stride + i] + scalar_d * d[j * d_stride + i];
        }
    }
}

// one wave: lane i looks at columns i, i + 64, ...
__global__ __launch_bounds__(wave_size) void kcycle_check_stop_kernel(
    int64_t nrhs, const double* __restrict__ old_norm, const double* __restrict__ new_norm, double rel_tol,
    uint8_t* __restrict__ is_stop)
{
    bool go_on = false;
    for (int64_t i = threadIdx.x; i < nrhs; i += wave_size) {
        if (new_norm[i] > rel_tol * old_norm[i]) go_on = true;
    }
    const bool any = __any(go_on);
    if (threadIdx.x == 0) *is_stop = any ? 0 : 1;
}

// ZeroGuess: the sweep of Ir with initial_guess_mode::zero -- x counts as filled with zeros and the residual is b
// itself, no product with A (ir.cpp:208-214); x_in is not read.
template <bool ZeroGuess>
__global__ __launch_bounds__(block) void jacobi_sweep_kernel(
    int n, const int32_t* __restrict__ row_ptrs, const int32_t* __restrict__ col_idxs,
    const double* __restrict__ vals, const double* __restrict__ inv_diag, double relax,
    const double* __restrict__ b, const double* __restrict__ x_in, double* __restrict__ x_out)
{
    const int row = blockIdx.x * block + threadIdx.x;
    if (row >= n) return;
    double t = b[row];
    double xi = 0.0;
    if (!ZeroGuess) {
        const int32_t end = row_ptrs[row + 1];
        for (int32_t k = row_ptrs[row]; k < end; ++k) {
            t += (-1.0 * vals[k]) * x_in[col_idxs[k]];
        }
        xi = x_in[row];
    }
    x_out[row] = 1.0 * xi + (relax * t) * inv_diag[row];
}

bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const char* pa = static_cast<const char*>(a);
    const char* pb = static_cast<const char*>(b);
    return pa < pb + b_bytes && pb < pa + a_bytes;
}

}  // namespace
}  // namespace gkomi

using namespace gkomi;

extern "C" int gkomi_multigrid_kcycle_step_1_f64(gkomi_stream_t s, int64_t nrows, int64_t nrhs,
                                                 const double* alpha, const double* rho, const double* v,
                                                 int64_t v_stride, double* g, int64_t g_stride, double* d,
                                                 int64_t d_stride, double* e, int64_t e_stride)
{
    if (nrows < 0 || nrhs < 0) return GKOMI_EINVAL;
    if (v_stride < nrhs || g_stride < nrhs || d_stride < nrhs || e_stride < nrhs) return GKOMI_EINVAL;
    if (nrows == 0 || nrhs == 0) return GKOMI_SUCCESS;
    if (alpha == nullptr || rho == nullptr || v == nullptr || g == nullptr || d == nullptr || e == nullptr)
        return GKOMI_EINVAL;
    hipLaunchKernelGGL(kcycle_step_1_kernel, dim3(grid_for(nrows * nrhs, block)), dim3(block), 0, to_stream(s),
                       nrows, nrhs, alpha, rho, v, v_stride, g, g_stride, d, d_stride, e, e_stride);
    return check_launch();
}

extern "C" int gkomi_multigrid_kcycle_step_2_f64(gkomi_stream_t s, int64_t nrows, int64_t nrhs,
                                                 const double* alpha, const double* rho, const double* gamma,
                                                 const double* beta, const double* zeta, const double* d,
                                                 int64_t d_stride, double* e, int64_t e_stride)
{
    if (nrows < 0 || nrhs < 0) return GKOMI_EINVAL;
    if (d_stride < nrhs || e_stride < nrhs) return GKOMI_EINVAL;
    if (nrows == 0 || nrhs == 0) return GKOMI_SUCCESS;
    if (alpha == nullptr || rho == nullptr || gamma == nullptr || beta == nullptr || zeta == nullptr ||
        d == nullptr || e == nullptr)
        return GKOMI_EINVAL;
    hipLaunchKernelGGL(kcycle_step_2_kernel, dim3(grid_for(nrows * nrhs, block)), dim3(block), 0, to_stream(s),
                       nrows, nrhs, alpha, rho, gamma, beta, zeta, d, d_stride, e, e_stride);
    return check_launch();
}

extern "C" int gkomi_multigrid_kcycle_check_stop_f64(gkomi_stream_t s, int64_t nrhs, const double* old_norm,
                                                     const double* new_norm, double rel_tol,
                                                     uint8_t* is_stop_device)
{
    if (nrhs < 0 || is_stop_device == nullptr) return GKOMI_EINVAL;
    if (nrhs > 0 && (old_norm == nullptr || new_norm == nullptr)) return GKOMI_EINVAL;
    hipLaunchKernelGGL(kcycle_check_stop_kernel, dim3(1), dim3(wave_size), 0, to_stream(s), nrhs, old_norm,
                       new_norm, rel_tol, is_stop_device);
    return check_launch();
}

extern "C" size_t gkomi_multigrid_jacobi_sweeps_workspace_bytes(int64_t n)
{
    return n > 0 ? align256(sizeof(double) * static_cast<size_t>(n)) : 0;
}

extern "C" int gkomi_multigrid_jacobi_sweeps_f64_i32(gkomi_stream_t s, int64_t n, int64_t nrhs, int64_t nnz,
                                                     const int32_t* row_ptrs, const int32_t* col_idxs,
                                                     const double* vals, const double* inv_diag, double relax,
                                                     const double* b, double* x, int64_t sweeps, int zero_guess,
                                                     void* workspace, size_t workspace_bytes)
{
    if (n < 0 || nnz < 0 || sweeps < 0 || nrhs != 1) return GKOMI_EINVAL;
    if (n > INT32_MAX || nnz > INT32_MAX) return GKOMI_ENOTSUPPORTED;
    if (n == 0) return GKOMI_SUCCESS;
    if (row_ptrs == nullptr || inv_diag == nullptr || b == nullptr || x == nullptr) return GKOMI_EINVAL;
    if (nnz > 0 && (col_idxs == nullptr || vals == nullptr)) return GKOMI_EINVAL;
    const size_t vec_bytes = sizeof(double) * static_cast<size_t>(n);
    if (workspace == nullptr || workspace_bytes < gkomi_multigrid_jacobi_sweeps_workspace_bytes(n))
        return GKOMI_EINVAL;
    if (overlaps(workspace, workspace_bytes, x, vec_bytes) || overlaps(workspace, workspace_bytes, b, vec_bytes))
        return GKOMI_EINVAL;
    hipStream_t stream = to_stream(s);
    if (sweeps == 0) {
        // Ir still prepares the initial guess (ir.cpp:179)
        return zero_guess ? static_cast<int>(hipMemsetAsync(x, 0, vec_bytes, stream)) : GKOMI_SUCCESS;
    }
    double* other = static_cast<double*>(workspace);
    const int rows = static_cast<int>(n);
    const dim3 grid(static_cast<unsigned>(ceildiv(n, block)));
    // sweep j writes to x when an even number of sweeps follows it.  The first sweep of a provided guess reads x, so
    // with an odd count it cannot also write there: the guess moves to the workspace first (the one extra pass).
    const double* src = x;
    int64_t j = 0;
    if (zero_guess) {
        double* dst = (sweeps - 1) % 2 == 0 ? x : other;
        hipLaunchKernelGGL(jacobi_sweep_kernel<true>, grid, dim3(block), 0, stream, rows, row_ptrs, col_idxs, vals,
                           inv_diag, relax, b, src, dst);
        src = dst;
        j = 1;
    } else if (sweeps % 2 != 0) {
        const int err = static_cast<int>(hipMemcpyAsync(other, x, vec_bytes, hipMemcpyDeviceToDevice, stream));
        if (err) return err;
        src = other;
    }
    for (; j < sweeps; ++j) {
        double* dst = src == x ? other : x;
        hipLaunchKernelGGL(jacobi_sweep_kernel<false>, grid, dim3(block), 0, stream, rows, row_ptrs, col_idxs,
                           vals, inv_diag, relax, b, src, dst);
        src = dst;
    }
    return check_launch();
}
