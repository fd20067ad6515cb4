// BiCGSTAB, FCG and CGS for gfx950 (the Krylov solvers that
// share CG's BLAS-1).  Replaces gko::kernels::hip::{bicgstab, fcg, cgs}::
// {initialize, step_1, step_2, step_3, finalize}
// (core/solver/{bicgstab,fcg,cgs}_kernels.hpp; the reference's GPU versions
// are the unified kernels common/unified/solver/*_kernels.cpp) and provides
// native drivers for {Bicgstab,Fcg,Cgs}::apply_dense_impl
// (core/solver/bicgstab.cpp:107-234, fcg.cpp:104-196, cgs.cpp:107-205).
// Semantics = reference/solver/{bicgstab,fcg,cgs}_kernels.cpp.
//
// The step kernels are pure streaming (3n..7n values, HBM-bound): one thread
// per element, the per-column scalars read from device memory, every
// expression written exactly as the reference's (-ffp-contract=off) ->
// bit-identical.  Scalars a step defines (alpha, omega, beta) are recomputed by
// every thread from their inputs and stored once by row 0.
#include <algorithm>
#include <utility>

#include "common.hpp"
#include "fused_krylov.hpp"
#include "internal.hpp"
#include "krylov_driver.hpp"

namespace gkomi {
namespace {

constexpr int block = 256;
constexpr uint8_t finalized_mask = 0x40;  // stopping_status::is_finalized (stopping_status.hpp)

#define GKOMI_ELEMENTWISE(i, j)                                                         \
    const int64_t idx_ = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x;        \
    if (idx_ >= n * nrhs) return;                                                       \
    const int64_t i = idx_ / nrhs;                                                      \
    const int64_t j = idx_ - i * nrhs

// ---- BiCGSTAB ---------------------------------------------------------------
__global__ __launch_bounds__(block) void bicgstab_initialize_kernel(
    int64_t n, int64_t nrhs, const double* __restrict__ b, int64_t b_stride,
    double* __restrict__ r, int64_t r_stride, double* __restrict__ rr, int64_t rr_stride,
    double* __restrict__ y, int64_t y_stride, double* __restrict__ s, int64_t s_stride,
    double* __restrict__ t, int64_t t_stride, double* __restrict__ z, int64_t z_stride,
    double* __restrict__ v, int64_t v_stride, double* __restrict__ p, int64_t p_stride,
    double* __restrict__ prev_rho, double* __restrict__ rho, double* __restrict__ alpha,
    double* __restrict__ beta, double* __restrict__ gamma, double* __restrict__ omega,
    uint8_t* __restrict__ stop_status)
{
    const int64_t idx = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x;
    if (idx < nrhs) {
        rho[idx] = prev_rho[idx] = alpha[idx] = beta[idx] = gamma[idx] = omega[idx] = 1.0;
        stop_status[idx] = 0;
    }
    if (idx >= n * nrhs) return;
    const int64_t i = idx / nrhs, j = idx - i * nrhs;
    r[i * r_stride + j] = b[i * b_stride + j];
    rr[i * rr_stride + j] = z[i * z_stride + j] = v[i * v_stride + j] = s[i * s_stride + j] =
        t[i * t_stride + j] = y[i * y_stride + j] = p[i * p_stride + j] = 0.0;
}

__global__ __launch_bounds__(block) void bicgstab_step_1_kernel(
    int64_t n, int64_t nrhs, const double* __restrict__ r, int64_t r_stride,
    double* __restrict__ p, int64_t p_stride, const double* __restrict__ v, int64_t v_stride,
    const double* __restrict__ rho, const double* __restrict__ prev_rho,
    const double* __restrict__ alpha, const double* __restrict__ omega,
    const uint8_t* __restrict__ stop_status)
{
    GKOMI_ELEMENTWISE(i, j);
    if (status_has_stopped(stop_status[j])) return;
    if (prev_rho[j] * omega[j] != 0.0) {
        const double tmp = rho[j] / prev_rho[j] * alpha[j] / omega[j];
        p[i * p_stride + j] =
            r[i * r_stride + j] + tmp * (p[i * p_stride + j] - omega[j] * v[i * v_stride + j]);
    } else {
        p[i * p_stride + j] = r[i * r_stride + j];
    }
}

__global__ __launch_bounds__(block) void bicgstab_step_2_kernel(
    int64_t n, int64_t nrhs, const double* __restrict__ r, int64_t r_stride,
    double* __restrict__ s, int64_t s_stride, const double* __restrict__ v, int64_t v_stride,
    const double* __restrict__ rho, double* __restrict__ alpha, const double* __restrict__ beta,
    const uint8_t* __restrict__ stop_status)
{
    GKOMI_ELEMENTWISE(i, j);
    if (status_has_stopped(stop_status[j])) return;
    double a = 0.0;
    if (beta[j] != 0.0) {
        a = rho[j] / beta[j];
        s[i * s_stride + j] = r[i * r_stride + j] - a * v[i * v_stride + j];
    } else {
        s[i * s_stride + j] = r[i * r_stride + j];
    }
    if (i == 0) alpha[j] = a;  // nobody reads alpha in this kernel
}

__global__ __launch_bounds__(block) void bicgstab_step_3_kernel(
    int64_t n, int64_t nrhs, double* __restrict__ x, int64_t x_stride, double* __restrict__ r,
    int64_t r_stride, const double* __restrict__ s, int64_t s_stride,
    const double* __restrict__ t, int64_t t_stride, const double* __restrict__ y,
    int64_t y_stride, const double* __restrict__ z, int64_t z_stride,
    const double* __restrict__ alpha, const double* __restrict__ beta,
    const double* __restrict__ gamma, double* __restrict__ omega,
    const uint8_t* __restrict__ stop_status)
{
    GKOMI_ELEMENTWISE(i, j);
    if (status_has_stopped(stop_status[j])) return;
    const double om = beta[j] != 0.0 ? gamma[j] / beta[j] : 0.0;
    x[i * x_stride + j] += alpha[j] * y[i * y_stride + j] + om * z[i * z_stride + j];
    r[i * r_stride + j] = s[i * s_stride + j] - om * t[i * t_stride + j];
    if (i == 0) omega[j] = om;
}

// x += alpha * y for the columns that stopped but are not finalized yet ...
__global__ __launch_bounds__(block) void bicgstab_finalize_kernel(
    int64_t n, int64_t nrhs, double* __restrict__ x, int64_t x_stride,
    const double* __restrict__ y, int64_t y_stride, const double* __restrict__ alpha,
    const uint8_t* __restrict__ stop_status)
{
    GKOMI_ELEMENTWISE(i, j);
    const uint8_t st = stop_status[j];
    if (status_has_stopped(st) && !(st & finalized_mask)) {
        x[i * x_stride + j] += alpha[j] * y[i * y_stride + j];
    }
}

// ... which then become finalized (separate launch: every row reads the status)
__global__ __launch_bounds__(block) void finalize_status_kernel(int64_t nrhs, bool have_rows,
                                                                uint8_t* __restrict__ stop_status)
{
    const int64_t j = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x;
    if (j < nrhs && have_rows && status_has_stopped(stop_status[j])) stop_status[j] |= finalized_mask;
}

// ---- FCG ----------------------------------------------------------------------
__global__ __launch_bounds__(block) void fcg_initialize_kernel(
    int64_t n, int64_t nrhs, const double* __restrict__ b, int64_t b_stride,
    double* __restrict__ r, int64_t r_stride, double* __restrict__ z, int64_t z_stride,
    double* __restrict__ p, int64_t p_stride, double* __restrict__ q, int64_t q_stride,
    double* __restrict__ t, int64_t t_stride, double* __restrict__ prev_rho,
    double* __restrict__ rho, double* __restrict__ rho_t, uint8_t* __restrict__ stop_status)
{
    const int64_t idx = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x;
    if (idx < nrhs) {
        rho[idx] = 0.0;
        prev_rho[idx] = rho_t[idx] = 1.0;
        stop_status[idx] = 0;
    }
    if (idx >= n * nrhs) return;
    const int64_t i = idx / nrhs, j = idx - i * nrhs;
    t[i * t_stride + j] = r[i * r_stride + j] = b[i * b_stride + j];
    z[i * z_stride + j] = p[i * p_stride + j] = q[i * q_stride + j] = 0.0;
}

__global__ __launch_bounds__(block) void fcg_step_1_kernel(
    int64_t n, int64_t nrhs, double* __restrict__ p, int64_t p_stride,
    const double* __restrict__ z, int64_t z_stride, const double* __restrict__ rho_t,
    const double* __restrict__ prev_rho, const uint8_t* __restrict__ stop_status)
{
    GKOMI_ELEMENTWISE(i, j);
    if (status_has_stopped(stop_status[j])) return;
    if (prev_rho[j] == 0.0) {
        p[i * p_stride + j] = z[i * z_stride + j];
    } else {
        const double tmp = rho_t[j] / prev_rho[j];
        p[i * p_stride + j] = z[i * z_stride + j] + tmp * p[i * p_stride + j];
    }
}

__global__ __launch_bounds__(block) void fcg_step_2_kernel(
    int64_t n, int64_t nrhs, double* __restrict__ x, int64_t x_stride, double* __restrict__ r,
    int64_t r_stride, double* __restrict__ t, int64_t t_stride, const double* __restrict__ p,
    int64_t p_stride, const double* __restrict__ q, int64_t q_stride,
    const double* __restrict__ beta, const double* __restrict__ rho,
    const uint8_t* __restrict__ stop_status)
{
    GKOMI_ELEMENTWISE(i, j);
    if (status_has_stopped(stop_status[j])) return;
    if (beta[j] != 0.0) {
        const double tmp = rho[j] / beta[j];
        const double prev_r = r[i * r_stride + j];
        x[i * x_stride + j] += tmp * p[i * p_stride + j];
        const double new_r = prev_r - tmp * q[i * q_stride + j];
        r[i * r_stride + j] = new_r;
        t[i * t_stride + j] = new_r - prev_r;
    }
}

// ---- CGS ----------------------------------------------------------------------
__global__ __launch_bounds__(block) void cgs_initialize_kernel(
    int64_t n, int64_t nrhs, const double* __restrict__ b, int64_t b_stride,
    double* __restrict__ r, int64_t r_stride, double* __restrict__ r_tld, int64_t r_tld_stride,
    double* __restrict__ p, int64_t p_stride, double* __restrict__ q, int64_t q_stride,
    double* __restrict__ u, int64_t u_stride, double* __restrict__ u_hat, int64_t u_hat_stride,
    double* __restrict__ v_hat, int64_t v_hat_stride, double* __restrict__ t, int64_t t_stride,
    double* __restrict__ alpha, double* __restrict__ beta, double* __restrict__ gamma,
    double* __restrict__ prev_rho, double* __restrict__ rho, uint8_t* __restrict__ stop_status)
{
    const int64_t idx = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x;
    if (idx < nrhs) {
        rho[idx] = 0.0;
        prev_rho[idx] = alpha[idx] = beta[idx] = gamma[idx] = 1.0;
        stop_status[idx] = 0;
    }
    if (idx >= n * nrhs) return;
    const int64_t i = idx / nrhs, j = idx - i * nrhs;
    r[i * r_stride + j] = r_tld[i * r_tld_stride + j] = b[i * b_stride + j];
    u[i * u_stride + j] = u_hat[i * u_hat_stride + j] = p[i * p_stride + j] = q[i * q_stride + j] =
        v_hat[i * v_hat_stride + j] = t[i * t_stride + j] = 0.0;
}

// beta is rewritten only when prev_rho != 0, and then nobody reads the old value
__global__ __launch_bounds__(block) void cgs_step_1_kernel(
    int64_t n, int64_t nrhs, const double* __restrict__ r, int64_t r_stride,
    double* __restrict__ u, int64_t u_stride, double* __restrict__ p, int64_t p_stride,
    const double* __restrict__ q, int64_t q_stride, double* beta, const double* __restrict__ rho,
    const double* __restrict__ prev_rho, const uint8_t* __restrict__ stop_status)
{
    GKOMI_ELEMENTWISE(i, j);
    if (status_has_stopped(stop_status[j])) return;
    const bool update = prev_rho[j] != 0.0;
    const double bt = update ? rho[j] / prev_rho[j] : beta[j];
    const double uu = r[i * r_stride + j] + bt * q[i * q_stride + j];
    u[i * u_stride + j] = uu;
    p[i * p_stride + j] = uu + bt * (q[i * q_stride + j] + bt * p[i * p_stride + j]);
    if (i == 0 && update) beta[j] = bt;
}

__global__ __launch_bounds__(block) void cgs_step_2_kernel(
    int64_t n, int64_t nrhs, const double* __restrict__ u, int64_t u_stride,
    const double* __restrict__ v_hat, int64_t v_hat_stride, double* __restrict__ q,
    int64_t q_stride, double* __restrict__ t, int64_t t_stride, double* alpha,
    const double* __restrict__ rho, const double* __restrict__ gamma,
    const uint8_t* __restrict__ stop_status)
{
    GKOMI_ELEMENTWISE(i, j);
    if (status_has_stopped(stop_status[j])) return;
    const bool update = gamma[j] != 0.0;
    const double a = update ? rho[j] / gamma[j] : alpha[j];
    const double qq = u[i * u_stride + j] - a * v_hat[i * v_hat_stride + j];
    q[i * q_stride + j] = qq;
    t[i * t_stride + j] = u[i * u_stride + j] + qq;
    if (i == 0 && update) alpha[j] = a;
}

__global__ __launch_bounds__(block) void cgs_step_3_kernel(
    int64_t n, int64_t nrhs, const double* __restrict__ t, int64_t t_stride,
    const double* __restrict__ u_hat, int64_t u_hat_stride, double* __restrict__ r,
    int64_t r_stride, double* __restrict__ x, int64_t x_stride, const double* __restrict__ alpha,
    const uint8_t* __restrict__ stop_status)
{
    GKOMI_ELEMENTWISE(i, j);
    if (status_has_stopped(stop_status[j])) return;
    x[i * x_stride + j] += alpha[j] * u_hat[i * u_hat_stride + j];
    r[i * r_stride + j] -= alpha[j] * t[i * t_stride + j];
}

// ---- BiCG ---------------------------------------------------------------------
__global__ __launch_bounds__(block) void bicg_initialize_kernel(
    int64_t n, int64_t nrhs, const double* __restrict__ b, int64_t b_stride,
    double* __restrict__ r, int64_t r_stride, double* __restrict__ z, int64_t z_stride,
    double* __restrict__ p, int64_t p_stride, double* __restrict__ q, int64_t q_stride,
    double* __restrict__ prev_rho, double* __restrict__ rho, double* __restrict__ r2,
    int64_t r2_stride, double* __restrict__ z2, int64_t z2_stride, double* __restrict__ p2,
    int64_t p2_stride, double* __restrict__ q2, int64_t q2_stride,
    uint8_t* __restrict__ stop_status)
{
    const int64_t idx = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x;
    if (idx < nrhs) {
        rho[idx] = 0.0;
        prev_rho[idx] = 1.0;
        stop_status[idx] = 0;
    }
    if (idx >= n * nrhs) return;
    const int64_t i = idx / nrhs, j = idx - i * nrhs;
    r[i * r_stride + j] = r2[i * r2_stride + j] = b[i * b_stride + j];
    z[i * z_stride + j] = p[i * p_stride + j] = q[i * q_stride + j] = 0.0;
    z2[i * z2_stride + j] = p2[i * p2_stride + j] = q2[i * q2_stride + j] = 0.0;
}

__global__ __launch_bounds__(block) void bicg_step_1_kernel(
    int64_t n, int64_t nrhs, double* __restrict__ p, int64_t p_stride,
    const double* __restrict__ z, int64_t z_stride, double* __restrict__ p2, int64_t p2_stride,
    const double* __restrict__ z2, int64_t z2_stride, const double* __restrict__ rho,
    const double* __restrict__ prev_rho, const uint8_t* __restrict__ stop_status)
{
    GKOMI_ELEMENTWISE(i, j);
    if (status_has_stopped(stop_status[j])) return;
    if (prev_rho[j] == 0.0) {
        p[i * p_stride + j] = z[i * z_stride + j];
        p2[i * p2_stride + j] = z2[i * z2_stride + j];
    } else {
        const double tmp = rho[j] / prev_rho[j];
        p[i * p_stride + j] = z[i * z_stride + j] + tmp * p[i * p_stride + j];
        p2[i * p2_stride + j] = z2[i * z2_stride + j] + tmp * p2[i * p2_stride + j];
    }
}

__global__ __launch_bounds__(block) void bicg_step_2_kernel(
    int64_t n, int64_t nrhs, double* __restrict__ x, int64_t x_stride, double* __restrict__ r,
    int64_t r_stride, double* __restrict__ r2, int64_t r2_stride, const double* __restrict__ p,
    int64_t p_stride, const double* __restrict__ q, int64_t q_stride,
    const double* __restrict__ q2, int64_t q2_stride, const double* __restrict__ beta,
    const double* __restrict__ rho, const uint8_t* __restrict__ stop_status)
{
    GKOMI_ELEMENTWISE(i, j);
    if (status_has_stopped(stop_status[j])) return;
    if (beta[j] != 0.0) {
        const double tmp = rho[j] / beta[j];
        x[i * x_stride + j] += tmp * p[i * p_stride + j];
        r[i * r_stride + j] -= tmp * q[i * q_stride + j];
        r2[i * r2_stride + j] -= tmp * q2[i * q2_stride + j];
    }
}

__global__ __launch_bounds__(block) void ir_initialize_kernel(int64_t nrhs,
                                                              uint8_t* __restrict__ stop_status)
{
    const int64_t j = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x;
    if (j < nrhs) stop_status[j] = 0;
}

// the scalar updates of steps that define a scalar must also happen for n == 0
// (the reference loops over the columns first): tiny single-block kernels
__global__ void cgs_scalar_kernel(int64_t nrhs, double* out, const double* num, const double* den,
                                  const uint8_t* stop_status)
{
    for (int64_t j = threadIdx.x; j < nrhs; j += blockDim.x) {
        if (!status_has_stopped(stop_status[j]) && den[j] != 0.0) out[j] = num[j] / den[j];
    }
}
__global__ void bicgstab_omega_kernel(int64_t nrhs, double* omega, const double* gamma,
                                      const double* beta, const uint8_t* stop_status)
{
    for (int64_t j = threadIdx.x; j < nrhs; j += blockDim.x) {
        if (!status_has_stopped(stop_status[j])) omega[j] = beta[j] != 0.0 ? gamma[j] / beta[j] : 0.0;
    }
}

bool bad_dims(int64_t n, int64_t nrhs) { return n < 0 || nrhs < 0; }
dim3 grid_of(int64_t n, int64_t nrhs) { return dim3(static_cast<unsigned>(ceildiv(std::max<int64_t>(n * nrhs, nrhs), block))); }

// the request record, the workspace layout, the shared start and criterion, the fused drivers' host side: krylov_driver.hpp

}  // namespace
}  // namespace gkomi

using namespace gkomi;

// ---- kernel entry points ---------------------------------------------------------
extern "C" int gkomi_bicgstab_initialize_f64(
    gkomi_stream_t s, int64_t n, int64_t nrhs, const double* b, int64_t b_stride, double* r,
    int64_t r_stride, double* rr, int64_t rr_stride, double* y, int64_t y_stride, double* sv,
    int64_t s_stride, double* t, int64_t t_stride, double* z, int64_t z_stride, double* v,
    int64_t v_stride, double* p, int64_t p_stride, double* prev_rho, double* rho, double* alpha,
    double* beta, double* gamma, double* omega, uint8_t* stop_status)
{
    if (bad_dims(n, nrhs)) return GKOMI_EINVAL;
    if (nrhs == 0) return GKOMI_SUCCESS;
    hipLaunchKernelGGL(bicgstab_initialize_kernel, grid_of(n, nrhs), dim3(block), 0, to_stream(s), n,
                       nrhs, b, b_stride, r, r_stride, rr, rr_stride, y, y_stride, sv, s_stride, t,
                       t_stride, z, z_stride, v, v_stride, p, p_stride, prev_rho, rho, alpha, beta,
                       gamma, omega, stop_status);
    return check_launch();
}

extern "C" int gkomi_bicgstab_step_1_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, const double* r,
                                         int64_t r_stride, double* p, int64_t p_stride,
                                         const double* v, int64_t v_stride, const double* rho,
                                         const double* prev_rho, const double* alpha,
                                         const double* omega, const uint8_t* stop_status)
{
    if (bad_dims(n, nrhs)) return GKOMI_EINVAL;
    if (n == 0 || nrhs == 0) return GKOMI_SUCCESS;
    hipLaunchKernelGGL(bicgstab_step_1_kernel, grid_of(n, nrhs), dim3(block), 0, to_stream(s), n,
                       nrhs, r, r_stride, p, p_stride, v, v_stride, rho, prev_rho, alpha, omega,
                       stop_status);
    return check_launch();
}

extern "C" int gkomi_bicgstab_step_2_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, const double* r,
                                         int64_t r_stride, double* sv, int64_t s_stride,
                                         const double* v, int64_t v_stride, const double* rho,
                                         double* alpha, const double* beta,
                                         const uint8_t* stop_status)
{
    if (bad_dims(n, nrhs)) return GKOMI_EINVAL;
    if (n == 0 || nrhs == 0) return GKOMI_SUCCESS;  // the reference sets alpha inside the row loop
    hipLaunchKernelGGL(bicgstab_step_2_kernel, grid_of(n, nrhs), dim3(block), 0, to_stream(s), n,
                       nrhs, r, r_stride, sv, s_stride, v, v_stride, rho, alpha, beta, stop_status);
    return check_launch();
}

extern "C" int gkomi_bicgstab_step_3_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, double* x,
                                         int64_t x_stride, double* r, int64_t r_stride,
                                         const double* sv, int64_t s_stride, const double* t,
                                         int64_t t_stride, const double* y, int64_t y_stride,
                                         const double* z, int64_t z_stride, const double* alpha,
                                         const double* beta, const double* gamma, double* omega,
                                         const uint8_t* stop_status)
{
    if (bad_dims(n, nrhs)) return GKOMI_EINVAL;
    if (nrhs == 0) return GKOMI_SUCCESS;
    if (n == 0) {
        hipLaunchKernelGGL(bicgstab_omega_kernel, dim3(1), dim3(block), 0, to_stream(s), nrhs, omega,
                           gamma, beta, stop_status);
        return check_launch();
    }
    hipLaunchKernelGGL(bicgstab_step_3_kernel, grid_of(n, nrhs), dim3(block), 0, to_stream(s), n,
                       nrhs, x, x_stride, r, r_stride, sv, s_stride, t, t_stride, y, y_stride, z,
                       z_stride, alpha, beta, gamma, omega, stop_status);
    return check_launch();
}

extern "C" int gkomi_bicgstab_finalize_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, double* x,
                                           int64_t x_stride, const double* y, int64_t y_stride,
                                           const double* alpha, uint8_t* stop_status)
{
    if (bad_dims(n, nrhs)) return GKOMI_EINVAL;
    if (nrhs == 0) return GKOMI_SUCCESS;
    hipStream_t stream = to_stream(s);
    if (n > 0) {
        hipLaunchKernelGGL(bicgstab_finalize_kernel, grid_of(n, nrhs), dim3(block), 0, stream, n,
                           nrhs, x, x_stride, y, y_stride, alpha, stop_status);
    }
    // the reference finalizes inside the row loop: nothing happens for n == 0
    hipLaunchKernelGGL(finalize_status_kernel, dim3(static_cast<unsigned>(ceildiv(nrhs, block))),
                       dim3(block), 0, stream, nrhs, n > 0, stop_status);
    return check_launch();
}

extern "C" int gkomi_fcg_initialize_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, const double* b,
                                        int64_t b_stride, double* r, int64_t r_stride, double* z,
                                        int64_t z_stride, double* p, int64_t p_stride, double* q,
                                        int64_t q_stride, double* t, int64_t t_stride,
                                        double* prev_rho, double* rho, double* rho_t,
                                        uint8_t* stop_status)
{
    if (bad_dims(n, nrhs)) return GKOMI_EINVAL;
    if (nrhs == 0) return GKOMI_SUCCESS;
    hipLaunchKernelGGL(fcg_initialize_kernel, grid_of(n, nrhs), dim3(block), 0, to_stream(s), n, nrhs,
                       b, b_stride, r, r_stride, z, z_stride, p, p_stride, q, q_stride, t, t_stride,
                       prev_rho, rho, rho_t, stop_status);
    return check_launch();
}

extern "C" int gkomi_fcg_step_1_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, double* p,
                                    int64_t p_stride, const double* z, int64_t z_stride,
                                    const double* rho_t, const double* prev_rho,
                                    const uint8_t* stop_status)
{
    if (bad_dims(n, nrhs)) return GKOMI_EINVAL;
    if (n == 0 || nrhs == 0) return GKOMI_SUCCESS;
    hipLaunchKernelGGL(fcg_step_1_kernel, grid_of(n, nrhs), dim3(block), 0, to_stream(s), n, nrhs, p,
                       p_stride, z, z_stride, rho_t, prev_rho, stop_status);
    return check_launch();
}

extern "C" int gkomi_fcg_step_2_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, double* x,
                                    int64_t x_stride, double* r, int64_t r_stride, double* t,
                                    int64_t t_stride, const double* p, int64_t p_stride,
                                    const double* q, int64_t q_stride, const double* beta,
                                    const double* rho, const uint8_t* stop_status)
{
    if (bad_dims(n, nrhs)) return GKOMI_EINVAL;
    if (n == 0 || nrhs == 0) return GKOMI_SUCCESS;
    hipLaunchKernelGGL(fcg_step_2_kernel, grid_of(n, nrhs), dim3(block), 0, to_stream(s), n, nrhs, x,
                       x_stride, r, r_stride, t, t_stride, p, p_stride, q, q_stride, beta, rho,
                       stop_status);
    return check_launch();
}

extern "C" int gkomi_cgs_initialize_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, const double* b,
                                        int64_t b_stride, double* r, int64_t r_stride,
                                        double* r_tld, int64_t r_tld_stride, double* p,
                                        int64_t p_stride, double* q, int64_t q_stride, double* u,
                                        int64_t u_stride, double* u_hat, int64_t u_hat_stride,
                                        double* v_hat, int64_t v_hat_stride, double* t,
                                        int64_t t_stride, double* alpha, double* beta,
                                        double* gamma, double* prev_rho, double* rho,
                                        uint8_t* stop_status)
{
    if (bad_dims(n, nrhs)) return GKOMI_EINVAL;
    if (nrhs == 0) return GKOMI_SUCCESS;
    hipLaunchKernelGGL(cgs_initialize_kernel, grid_of(n, nrhs), dim3(block), 0, to_stream(s), n, nrhs,
                       b, b_stride, r, r_stride, r_tld, r_tld_stride, p, p_stride, q, q_stride, u,
                       u_stride, u_hat, u_hat_stride, v_hat, v_hat_stride, t, t_stride, alpha, beta,
                       gamma, prev_rho, rho, stop_status);
    return check_launch();
}

extern "C" int gkomi_cgs_step_1_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, const double* r,
                                    int64_t r_stride, double* u, int64_t u_stride, double* p,
                                    int64_t p_stride, const double* q, int64_t q_stride,
                                    double* beta, const double* rho, const double* prev_rho,
                                    const uint8_t* stop_status)
{
    if (bad_dims(n, nrhs)) return GKOMI_EINVAL;
    if (nrhs == 0) return GKOMI_SUCCESS;
    if (n == 0) {
        hipLaunchKernelGGL(cgs_scalar_kernel, dim3(1), dim3(block), 0, to_stream(s), nrhs, beta, rho,
                           prev_rho, stop_status);
        return check_launch();
    }
    hipLaunchKernelGGL(cgs_step_1_kernel, grid_of(n, nrhs), dim3(block), 0, to_stream(s), n, nrhs, r,
                       r_stride, u, u_stride, p, p_stride, q, q_stride, beta, rho, prev_rho,
                       stop_status);
    return check_launch();
}

extern "C" int gkomi_cgs_step_2_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, const double* u,
                                    int64_t u_stride, const double* v_hat, int64_t v_hat_stride,
                                    double* q, int64_t q_stride, double* t, int64_t t_stride,
                                    double* alpha, const double* rho, const double* gamma,
                                    const uint8_t* stop_status)
{
    if (bad_dims(n, nrhs)) return GKOMI_EINVAL;
    if (nrhs == 0) return GKOMI_SUCCESS;
    if (n == 0) {
        hipLaunchKernelGGL(cgs_scalar_kernel, dim3(1), dim3(block), 0, to_stream(s), nrhs, alpha, rho,
                           gamma, stop_status);
        return check_launch();
    }
    hipLaunchKernelGGL(cgs_step_2_kernel, grid_of(n, nrhs), dim3(block), 0, to_stream(s), n, nrhs, u,
                       u_stride, v_hat, v_hat_stride, q, q_stride, t, t_stride, alpha, rho, gamma,
                       stop_status);
    return check_launch();
}

extern "C" int gkomi_cgs_step_3_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, const double* t,
                                    int64_t t_stride, const double* u_hat, int64_t u_hat_stride,
                                    double* r, int64_t r_stride, double* x, int64_t x_stride,
                                    const double* alpha, const uint8_t* stop_status)
{
    if (bad_dims(n, nrhs)) return GKOMI_EINVAL;
    if (n == 0 || nrhs == 0) return GKOMI_SUCCESS;
    hipLaunchKernelGGL(cgs_step_3_kernel, grid_of(n, nrhs), dim3(block), 0, to_stream(s), n, nrhs, t,
                       t_stride, u_hat, u_hat_stride, r, r_stride, x, x_stride, alpha, stop_status);
    return check_launch();
}

// ---- drivers ------------------------------------------------------------------------
extern "C" size_t gkomi_krylov_workspace_bytes(int64_t n, int64_t nrhs)
{
    if (n < 0 || nrhs <= 0) return 0;
    return make_solver_layout(n, nrhs, 8).total;
}

namespace {
int bicgstab_solve_impl(const solve_request& req)
{
    driver_common c;
    GKOMI_TRY(c.init(req, 10));
    const gkomi_stream_t s = c.s;
    const int64_t n = c.n, nrhs = c.nrhs;
    double *x = req.x, *sc = c.scalars;
    double *r = c.vec(0), *z = c.vec(1), *y = c.vec(2), *v = c.vec(3), *sv = c.vec(4), *t = c.vec(5), *p = c.vec(6),
           *rr = c.vec(7);
    double *alpha = sc, *beta = sc + nrhs, *gamma = sc + 2 * nrhs, *prev_rho = sc + 3 * nrhs,
           *rho = sc + 4 * nrhs, *omega = sc + 5 * nrhs;
    GKOMI_TRY(gkomi_bicgstab_initialize_f64(s, n, nrhs, req.b, nrhs, r, nrhs, rr, nrhs, y, nrhs, sv, nrhs,
                                            t, nrhs, z, nrhs, v, nrhs, p, nrhs, prev_rho, rho, alpha,
                                            beta, gamma, omega, c.stop_status));
    GKOMI_TRY(c.start(req, r));
    GKOMI_TRY(gkomi_dense_copy_f64(s, n, nrhs, r, nrhs, rr, nrhs));
    int64_t iter = -1;
    while (true) {
        ++iter;
        GKOMI_TRY(c.dot(rr, r, rho));
        bool stop = false;
        GKOMI_TRY(c.check(iter, r, true, 1, &stop));
        if (stop) break;
        GKOMI_TRY(gkomi_bicgstab_step_1_f64(s, n, nrhs, r, nrhs, p, nrhs, v, nrhs, rho, prev_rho,
                                            alpha, omega, c.stop_status));
        GKOMI_TRY(c.apply_precond(p, y));
        GKOMI_TRY(c.spmv(y, v));
        GKOMI_TRY(c.dot(rr, v, beta));
        GKOMI_TRY(gkomi_bicgstab_step_2_f64(s, n, nrhs, r, nrhs, sv, nrhs, v, nrhs, rho, alpha, beta,
                                            c.stop_status));
        GKOMI_TRY(c.check(iter, sv, false, 2, &stop));
        // the reference finalizes "if (one_changed)"; the kernel only touches
        // columns that stopped without being finalized, so calling it always
        // is the same thing without asking the host
        GKOMI_TRY(gkomi_bicgstab_finalize_f64(s, n, nrhs, x, nrhs, y, nrhs, alpha, c.stop_status));
        if (stop) break;
        GKOMI_TRY(c.apply_precond(sv, z));
        GKOMI_TRY(c.spmv(z, t));
        GKOMI_TRY(c.dot(sv, t, gamma));
        GKOMI_TRY(c.dot(t, t, beta));
        GKOMI_TRY(gkomi_bicgstab_step_3_f64(s, n, nrhs, x, nrhs, r, nrhs, sv, nrhs, t, nrhs, y, nrhs,
                                            z, nrhs, alpha, beta, gamma, omega, c.stop_status));
        std::swap(prev_rho, rho);
    }
    return c.finish(c.stop_iter(), c.host_record.phase == 2 ? sv : r, req.host_info);
}


// ---- fused BiCGSTAB, one right-hand side --------------------------------------------
//
// The reference sequence above costs 25 launches per iteration (two-stage dots,
// the criterion, the step kernels).  The fused driver keeps the same recurrences
// and check points in 5 launches (+ the preconditioner's):
//   KA  re-adds the partials of rho = rr.r and |r|^2 left by KE, evaluates the
//       criterion on r (phase 1) and -- unless stopped -- updates p (step_1)
//   KB  v = A y with the partials of rr.v in the SpMV epilogue
//   KC  re-adds them: alpha, s = r - alpha v (step_2), partials of |s|^2
//   KD  t = A z with the partials of s.t and t.t in the epilogue
//   KE  first re-adds the partials of |s|^2 and evaluates the criterion on s (phase 2; a launch of its own until
//       round 3: 4.8 us per iteration): if it fires, x += alpha y (finalize) and nothing else -- KD ran once for
//       nothing; otherwise re-adds KD's: omega, x += alpha y + omega z, r = s - omega t (step_3), partials of rr.r
//       and |r|^2 for the next KA
// Every workgroup re-adds the partials in the same order, so all agree on the
// scalars bit for bit; workgroup 0 stores them for the kernels that follow.
// Once a criterion fires the remaining launches return at once, so x and the
// iteration count are those of the stopping iteration whatever `check_every`.
// The sweep, the criterion and the partial sums are those of fused_krylov.hpp; these kernels report id 1 for both criteria.
struct bicgstab_scalars : fused_scalars {
    double alpha, omega;
    long long stop2_iter;   // iteration whose half step converged (written by KE only), -1 before
    int phase;
    unsigned char status2;  // written by KE only (the half step's criterion); `status` by KA only
    unsigned char pad2[3];
    unsigned final_status() const { return status | status2; }
};

__device__ __forceinline__ bool fused_stopped(const bicgstab_scalars* scal)
{
    return status_has_stopped(scal->status) || status_has_stopped(scal->status2);
}

__global__ void bicgstab_fused_init_kernel(bicgstab_scalars* scal, const double* orig_tau)
{
    init_fused_scalars(scal, 1.0, orig_tau[0]);  // prev_rho = rho = alpha = omega = 1 (bicgstab::initialize)
    scal->alpha = 1.0;
    scal->omega = 1.0;
    scal->stop2_iter = -1;
    scal->phase = 0;
    scal->status2 = 0;
}

// pa[block] = sum a*b, pb[block] = sum c*c over the workgroup's share (pb optional).
// (8 B per lane, one accumulator per sum: not cg_dot2_partials_kernel of cg_fused.hpp, whose sums associate differently.)
__global__ __launch_bounds__(fblock) void fused_dot2_partials_kernel(
    int64_t n, const double* __restrict__ a, const double* __restrict__ b,
    const double* __restrict__ c, const bicgstab_scalars* scal, double* __restrict__ pa,
    double* __restrict__ pb)
{
    __shared__ double smem[fblock / wave_size];
    if (scal != nullptr && fused_stopped(scal)) return;
    const int64_t step = static_cast<int64_t>(gridDim.x) * fblock;
    double u = 0.0, w = 0.0;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(fblock) + threadIdx.x; i < n; i += step) {
        u += a[i] * b[i];
        if (pb != nullptr) {
            const double cv = c[i];
            w += cv * cv;
        }
    }
    const double sum[] = {u, w};
    double* const part[] = {pa, pb};
    store_block_sums(false, sum, part, smem);
}

// KA
__global__ __launch_bounds__(fblock) void bicgstab_fused_step1_kernel(
    int64_t n, const double* __restrict__ r, double* __restrict__ p, const double* __restrict__ v,
    const double* __restrict__ rho_part, const double* __restrict__ tau_part, int nparts,
    bicgstab_scalars* scal, long long it, long long max_iters, double goal, host_watch_line* watch = nullptr)
{
    __shared__ double smem[fblock / wave_size];
    if (fused_stopped_before(fused_stopped(scal), scal, watch, it)) return;
    const pair_sweep sw(n);
    const double* const in[] = {r, p, v};
    double* const out[] = {p};
    const auto first = sw.prefetch(in);
    const double rho = sum_partials(rho_part, nparts, smem);
    const double tau = sqrt(sum_partials(tau_part, nparts, smem));
    const double prev = scal->rho[(it + 1) & 1];
    const double alpha = scal->alpha, omega = scal->omega;
    if (fused_criterion(scal, watch, it, max_iters, rho, tau, goal, 1, 1, [&](uint8_t st) {
            if (st) scal->phase = 1;
        })) {
        return;
    }
    // bicgstab::step_1 (reference/solver/bicgstab_kernels.cpp)
    const bool update = prev * omega != 0.0;
    const double tmp = update ? rho / prev * alpha / omega : 0.0;
    sw.run(first, in, out, true,
           [&](int, const double* e, double* o) { o[0] = update ? e[0] + tmp * (e[1] - omega * e[2]) : e[0]; });
}

// KC
__global__ __launch_bounds__(fblock) void bicgstab_fused_step2_kernel(
    int64_t n, const double* __restrict__ r, double* __restrict__ sv, const double* __restrict__ v,
    const double* __restrict__ beta_part, int nparts, bicgstab_scalars* scal, long long it,
    double* __restrict__ ss_part)
{
    __shared__ double smem[fblock / wave_size];
    if (fused_stopped(scal)) return;
    const pair_sweep sw(n);
    const double* const in[] = {r, v};
    double* const out[] = {sv};
    const auto first = sw.prefetch(in);
    const double beta = sum_partials(beta_part, nparts, smem);
    const double rho = scal->rho[it & 1];
    const bool update = beta != 0.0;
    const double alpha = update ? rho / beta : 0.0;
    if (fused_leader()) scal->alpha = alpha;
    // bicgstab::step_2; s.s of .x and of .y apart, the tail with .x
    double acc[2] = {0.0, 0.0};
    sw.run(first, in, out, true, [&](int half, const double* e, double* o) {
        o[0] = update ? e[0] - alpha * e[1] : e[0];
        acc[half] += o[0] * o[0];
    });
    const double sum[] = {acc[0] + acc[1]};
    double* const part[] = {ss_part};
    store_block_sums(true, sum, part, smem);
}

// KE
__global__ __launch_bounds__(fblock) void bicgstab_fused_step3_kernel(
    int64_t n, double* __restrict__ x, double* __restrict__ r, const double* __restrict__ sv,
    const double* __restrict__ t, const double* __restrict__ y, const double* __restrict__ z,
    const double* __restrict__ rr, const double* __restrict__ gamma_part,
    const double* __restrict__ tt_part, int nparts, bicgstab_scalars* scal,
    double* __restrict__ rho_part, double* __restrict__ tau_part,
    const double* __restrict__ ss_part, int nss, long long it, double goal)
{
    __shared__ double smem[fblock / wave_size];
    if (status_has_stopped(scal->status)) return;
    // the half step's criterion (KD0 of round 1 was a launch of its own: 4.8 us per iteration for a kernel that moves
    // data once per solve).  status2 / stop2_iter are written here: workgroup 0 may be writing them while a late
    // workgroup of the same launch starts, so "stopped in an earlier launch" is read from the one 8-byte word
    const long long stopped_at = scal->stop2_iter;
    if (stopped_at >= 0 && stopped_at != it) return;
    const pair_sweep sw(n);
    const double* const in[] = {x, y, z, sv, t, rr};
    const auto first = sw.prefetch(in);
    const double tau_s = sqrt(sum_partials(ss_part, nss, smem));
    if (tau_s < goal * scal->orig_tau) {
        // bicgstab::finalize (core/solver/bicgstab.cpp:196-203): s has converged, x += alpha y and nothing else
        // (the preconditioner apply and the SpMV between step 2 and here ran on that s for nothing, once per solve)
        const double alpha = scal->alpha;
        if (fused_leader()) {
            scal->tau = tau_s;
            scal->stop_iter = it;
            scal->stop2_iter = it;
            scal->phase = 2;
            scal->status2 = GKOMI_STATUS_CONVERGED | 1 | GKOMI_STATUS_FINALIZED;
        }
        const double* const fin[] = {x, y};
        double* const fout[] = {x};
        const pair_values<2> ffirst{{first.v[0], first.v[1]}};
        sw.run(ffirst, fin, fout, true, [&](int, const double* e, double* o) { o[0] = e[0] + alpha * e[1]; });
        return;
    }
    const double gamma = sum_partials(gamma_part, nparts, smem);
    const double beta = sum_partials(tt_part, nparts, smem);
    const double omega = beta != 0.0 ? gamma / beta : 0.0;
    const double alpha = scal->alpha;
    if (fused_leader()) scal->omega = omega;
    // bicgstab::step_3; rr.r and r.r, both halves and the tail into the same two accumulators
    double acc[2] = {0.0, 0.0};
    double* const out[] = {x, r};
    sw.run(first, in, out, true, [&](int, const double* e, double* o) {
        o[0] = e[0] + (alpha * e[1] + omega * e[2]);
        o[1] = e[3] - omega * e[4];
        acc[0] += e[5] * o[1];
        acc[1] += o[1] * o[1];
    });
    double* const part[] = {rho_part, tau_part};
    store_block_sums(true, acc, part, smem);
}

int bicgstab_fused_impl(const solve_request& req)
{
    bool reference;
    GKOMI_TRY(fused_preflight(req, &reference));
    if (reference) return bicgstab_solve_impl(req);
    driver_common c;
    GKOMI_TRY(c.init(req, 10));
    const gkomi_stream_t s = c.s;
    const int64_t n = c.n;
    const sysmat& A = c.A;
    double *x = req.x, *sc = c.scalars;
    double *r = c.vec(0), *z = c.vec(1), *y = c.vec(2), *v = c.vec(3), *sv = c.vec(4), *t = c.vec(5), *p = c.vec(6),
           *rr = c.vec(7);
    GKOMI_TRY(gkomi_bicgstab_initialize_f64(s, n, 1, req.b, 1, r, 1, rr, 1, y, 1, sv, 1, t, 1, z, 1, v, 1, p,
                                            1, sc, sc + 1, sc + 2, sc + 3, sc + 4, sc + 5,
                                            c.stop_status));
    GKOMI_TRY(c.start(req, r));
    GKOMI_TRY(gkomi_dense_copy_f64(s, n, 1, r, 1, rr, 1));
    hipStream_t stream = c.stream;
    fused_driver<bicgstab_scalars> f(c);
    bicgstab_scalars* scal = f.scal;
    double *part_rho = f.vec_partials(), *part_tau = f.vec_partials(), *part_ss = f.vec_partials();
    double *part_beta = f.spmv_partials(), *part_gamma = f.spmv_partials(), *part_tt = f.spmv_partials();
    const int g = f.g, nb = f.nb;
    const spmv_dot_plan& spmv = f.spmv;
    const bool csr_epilogue = spmv.fused();
    if (c.precond == nullptr) {  // Identity: y = p, z = s without the copies
        y = p;
        z = sv;
    }
    hipLaunchKernelGGL(bicgstab_fused_init_kernel, dim3(1), dim3(1), 0, stream, scal, c.orig_tau);
    hipLaunchKernelGGL(fused_dot2_partials_kernel, dim3(g), dim3(fblock), 0, stream, n, rr, r, r,
                       static_cast<const bicgstab_scalars*>(nullptr), part_rho, part_tau);
    GKOMI_TRY(check_launch());
    // q = A in, partials of w.q (and q.q) -- in the SpMV epilogue when A is CSR
    auto spmv_dots = [&](const double* in, double* out, const double* w, double* pw, double* pq) {
        if (csr_epilogue) {
            return spmv.launch(stream, in, out, pw, &scal->status, w, pq);
        }
        GKOMI_TRY(A.apply(s, 1, nullptr, in, nullptr, out));
        hipLaunchKernelGGL(fused_dot2_partials_kernel, dim3(g), dim3(fblock), 0, stream, n, w, out,
                           out, static_cast<const bicgstab_scalars*>(scal), pw, pq);
        return check_launch();
    };
    host_watch& watch = f.watch;
    auto issue = [&](long long it, bool last) -> int {
        hipLaunchKernelGGL(bicgstab_fused_step1_kernel, dim3(g), dim3(fblock), 0, stream, n, r, p, v,
                           part_rho, part_tau, g, scal, it, static_cast<long long>(c.max_iters),
                           c.reduction, watch.dev);
        if (last) return check_launch();
        if (c.precond != nullptr) GKOMI_TRY(c.apply_precond(p, y));
        GKOMI_TRY(spmv_dots(y, v, rr, part_beta, nullptr));
        hipLaunchKernelGGL(bicgstab_fused_step2_kernel, dim3(g), dim3(fblock), 0, stream, n, r, sv,
                           v, part_beta, nb, scal, it, part_ss);
        if (c.precond != nullptr) GKOMI_TRY(c.apply_precond(sv, z));
        GKOMI_TRY(spmv_dots(z, t, sv, part_gamma, part_tt));
        hipLaunchKernelGGL(bicgstab_fused_step3_kernel, dim3(g), dim3(fblock), 0, stream, n, x, r,
                           sv, t, y, z, rr, part_gamma, part_tt, nb, scal, part_rho, part_tau, part_ss, g, it,
                           c.reduction);
        return check_launch();
    };
    return f.solve(issue, req.host_info);
}

}  // namespace

extern "C" int gkomi_bicgstab_solve_fused_f64_i32(
    gkomi_stream_t s, int64_t n, int64_t nnz, const int32_t* row_ptrs, const int32_t* col_idxs,
    const double* vals, int spmv_strategy, int64_t max_row_nnz_hint, gkomi_apply_fn precond,
    void* precond_ctx, const double* b, double* x, int64_t max_iters, double reduction_factor,
    int baseline, int64_t check_every, void* workspace, size_t workspace_bytes, double* host_info)
{
    return bicgstab_fused_impl({s, n, 1, make_csr_sysmat(n, nnz, row_ptrs, col_idxs, vals, spmv_strategy, max_row_nnz_hint),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, check_every, workspace, workspace_bytes,
        host_info});
}

extern "C" int gkomi_bicgstab_solve_fused_op_f64(
    gkomi_stream_t s, int64_t n, gkomi_matrix_apply_fn matrix, void* matrix_ctx,
    gkomi_apply_fn precond, void* precond_ctx, const double* b, double* x, int64_t max_iters,
    double reduction_factor, int baseline, int64_t check_every, void* workspace,
    size_t workspace_bytes, double* host_info)
{
    if (matrix == nullptr) return GKOMI_EINVAL;
    return bicgstab_fused_impl({s, n, 1, make_op_sysmat(n, matrix, matrix_ctx),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, check_every, workspace, workspace_bytes,
        host_info});
}

extern "C" int gkomi_bicgstab_solve_f64_i32(
    gkomi_stream_t s, int64_t n, int64_t nrhs, int64_t nnz, const int32_t* row_ptrs,
    const int32_t* col_idxs, const double* vals, int spmv_strategy, int64_t max_row_nnz_hint,
    gkomi_apply_fn precond, void* precond_ctx, const double* b, double* x, int64_t max_iters,
    double reduction_factor, int baseline, int64_t check_every, void* workspace,
    size_t workspace_bytes, double* host_info)
{
    return bicgstab_solve_impl({s, n, nrhs,
        make_csr_sysmat(n, nnz, row_ptrs, col_idxs, vals, spmv_strategy, max_row_nnz_hint),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, check_every, workspace, workspace_bytes,
        host_info});
}

extern "C" int gkomi_bicgstab_solve_op_f64(gkomi_stream_t s, int64_t n, int64_t nrhs,
                                        gkomi_matrix_apply_fn matrix, void* matrix_ctx,
                                        gkomi_apply_fn precond, void* precond_ctx, const double* b,
                                        double* x, int64_t max_iters, double reduction_factor,
                                        int baseline, int64_t check_every, void* workspace,
                                        size_t workspace_bytes, double* host_info)
{
    if (matrix == nullptr) return GKOMI_EINVAL;
    return bicgstab_solve_impl({s, n, nrhs, make_op_sysmat(n, matrix, matrix_ctx),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, check_every, workspace, workspace_bytes,
        host_info});
}

namespace {
int fcg_solve_impl(const solve_request& req)
{
    driver_common c;
    GKOMI_TRY(c.init(req, 7));
    const gkomi_stream_t s = c.s;
    const int64_t n = c.n, nrhs = c.nrhs;
    double *x = req.x, *sc = c.scalars;
    double *r = c.vec(0), *z = c.vec(1), *p = c.vec(2), *q = c.vec(3), *t = c.vec(4);
    double *beta = sc, *prev_rho = sc + nrhs, *rho = sc + 2 * nrhs, *rho_t = sc + 3 * nrhs;
    GKOMI_TRY(gkomi_fcg_initialize_f64(s, n, nrhs, req.b, nrhs, r, nrhs, z, nrhs, p, nrhs, q, nrhs, t,
                                       nrhs, prev_rho, rho, rho_t, c.stop_status));
    GKOMI_TRY(c.start(req, r));
    int64_t iter = -1;
    while (true) {
        GKOMI_TRY(c.apply_precond(r, z));
        GKOMI_TRY(c.dot(r, z, rho));
        GKOMI_TRY(c.dot(t, z, rho_t));
        ++iter;
        bool stop = false;
        GKOMI_TRY(c.check(iter, r, true, 1, &stop));
        if (stop) break;
        GKOMI_TRY(gkomi_fcg_step_1_f64(s, n, nrhs, p, nrhs, z, nrhs, rho_t, prev_rho, c.stop_status));
        GKOMI_TRY(c.spmv(p, q));
        GKOMI_TRY(c.dot(p, q, beta));
        GKOMI_TRY(gkomi_fcg_step_2_f64(s, n, nrhs, x, nrhs, r, nrhs, t, nrhs, p, nrhs, q, nrhs, beta,
                                       rho, c.stop_status));
        std::swap(prev_rho, rho);
    }
    return c.finish(c.stop_iter(), r, req.host_info);
}

}  // namespace

// ---- fused FCG, one right-hand side: 3 launches per iteration -----------------------
// (the structure of the fused CG of cg_solver.hip plus the vector t = r_new - r_old)
//   FA  re-adds the partials of rho = r.z, rho_t = t.z and |r|^2, evaluates the
//       criterion, p = z + (rho_t / prev_rho) p (fcg::step_1)
//   FB  q = A p with the p.q partials in the SpMV epilogue
//   FC  beta -> x += (rho/beta) p, r -= (rho/beta) q, t = r_new - r_old
//       (fcg::step_2) and, without a preconditioner (z = r), the partials for
//       the next FA; with one: z = M r, then a three-dot partials kernel
namespace {

struct fcg_scalars : fused_scalars {};

__global__ void fcg_fused_init_kernel(fcg_scalars* scal, const double* orig_tau)
{
    init_fused_scalars(scal, 0.0, orig_tau[0]);  // prev_rho = 1 (fcg::initialize)
}

// p0[b] = sum r*z, p1[b] = sum t*z, p2[b] = sum r*r
__global__ __launch_bounds__(fblock) void fused_dot3_partials_kernel(
    int64_t n, const double* __restrict__ r, const double* __restrict__ z, const double* __restrict__ t,
    const unsigned char* status, double* __restrict__ p0, double* __restrict__ p1,
    double* __restrict__ p2)
{
    __shared__ double smem[fblock / wave_size];
    if (status != nullptr && status_has_stopped(status[0])) return;
    double sum[3] = {0.0, 0.0, 0.0};
    const bool vec = ((reinterpret_cast<uintptr_t>(r) | reinterpret_cast<uintptr_t>(z) |
                       reinterpret_cast<uintptr_t>(t)) & 15) == 0;
    if (vec) {  // 16 B per lane
        const pair_sweep sw(n);
        const double* const in[] = {r, z, t};
        double a[2] = {0.0, 0.0}, b[2] = {0.0, 0.0}, c[2] = {0.0, 0.0};
        auto dots = [&](int half, const double* e) {
            a[half] += e[0] * e[1];
            b[half] += e[2] * e[1];
            c[half] += e[0] * e[0];
        };
        sw.loop(sw.i0, in, dots);
        // the halves are joined before the tail is added
        a[0] += a[1];
        b[0] += b[1];
        c[0] += c[1];
        sw.tail(in, dots);
        sum[0] = a[0];
        sum[1] = b[0];
        sum[2] = c[0];
    } else {
        const int64_t step = static_cast<int64_t>(gridDim.x) * fblock;
        for (int64_t i = blockIdx.x * static_cast<int64_t>(fblock) + threadIdx.x; i < n; i += step) {
            const double rv = r[i], zv = z[i];
            sum[0] += rv * zv;
            sum[1] += t[i] * zv;
            sum[2] += rv * rv;
        }
    }
    double* const part[] = {p0, p1, p2};
    store_block_sums(false, sum, part, smem);
}

// FA.  z may alias r (Identity).
__global__ __launch_bounds__(fblock) void fcg_fused_step1_kernel(
    int64_t n, double* __restrict__ p, const double* __restrict__ z,
    const double* __restrict__ rho_part, const double* __restrict__ rhot_part,
    const double* __restrict__ tau_part, int nparts, fcg_scalars* scal, long long it,
    long long max_iters, double goal, host_watch_line* watch = nullptr)
{
    __shared__ double smem[fblock / wave_size];
    if (fused_stopped_before(status_has_stopped(scal->status), scal, watch, it)) return;
    const pair_sweep sw(n);
    const double* const in[] = {z, p};
    double* const out[] = {p};
    const auto first = sw.prefetch(in);
    const double rho = sum_partials(rho_part, nparts, smem);
    const double rho_t = sum_partials(rhot_part, nparts, smem);
    const double tau = sqrt(rho_part == tau_part ? rho : sum_partials(tau_part, nparts, smem));
    const double prev = scal->rho[(it + 1) & 1];
    if (fused_criterion(scal, watch, it, max_iters, rho, tau, goal, 1, 1)) return;
    // fcg::step_1
    const bool restart = prev == 0.0;
    const double tmp = restart ? 0.0 : rho_t / prev;
    sw.run(first, in, out, true, [&](int, const double* e, double* o) { o[0] = restart ? e[0] : e[0] + tmp * e[1]; });
}

// FC.  With partials != nullptr (Identity): leaves r.r and t.r of the new r, t.
__global__ __launch_bounds__(fblock) void fcg_fused_step2_kernel(
    int64_t n, double* __restrict__ x, double* __restrict__ r, double* __restrict__ t,
    const double* __restrict__ p, const double* __restrict__ q,
    const double* __restrict__ beta_part, int nparts, fcg_scalars* scal, long long it,
    double* __restrict__ rr_part, double* __restrict__ tr_part)
{
    __shared__ double smem[fblock / wave_size];
    if (status_has_stopped(scal->status)) return;
    const pair_sweep sw(n);
    const double* const in[] = {x, r, t, p, q};
    double* const out[] = {x, r, t};
    const auto first = sw.prefetch(in);
    const double beta = sum_partials(beta_part, nparts, smem);
    const double rho = scal->rho[it & 1];
    const bool update = beta != 0.0;
    const double tmp = update ? rho / beta : 0.0;
    // fcg::step_2; r.r and t.r, both halves and the tail into the same two accumulators (beta == 0: nothing is written)
    double acc[2] = {0.0, 0.0};
    sw.run(first, in, out, update, [&](int, const double* e, double* o) {
        double xv = e[0], rv = e[1], tv = e[2];
        if (update) {
            const double prev_r = rv;
            xv += tmp * e[3];
            rv = prev_r - tmp * e[4];
            tv = rv - prev_r;
        }
        o[0] = xv;
        o[1] = rv;
        o[2] = tv;
        acc[0] += rv * rv;
        acc[1] += tv * rv;
    });
    if (rr_part == nullptr) return;
    double* const part[] = {rr_part, tr_part};
    store_block_sums(true, acc, part, smem);
}

int fcg_fused_impl(const solve_request& req)
{
    bool reference;
    GKOMI_TRY(fused_preflight(req, &reference));
    if (reference) return fcg_solve_impl(req);
    driver_common c;
    GKOMI_TRY(c.init(req, 7));
    const gkomi_stream_t s = c.s;
    const int64_t n = c.n;
    const sysmat& A = c.A;
    double *x = req.x, *sc = c.scalars;
    double *r = c.vec(0), *z = c.vec(1), *p = c.vec(2), *q = c.vec(3), *t = c.vec(4);
    GKOMI_TRY(gkomi_fcg_initialize_f64(s, n, 1, req.b, 1, r, 1, z, 1, p, 1, q, 1, t, 1, sc + 1, sc + 2, sc + 3,
                                       c.stop_status));
    GKOMI_TRY(c.start(req, r));
    // t = b from initialize, exactly like the reference (fcg.cpp:137 does not refresh it after r = b - A x)
    hipStream_t stream = c.stream;
    fused_driver<fcg_scalars> f(c);
    fcg_scalars* scal = f.scal;
    double *part_rho = f.vec_partials(), *part_rhot = f.vec_partials(), *part_tau = f.vec_partials();
    double* part_beta = f.spmv_partials();  // (and, without the epilogue, two more of that size as scratch)
    const size_t per_spmv = f.per_spmv;
    const int g = f.g, nb = f.nb;
    const spmv_dot_plan& spmv = f.spmv;
    const bool csr_epilogue = spmv.fused();
    const bool identity = c.precond == nullptr;
    if (identity) z = r;
    hipLaunchKernelGGL(fcg_fused_init_kernel, dim3(1), dim3(1), 0, stream, scal, c.orig_tau);
    if (!identity) GKOMI_TRY(c.apply_precond(r, z));
    hipLaunchKernelGGL(fused_dot3_partials_kernel, dim3(g), dim3(fblock), 0, stream, n, r, z, t,
                       static_cast<const unsigned char*>(nullptr), part_rho, part_rhot, part_tau);
    GKOMI_TRY(check_launch());
    host_watch& watch = f.watch;
    auto issue = [&](long long it, bool last) -> int {
        hipLaunchKernelGGL(fcg_fused_step1_kernel, dim3(g), dim3(fblock), 0, stream, n, p, z, part_rho,
                           part_rhot, identity ? part_rho : part_tau, g, scal, it,
                           static_cast<long long>(c.max_iters), c.reduction, watch.dev);
        if (last) return check_launch();
        if (csr_epilogue) {
            GKOMI_TRY(spmv.launch(stream, p, q, part_beta, &scal->status));
        } else {
            GKOMI_TRY(A.apply(s, 1, nullptr, p, nullptr, q));
            // only p.q is wanted: the other two sums land in scratch
            hipLaunchKernelGGL(fused_dot3_partials_kernel, dim3(g), dim3(fblock), 0, stream, n, p, q, p,
                               &scal->status, part_beta, part_beta + per_spmv, part_beta + 2 * per_spmv);
        }
        hipLaunchKernelGGL(fcg_fused_step2_kernel, dim3(g), dim3(fblock), 0, stream, n, x, r, t, p, q,
                           part_beta, nb, scal, it, identity ? part_rho : static_cast<double*>(nullptr),
                           identity ? part_rhot : static_cast<double*>(nullptr));
        if (!identity) {
            GKOMI_TRY(c.apply_precond(r, z));
            hipLaunchKernelGGL(fused_dot3_partials_kernel, dim3(g), dim3(fblock), 0, stream, n, r, z, t,
                               &scal->status, part_rho, part_rhot, part_tau);
        }
        return check_launch();
    };
    return f.solve(issue, req.host_info);
}

}  // namespace

extern "C" int gkomi_fcg_solve_fused_f64_i32(
    gkomi_stream_t s, int64_t n, int64_t nnz, const int32_t* row_ptrs, const int32_t* col_idxs,
    const double* vals, int spmv_strategy, int64_t max_row_nnz_hint, gkomi_apply_fn precond,
    void* precond_ctx, const double* b, double* x, int64_t max_iters, double reduction_factor,
    int baseline, int64_t check_every, void* workspace, size_t workspace_bytes, double* host_info)
{
    return fcg_fused_impl({s, n, 1, make_csr_sysmat(n, nnz, row_ptrs, col_idxs, vals, spmv_strategy, max_row_nnz_hint),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, check_every, workspace, workspace_bytes,
        host_info});
}

extern "C" int gkomi_fcg_solve_fused_op_f64(
    gkomi_stream_t s, int64_t n, gkomi_matrix_apply_fn matrix, void* matrix_ctx,
    gkomi_apply_fn precond, void* precond_ctx, const double* b, double* x, int64_t max_iters,
    double reduction_factor, int baseline, int64_t check_every, void* workspace,
    size_t workspace_bytes, double* host_info)
{
    if (matrix == nullptr) return GKOMI_EINVAL;
    return fcg_fused_impl({s, n, 1, make_op_sysmat(n, matrix, matrix_ctx),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, check_every, workspace, workspace_bytes,
        host_info});
}

extern "C" int gkomi_fcg_solve_f64_i32(
    gkomi_stream_t s, int64_t n, int64_t nrhs, int64_t nnz, const int32_t* row_ptrs,
    const int32_t* col_idxs, const double* vals, int spmv_strategy, int64_t max_row_nnz_hint,
    gkomi_apply_fn precond, void* precond_ctx, const double* b, double* x, int64_t max_iters,
    double reduction_factor, int baseline, int64_t check_every, void* workspace,
    size_t workspace_bytes, double* host_info)
{
    return fcg_solve_impl({s, n, nrhs, make_csr_sysmat(n, nnz, row_ptrs, col_idxs, vals, spmv_strategy, max_row_nnz_hint),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, check_every, workspace, workspace_bytes,
        host_info});
}

extern "C" int gkomi_fcg_solve_op_f64(gkomi_stream_t s, int64_t n, int64_t nrhs,
                                        gkomi_matrix_apply_fn matrix, void* matrix_ctx,
                                        gkomi_apply_fn precond, void* precond_ctx, const double* b,
                                        double* x, int64_t max_iters, double reduction_factor,
                                        int baseline, int64_t check_every, void* workspace,
                                        size_t workspace_bytes, double* host_info)
{
    if (matrix == nullptr) return GKOMI_EINVAL;
    return fcg_solve_impl({s, n, nrhs, make_op_sysmat(n, matrix, matrix_ctx),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, check_every, workspace, workspace_bytes,
        host_info});
}

namespace {
int cgs_solve_impl(const solve_request& req)
{
    driver_common c;
    GKOMI_TRY(c.init(req, 11));
    const gkomi_stream_t s = c.s;
    const int64_t n = c.n, nrhs = c.nrhs;
    double *x = req.x, *sc = c.scalars;
    double *r = c.vec(0), *r_tld = c.vec(1), *p = c.vec(2), *q = c.vec(3), *u = c.vec(4), *u_hat = c.vec(5),
           *v_hat = c.vec(6), *t = c.vec(7);
    double *alpha = sc, *beta = sc + nrhs, *gamma = sc + 2 * nrhs, *prev_rho = sc + 3 * nrhs,
           *rho = sc + 4 * nrhs;
    GKOMI_TRY(gkomi_cgs_initialize_f64(s, n, nrhs, req.b, nrhs, r, nrhs, r_tld, nrhs, p, nrhs, q, nrhs, u,
                                       nrhs, u_hat, nrhs, v_hat, nrhs, t, nrhs, alpha, beta, gamma,
                                       prev_rho, rho, c.stop_status));
    GKOMI_TRY(c.start(req, r));
    GKOMI_TRY(gkomi_dense_copy_f64(s, n, nrhs, r, nrhs, r_tld, nrhs));
    int64_t iter = -1;
    while (true) {
        GKOMI_TRY(c.dot(r, r_tld, rho));
        ++iter;
        bool stop = false;
        GKOMI_TRY(c.check(iter, r, true, 1, &stop));
        if (stop) break;
        GKOMI_TRY(gkomi_cgs_step_1_f64(s, n, nrhs, r, nrhs, u, nrhs, p, nrhs, q, nrhs, beta, rho,
                                       prev_rho, c.stop_status));
        GKOMI_TRY(c.apply_precond(p, t));
        GKOMI_TRY(c.spmv(t, v_hat));
        GKOMI_TRY(c.dot(r_tld, v_hat, gamma));
        GKOMI_TRY(gkomi_cgs_step_2_f64(s, n, nrhs, u, nrhs, v_hat, nrhs, q, nrhs, t, nrhs, alpha, rho,
                                       gamma, c.stop_status));
        GKOMI_TRY(c.apply_precond(t, u_hat));
        GKOMI_TRY(c.spmv(u_hat, t));
        GKOMI_TRY(gkomi_cgs_step_3_f64(s, n, nrhs, t, nrhs, u_hat, nrhs, r, nrhs, x, nrhs, alpha,
                                       c.stop_status));
        std::swap(prev_rho, rho);
    }
    return c.finish(c.stop_iter(), r, req.host_info);
}

}  // namespace

// ---- fused CGS, one right-hand side: 5 launches per iteration ------------------------
//   GA  re-adds the partials of rho = r.r_tld and |r|^2, evaluates the criterion,
//       u = r + beta q, p = u + beta (q + beta p) (cgs::step_1)
//   GB  v_hat = A (M p) with the r_tld.v_hat partials in the SpMV epilogue
//   GC  alpha, q = u - alpha v_hat, t = u + q (cgs::step_2)
//   GD  A (M t)
//   GE  x += alpha u_hat, r -= alpha t (cgs::step_3), partials for the next GA
namespace {

struct cgs_scalars : fused_scalars {
    double alpha, beta;
};

__global__ void cgs_fused_init_kernel(cgs_scalars* scal, const double* orig_tau)
{
    init_fused_scalars(scal, 0.0, orig_tau[0]);  // prev_rho = alpha = beta = gamma = 1 (cgs::initialize)
    scal->alpha = 1.0;
    scal->beta = 1.0;
}

// GA
__global__ __launch_bounds__(fblock) void cgs_fused_step1_kernel(
    int64_t n, const double* __restrict__ r, double* __restrict__ u, double* __restrict__ p,
    const double* __restrict__ q, const double* __restrict__ rho_part,
    const double* __restrict__ tau_part, int nparts, cgs_scalars* scal, long long it,
    long long max_iters, double goal, host_watch_line* watch = nullptr)
{
    __shared__ double smem[fblock / wave_size];
    if (fused_stopped_before(status_has_stopped(scal->status), scal, watch, it)) return;
    const pair_sweep sw(n);
    const double* const in[] = {r, q, p};
    double* const out[] = {u, p};
    const auto first = sw.prefetch(in);
    const double rho = sum_partials(rho_part, nparts, smem);
    const double tau = sqrt(sum_partials(tau_part, nparts, smem));
    const double prev = scal->rho[(it + 1) & 1];
    const bool update = prev != 0.0;
    // beta is rewritten only when prev_rho != 0, and then nobody reads the old value.  (Read before the select, not
    // inside it: with the store in fused_criterion's lambda the other form costs 14 VGPRs and a wave per SIMD.)
    const double old_beta = scal->beta;
    const double bt = update ? rho / prev : old_beta;
    if (fused_criterion(scal, watch, it, max_iters, rho, tau, goal, 1, 1, [&](uint8_t st) {
            if (!st && update) scal->beta = bt;
        })) {
        return;
    }
    // cgs::step_1
    sw.run(first, in, out, true, [&](int, const double* e, double* o) {
        const double uu = e[0] + bt * e[1];
        o[0] = uu;
        o[1] = uu + bt * (e[1] + bt * e[2]);
    });
}

// GC
__global__ __launch_bounds__(fblock) void cgs_fused_step2_kernel(
    int64_t n, const double* __restrict__ u, const double* __restrict__ v_hat,
    double* __restrict__ q, double* __restrict__ t, const double* __restrict__ gamma_part,
    int nparts, cgs_scalars* scal, long long it)
{
    __shared__ double smem[fblock / wave_size];
    if (status_has_stopped(scal->status)) return;
    const pair_sweep sw(n);
    const double* const in[] = {u, v_hat};
    double* const out[] = {q, t};
    const auto first = sw.prefetch(in);
    const double gamma = sum_partials(gamma_part, nparts, smem);
    const bool update = gamma != 0.0;
    const double a = update ? scal->rho[it & 1] / gamma : scal->alpha;
    if (update && fused_leader()) scal->alpha = a;
    // cgs::step_2
    sw.run(first, in, out, true, [&](int, const double* e, double* o) {
        o[0] = e[0] - a * e[1];
        o[1] = e[0] + o[0];
    });
}

// GE: x += alpha xdir, r -= alpha rdir; partials of r.r_tld and r.r.  No prefetch: nothing to re-add, alpha is there.
__global__ __launch_bounds__(fblock) void cgs_fused_step3_kernel(
    int64_t n, double* __restrict__ x, double* __restrict__ r, const double* __restrict__ xdir,
    const double* __restrict__ rdir, const double* __restrict__ r_tld, cgs_scalars* scal,
    double* __restrict__ rho_part, double* __restrict__ tau_part)
{
    __shared__ double smem[fblock / wave_size];
    if (status_has_stopped(scal->status)) return;
    const double alpha = scal->alpha;
    const pair_sweep sw(n);
    const double* const in[] = {x, r, xdir, rdir, r_tld};
    double* const out[] = {x, r};
    // cgs::step_3; both halves and the tail into the same two accumulators
    double acc[2] = {0.0, 0.0};
    sw.run(in, out, true, [&](int, const double* e, double* o) {
        o[0] = e[0] + alpha * e[2];
        o[1] = e[1] - alpha * e[3];
        acc[0] += o[1] * e[4];
        acc[1] += o[1] * o[1];
    });
    double* const part[] = {rho_part, tau_part};
    store_block_sums(true, acc, part, smem);
}

int cgs_fused_impl(const solve_request& req)
{
    bool reference;
    GKOMI_TRY(fused_preflight(req, &reference));
    if (reference) return cgs_solve_impl(req);
    driver_common c;
    GKOMI_TRY(c.init(req, 11));
    const gkomi_stream_t s = c.s;
    const int64_t n = c.n;
    const sysmat& A = c.A;
    double *x = req.x, *sc = c.scalars;
    double *r = c.vec(0), *r_tld = c.vec(1), *p = c.vec(2), *q = c.vec(3), *u = c.vec(4), *u_hat = c.vec(5),
           *v_hat = c.vec(6), *t = c.vec(7);
    GKOMI_TRY(gkomi_cgs_initialize_f64(s, n, 1, req.b, 1, r, 1, r_tld, 1, p, 1, q, 1, u, 1, u_hat, 1, v_hat, 1, t, 1,
                                       sc, sc + 1, sc + 2, sc + 3, sc + 4, c.stop_status));
    GKOMI_TRY(c.start(req, r));
    GKOMI_TRY(gkomi_dense_copy_f64(s, n, 1, r, 1, r_tld, 1));
    hipStream_t stream = c.stream;
    fused_driver<cgs_scalars> f(c);
    cgs_scalars* scal = f.scal;
    double *part_rho = f.vec_partials(), *part_tau = f.vec_partials();
    double* part_gamma = f.spmv_partials();  // (and two more of that size as scratch)
    const size_t per_spmv = f.per_spmv;
    const int g = f.g, nb = f.nb;
    const spmv_dot_plan& spmv = f.spmv;
    const bool csr_epilogue = spmv.fused();
    const bool identity = c.precond == nullptr;
    hipLaunchKernelGGL(cgs_fused_init_kernel, dim3(1), dim3(1), 0, stream, scal, c.orig_tau);
    // partials of r.r_tld and r.r (the third sum is scratch)
    hipLaunchKernelGGL(fused_dot3_partials_kernel, dim3(g), dim3(fblock), 0, stream, n, r, r_tld, r,
                       static_cast<const unsigned char*>(nullptr), part_rho, part_gamma + per_spmv, part_tau);
    GKOMI_TRY(check_launch());
    host_watch& watch = f.watch;
    auto issue = [&](long long it, bool last) -> int {
        hipLaunchKernelGGL(cgs_fused_step1_kernel, dim3(g), dim3(fblock), 0, stream, n, r, u, p, q, part_rho,
                           part_tau, g, scal, it, static_cast<long long>(c.max_iters), c.reduction, watch.dev);
        if (last) return check_launch();
        // v_hat = A (M p), gamma = r_tld . v_hat
        const double* mp = p;
        if (!identity) {
            GKOMI_TRY(c.apply_precond(p, t));
            mp = t;
        }
        if (csr_epilogue) {
            GKOMI_TRY(spmv.launch(stream, mp, v_hat, part_gamma, &scal->status, r_tld));
        } else {
            GKOMI_TRY(A.apply(s, 1, nullptr, mp, nullptr, v_hat));
            hipLaunchKernelGGL(fused_dot3_partials_kernel, dim3(g), dim3(fblock), 0, stream, n, r_tld, v_hat,
                               r_tld, &scal->status, part_gamma, part_gamma + per_spmv,
                               part_gamma + 2 * per_spmv);
        }
        hipLaunchKernelGGL(cgs_fused_step2_kernel, dim3(g), dim3(fblock), 0, stream, n, u, v_hat, q, t,
                           part_gamma, nb, scal, it);
        // Identity: u_hat = t, and A t goes to the u_hat buffer; otherwise
        // u_hat = M t and A u_hat overwrites t, as in the reference
        const double *xdir, *rdir;
        if (identity) {
            GKOMI_TRY(A.apply(s, 1, nullptr, t, nullptr, u_hat));
            xdir = t;
            rdir = u_hat;
        } else {
            GKOMI_TRY(c.apply_precond(t, u_hat));
            GKOMI_TRY(A.apply(s, 1, nullptr, u_hat, nullptr, t));
            xdir = u_hat;
            rdir = t;
        }
        hipLaunchKernelGGL(cgs_fused_step3_kernel, dim3(g), dim3(fblock), 0, stream, n, x, r, xdir, rdir,
                           r_tld, scal, part_rho, part_tau);
        return check_launch();
    };
    return f.solve(issue, req.host_info);
}

}  // namespace

extern "C" int gkomi_cgs_solve_fused_f64_i32(
    gkomi_stream_t s, int64_t n, int64_t nnz, const int32_t* row_ptrs, const int32_t* col_idxs,
    const double* vals, int spmv_strategy, int64_t max_row_nnz_hint, gkomi_apply_fn precond,
    void* precond_ctx, const double* b, double* x, int64_t max_iters, double reduction_factor,
    int baseline, int64_t check_every, void* workspace, size_t workspace_bytes, double* host_info)
{
    return cgs_fused_impl({s, n, 1, make_csr_sysmat(n, nnz, row_ptrs, col_idxs, vals, spmv_strategy, max_row_nnz_hint),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, check_every, workspace, workspace_bytes,
        host_info});
}

extern "C" int gkomi_cgs_solve_fused_op_f64(
    gkomi_stream_t s, int64_t n, gkomi_matrix_apply_fn matrix, void* matrix_ctx,
    gkomi_apply_fn precond, void* precond_ctx, const double* b, double* x, int64_t max_iters,
    double reduction_factor, int baseline, int64_t check_every, void* workspace,
    size_t workspace_bytes, double* host_info)
{
    if (matrix == nullptr) return GKOMI_EINVAL;
    return cgs_fused_impl({s, n, 1, make_op_sysmat(n, matrix, matrix_ctx),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, check_every, workspace, workspace_bytes,
        host_info});
}

extern "C" int gkomi_cgs_solve_f64_i32(
    gkomi_stream_t s, int64_t n, int64_t nrhs, int64_t nnz, const int32_t* row_ptrs,
    const int32_t* col_idxs, const double* vals, int spmv_strategy, int64_t max_row_nnz_hint,
    gkomi_apply_fn precond, void* precond_ctx, const double* b, double* x, int64_t max_iters,
    double reduction_factor, int baseline, int64_t check_every, void* workspace,
    size_t workspace_bytes, double* host_info)
{
    return cgs_solve_impl({s, n, nrhs, make_csr_sysmat(n, nnz, row_ptrs, col_idxs, vals, spmv_strategy, max_row_nnz_hint),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, check_every, workspace, workspace_bytes,
        host_info});
}

extern "C" int gkomi_cgs_solve_op_f64(gkomi_stream_t s, int64_t n, int64_t nrhs,
                                        gkomi_matrix_apply_fn matrix, void* matrix_ctx,
                                        gkomi_apply_fn precond, void* precond_ctx, const double* b,
                                        double* x, int64_t max_iters, double reduction_factor,
                                        int baseline, int64_t check_every, void* workspace,
                                        size_t workspace_bytes, double* host_info)
{
    if (matrix == nullptr) return GKOMI_EINVAL;
    return cgs_solve_impl({s, n, nrhs, make_op_sysmat(n, matrix, matrix_ctx),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, check_every, workspace, workspace_bytes,
        host_info});
}

// ---- BiCG / IR ---------------------------------------------------------------------------
extern "C" int gkomi_bicg_initialize_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, const double* b,
                                         int64_t b_stride, double* r, int64_t r_stride, double* z,
                                         int64_t z_stride, double* p, int64_t p_stride, double* q,
                                         int64_t q_stride, double* prev_rho, double* rho,
                                         double* r2, int64_t r2_stride, double* z2,
                                         int64_t z2_stride, double* p2, int64_t p2_stride,
                                         double* q2, int64_t q2_stride, uint8_t* stop_status)
{
    if (bad_dims(n, nrhs)) return GKOMI_EINVAL;
    if (nrhs == 0) return GKOMI_SUCCESS;
    hipLaunchKernelGGL(bicg_initialize_kernel, grid_of(n, nrhs), dim3(block), 0, to_stream(s), n, nrhs,
                       b, b_stride, r, r_stride, z, z_stride, p, p_stride, q, q_stride, prev_rho, rho,
                       r2, r2_stride, z2, z2_stride, p2, p2_stride, q2, q2_stride, stop_status);
    return check_launch();
}

extern "C" int gkomi_bicg_step_1_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, double* p,
                                     int64_t p_stride, const double* z, int64_t z_stride,
                                     double* p2, int64_t p2_stride, const double* z2,
                                     int64_t z2_stride, const double* rho, const double* prev_rho,
                                     const uint8_t* stop_status)
{
    if (bad_dims(n, nrhs)) return GKOMI_EINVAL;
    if (n == 0 || nrhs == 0) return GKOMI_SUCCESS;
    hipLaunchKernelGGL(bicg_step_1_kernel, grid_of(n, nrhs), dim3(block), 0, to_stream(s), n, nrhs, p,
                       p_stride, z, z_stride, p2, p2_stride, z2, z2_stride, rho, prev_rho,
                       stop_status);
    return check_launch();
}

extern "C" int gkomi_bicg_step_2_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, double* x,
                                     int64_t x_stride, double* r, int64_t r_stride, double* r2,
                                     int64_t r2_stride, const double* p, int64_t p_stride,
                                     const double* q, int64_t q_stride, const double* q2,
                                     int64_t q2_stride, const double* beta, const double* rho,
                                     const uint8_t* stop_status)
{
    if (bad_dims(n, nrhs)) return GKOMI_EINVAL;
    if (n == 0 || nrhs == 0) return GKOMI_SUCCESS;
    hipLaunchKernelGGL(bicg_step_2_kernel, grid_of(n, nrhs), dim3(block), 0, to_stream(s), n, nrhs, x,
                       x_stride, r, r_stride, r2, r2_stride, p, p_stride, q, q_stride, q2, q2_stride,
                       beta, rho, stop_status);
    return check_launch();
}

extern "C" int gkomi_ir_initialize(gkomi_stream_t s, int64_t nrhs, uint8_t* stop_status)
{
    if (nrhs < 0) return GKOMI_EINVAL;
    if (nrhs == 0) return GKOMI_SUCCESS;
    hipLaunchKernelGGL(ir_initialize_kernel, dim3(static_cast<unsigned>(ceildiv(nrhs, block))),
                       dim3(block), 0, to_stream(s), nrhs, stop_status);
    return check_launch();
}

// Bicg::apply_dense_impl (core/solver/bicg.cpp:117-232).  The conjugate-transposed
// system matrix is passed in (t_*: csr::transpose of A, what the reference
// builds at the top of every apply); precond_t applies the transposed
// preconditioner (NULL with precond == NULL: Identity; a symmetric
// preconditioner passes the same callback twice).
namespace {

// At: the transposed system matrix, CSR arrays or an operator like A itself
int bicg_solve_impl(const solve_request& req, const sysmat& At, gkomi_apply_fn precond_t, void* precond_t_ctx)
{
    if ((req.precond == nullptr) != (precond_t == nullptr)) return GKOMI_EINVAL;
    const gkomi_stream_t s = req.s;
    const int64_t n = req.n, nrhs = req.nrhs;
    const double* b = req.b;
    double* x = req.x;
    double* host_info = req.host_info;
    driver_common c;
    GKOMI_TRY(c.init(req, 0));
    double *sc = c.scalars, *r = c.vec(0), *z = c.vec(1), *p = c.vec(2), *q = c.vec(3), *r2 = c.vec(4), *z2 = c.vec(5),
           *p2 = c.vec(6), *q2 = c.vec(7);
    double *beta = sc, *prev_rho = sc + nrhs, *rho = sc + 2 * nrhs;
    GKOMI_TRY(gkomi_bicg_initialize_f64(s, n, nrhs, b, nrhs, r, nrhs, z, nrhs, p, nrhs, q, nrhs,
                                        prev_rho, rho, r2, nrhs, z2, nrhs, p2, nrhs, q2, nrhs,
                                        c.stop_status));
    GKOMI_TRY(c.start(req, r));
    GKOMI_TRY(gkomi_dense_copy_f64(s, n, nrhs, r, nrhs, r2, nrhs));
    int64_t iter = -1;
    while (true) {
        GKOMI_TRY(c.apply_precond(r, z));
        if (precond_t == nullptr) {
            GKOMI_TRY(gkomi_dense_copy_f64(s, n, nrhs, r2, nrhs, z2, nrhs));
        } else {
            GKOMI_TRY(precond_t(precond_t_ctx, s, r2, z2));
        }
        GKOMI_TRY(c.dot(z, r2, rho));
        ++iter;
        bool stop = false;
        GKOMI_TRY(c.check(iter, r, true, 1, &stop));
        if (stop) break;
        GKOMI_TRY(gkomi_bicg_step_1_f64(s, n, nrhs, p, nrhs, z, nrhs, p2, nrhs, z2, nrhs, rho, prev_rho,
                                        c.stop_status));
        GKOMI_TRY(c.spmv(p, q));
        if (At.is_csr()) {
            GKOMI_TRY(gkomi_csr_spmv_f64_i32(s, n, n, nrhs, At.nnz, At.row_ptrs, At.col_idxs, At.vals, p2, nrhs,
                                             q2, nrhs, nullptr, nullptr, At.strategy, -1));
        } else {
            GKOMI_TRY(At.apply(s, nrhs, nullptr, p2, nullptr, q2));
        }
        GKOMI_TRY(c.dot(p2, q, beta));
        GKOMI_TRY(gkomi_bicg_step_2_f64(s, n, nrhs, x, nrhs, r, nrhs, r2, nrhs, p, nrhs, q, nrhs, q2,
                                        nrhs, beta, rho, c.stop_status));
        std::swap(prev_rho, rho);
    }
    return c.finish(c.stop_iter(), r, host_info);
}

}  // namespace

extern "C" int gkomi_bicg_solve_f64_i32(
    gkomi_stream_t s, int64_t n, int64_t nrhs, int64_t nnz, const int32_t* row_ptrs,
    const int32_t* col_idxs, const double* vals, const int32_t* t_row_ptrs,
    const int32_t* t_col_idxs, const double* t_vals, int spmv_strategy, int64_t max_row_nnz_hint,
    gkomi_apply_fn precond, void* precond_ctx, gkomi_apply_fn precond_t, void* precond_t_ctx,
    const double* b, double* x, int64_t max_iters, double reduction_factor, int baseline,
    int64_t check_every, void* workspace, size_t workspace_bytes, double* host_info)
{
    return bicg_solve_impl({s, n, nrhs, make_csr_sysmat(n, nnz, row_ptrs, col_idxs, vals, spmv_strategy, max_row_nnz_hint),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, check_every, workspace, workspace_bytes,
        host_info}, make_csr_sysmat(n, nnz, t_row_ptrs, t_col_idxs, t_vals, spmv_strategy, -1), precond_t, precond_t_ctx);
}

// the same loop with A and its transpose behind callbacks (any format: a Dense and its Dense::transpose, ...)
extern "C" int gkomi_bicg_solve_op_f64(
    gkomi_stream_t s, int64_t n, int64_t nrhs, gkomi_matrix_apply_fn matrix, void* matrix_ctx,
    gkomi_matrix_apply_fn matrix_t, void* matrix_t_ctx, gkomi_apply_fn precond, void* precond_ctx,
    gkomi_apply_fn precond_t, void* precond_t_ctx, const double* b, double* x, int64_t max_iters,
    double reduction_factor, int baseline, int64_t check_every, void* workspace, size_t workspace_bytes,
    double* host_info)
{
    if (matrix == nullptr || matrix_t == nullptr) return GKOMI_EINVAL;
    sysmat At;  // (kept an operator also where it is the library's CSR callback: its record carries the strategy)
    At.n = n;
    At.op = matrix_t;
    At.ctx = matrix_t_ctx;
    return bicg_solve_impl({s, n, nrhs, make_op_sysmat(n, matrix, matrix_ctx), precond, precond_ctx, b, x, max_iters,
        reduction_factor, baseline, check_every, workspace, workspace_bytes, host_info}, At, precond_t, precond_t_ctx);
}

// Ir::apply_dense_impl (core/solver/ir.cpp:186-277) with the caller's x as the
// initial guess: residual = b - A x, criterion, x += relaxation_factor *
// inner(residual); inner == NULL is the Identity (Richardson).  The criterion
// is looked at on the host every iteration (the update is not status-aware in
// the reference either: a stopped column keeps being relaxed until all stop).
extern "C" int gkomi_ir_solve_f64_i32(
    gkomi_stream_t s, int64_t n, int64_t nrhs, int64_t nnz, const int32_t* row_ptrs,
    const int32_t* col_idxs, const double* vals, int spmv_strategy, int64_t max_row_nnz_hint,
    gkomi_apply_fn inner, void* inner_ctx, double relaxation_factor, const double* b, double* x,
    int64_t max_iters, double reduction_factor, int baseline, void* workspace,
    size_t workspace_bytes, double* host_info)
{
    const solve_request req{s, n, nrhs, make_csr_sysmat(n, nnz, row_ptrs, col_idxs, vals, spmv_strategy, max_row_nnz_hint),
        inner, inner_ctx, b, x, max_iters, reduction_factor, baseline, 1, workspace, workspace_bytes, host_info};
    driver_common c;
    GKOMI_TRY(c.init(req, 0));
    double *residual = c.vec(0), *inner_solution = c.vec(1);
    double* relax = c.scalars;
    GKOMI_TRY(gkomi_dense_fill_f64(s, 1, nrhs, relax, nrhs, relaxation_factor));
    GKOMI_TRY(gkomi_ir_initialize(s, nrhs, c.stop_status));
    GKOMI_TRY(gkomi_dense_copy_f64(s, n, nrhs, b, nrhs, residual, nrhs));
    GKOMI_TRY(c.start(req, residual));
    int64_t iter = -1;
    while (true) {
        ++iter;
        if (iter > 0) {
            GKOMI_TRY(gkomi_dense_copy_f64(s, n, nrhs, b, nrhs, residual, nrhs));
            GKOMI_TRY(c.A.apply(s, nrhs, c.neg_one, x, c.one, residual));
        }
        bool stop = false;
        GKOMI_TRY(c.check(iter, residual, true, 1, &stop));
        if (stop) break;
        GKOMI_TRY(c.apply_precond(residual, inner_solution));
        GKOMI_TRY(gkomi_dense_add_scaled_f64(s, n, nrhs, relax, nrhs, inner_solution, nrhs, x, nrhs));
    }
    return c.finish(c.stop_iter(), residual, host_info);
}
