// IDR(s) for gfx950.  Replaces gko::kernels::hip::idr::{initialize, step_1, step_2, step_3, compute_omega}
// (core/solver/idr_kernels.hpp) and provides native drivers for Idr::iterate (core/solver/idr.cpp:157-290).
// Semantics = reference/solver/idr_kernels.cpp:134-315, real subspace, the caller fills P (deterministic == true).
//
// Three layers:
//   step kernels     the reference's layouts (g, u: n x (s nrhs) row-major, column k nrhs + i belongs to rhs i), so a
//                    shim is zero-copy.  step_1, step_2 and compute_omega are elementwise once c = M \ f is known and
//                    spell every expression as the reference does (-ffp-contract=off): bit-identical.  The dots of
//                    step_3 and of initialize are summed in a two-stage order: equal to rounding.
//   idr_solve_impl   the reference's kernel sequence, any number of right-hand sides, criterion on the device
//   idr_fused_impl   one right-hand side, s <= 8: g and u column-major, the projection of step 3 as one multi-dot sweep
//                    + an s x s solve in every workgroup + one update sweep, 4 s + 2 launches per outer iteration
#include <algorithm>
#include <type_traits>
#include <utility>

#include "common.hpp"
#include "fused_krylov.hpp"
#include "internal.hpp"
#include "krylov_driver.hpp"

namespace gkomi {
namespace {

constexpr int block = 256;
constexpr int64_t max_subspace = 32;
constexpr int fused_max_subspace = 8;
constexpr int dot_blocks = 128;  // partial sums per dot of the two-stage multi-dot

bool bad_idr_dims(int64_t n, int64_t nrhs, int64_t sdim, int64_t k)
{
    return n < 0 || nrhs < 0 || sdim < 1 || sdim > max_subspace || k < 0 || k >= sdim;
}
dim3 grid_of(int64_t n, int64_t nrhs) { return dim3(static_cast<unsigned>(ceildiv(std::max<int64_t>(n * nrhs, 1), block))); }

#define GKOMI_IDR_ELEMENT(row, i)                                                       \
    const int64_t idx_ = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x;        \
    if (idx_ >= n * nrhs) return;                                                       \
    const int64_t row = idx_ / nrhs;                                                    \
    const int64_t i = idx_ - row * nrhs;                                                \
    if (status_has_stopped(stop_status[i])) return

// ---- step kernels -----------------------------------------------------------------------------------------------
// m = identity pattern, statuses reset (idr_kernels.cpp:140-150)
__global__ __launch_bounds__(block) void idr_initialize_m_kernel(int64_t nrhs, int64_t sdim, double* __restrict__ m,
                                                                 int64_t m_stride, uint8_t* __restrict__ stop_status)
{
    const int64_t idx = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x;
    if (idx < nrhs) stop_status[idx] = 0;
    if (idx >= sdim * sdim * nrhs) return;
    const int64_t row = idx / (sdim * nrhs), col = idx - row * (sdim * nrhs);
    m[row * m_stride + col] = row == col / nrhs ? 1.0 : 0.0;
}

template <int Block>
__device__ __forceinline__ double block_allreduce_sum(double v, double* smem, double* bcast)
{
    const double total = block_reduce_sum<Block>(v, smem);
    if (threadIdx.x == 0) *bcast = total;
    __syncthreads();
    const double all = *bcast;
    __syncthreads();  // smem and bcast are free again
    return all;
}

// Modified Gram-Schmidt over the rows of P in row order (idr_kernels.cpp:152-188), one workgroup: a thread keeps
// the same columns in every phase, so only the sums cross threads.  Once per solve.
__global__ __launch_bounds__(fblock) void idr_orthonormalize_kernel(int64_t sdim, int64_t n, double* __restrict__ p,
                                                                    int64_t p_stride)
{
    __shared__ double smem[fblock / wave_size];
    __shared__ double bcast;
    for (int64_t row = 0; row < sdim; ++row) {
        double* pr = p + row * p_stride;
        for (int64_t i = 0; i < row; ++i) {
            const double* pi = p + i * p_stride;
            double acc = 0.0;
            for (int64_t j = threadIdx.x; j < n; j += fblock) acc += pr[j] * pi[j];
            const double dot = block_allreduce_sum<fblock>(acc, smem, &bcast);
            for (int64_t j = threadIdx.x; j < n; j += fblock) pr[j] -= dot * pi[j];
        }
        double acc = 0.0;
        for (int64_t j = threadIdx.x; j < n; j += fblock) acc += pr[j] * pr[j];
        const double norm = sqrt(block_allreduce_sum<fblock>(acc, smem, &bcast));
        for (int64_t j = threadIdx.x; j < n; j += fblock) pr[j] /= norm;
    }
}

// c = M \ f, one thread per column (solve_lower_triangular, idr_kernels.cpp:60-80)
__global__ __launch_bounds__(block) void idr_solve_lower_kernel(int64_t nrhs, int64_t sdim, const double* m,
                                                                int64_t m_stride, const double* f, int64_t f_stride,
                                                                double* c, int64_t c_stride,
                                                                const uint8_t* __restrict__ stop_status)
{
    const int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x;
    if (i >= nrhs || status_has_stopped(stop_status[i])) return;
    for (int64_t row = 0; row < sdim; ++row) {
        double temp = f[row * f_stride + i];
        for (int64_t col = 0; col < row; ++col) temp -= m[row * m_stride + col * nrhs + i] * c[col * c_stride + i];
        c[row * c_stride + i] = temp / m[row * m_stride + row * nrhs + i];
    }
}

// v = residual - c_k g_k - ... - c_{s-1} g_{s-1} (idr_kernels.cpp:206-218)
__global__ __launch_bounds__(block) void idr_step_1_kernel(int64_t n, int64_t nrhs, int64_t sdim, int64_t k,
                                                           const double* __restrict__ residual, int64_t r_stride,
                                                           const double* __restrict__ g, int64_t g_stride,
                                                           const double* __restrict__ c, int64_t c_stride,
                                                           double* __restrict__ v, int64_t v_stride,
                                                           const uint8_t* __restrict__ stop_status)
{
    GKOMI_IDR_ELEMENT(row, i);
    double temp = residual[row * r_stride + i];
    for (int64_t j = k; j < sdim; ++j) temp -= c[j * c_stride + i] * g[row * g_stride + j * nrhs + i];
    v[row * v_stride + i] = temp;
}

// u_k = omega * preconditioned_vector + c_k u_k + ... + c_{s-1} u_{s-1} (idr_kernels.cpp:231-243)
__global__ __launch_bounds__(block) void idr_step_2_kernel(int64_t n, int64_t nrhs, int64_t sdim, int64_t k,
                                                           const double* __restrict__ omega,
                                                           const double* __restrict__ pv, int64_t pv_stride,
                                                           const double* __restrict__ c, int64_t c_stride, double* u,
                                                           int64_t u_stride, const uint8_t* __restrict__ stop_status)
{
    GKOMI_IDR_ELEMENT(row, i);
    double temp = omega[i] * pv[row * pv_stride + i];
    for (int64_t j = k; j < sdim; ++j) temp += c[j * c_stride + i] * u[row * u_stride + j * nrhs + i];
    u[row * u_stride + k * nrhs + i] = temp;
}

// idr_kernels.cpp:299-312
__global__ __launch_bounds__(block) void idr_compute_omega_kernel(int64_t nrhs, double kappa,
                                                                  const double* __restrict__ tht,
                                                                  const double* __restrict__ residual_norm,
                                                                  double* __restrict__ omega,
                                                                  const uint8_t* __restrict__ stop_status)
{
    const int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x;
    if (i >= nrhs || status_has_stopped(stop_status[i])) return;
    const double thr = omega[i];
    const double normt = sqrt(tht[i]);
    double om = thr / tht[i];
    const double absrho = fabs(thr / (normt * residual_norm[i]));
    if (absrho < kappa) om *= kappa / absrho;
    omega[i] = om;
}

// Two-stage multi-dot: out(jj, i) = P_jj . w(:, i) for the rows P_0.. of `p` that gridDim.y covers.
// part[y * gridDim.x + blockIdx.x], y = jj * nrhs + i
__global__ __launch_bounds__(block) void idr_multidot_partials_kernel(int64_t n, int64_t nrhs,
                                                                      const double* __restrict__ p, int64_t p_stride,
                                                                      const double* __restrict__ w, int64_t w_stride,
                                                                      double* __restrict__ part,
                                                                      const uint8_t* __restrict__ stop_status)
{
    __shared__ double smem[block / wave_size];
    const int64_t y = blockIdx.y, jj = y / nrhs, i = y - jj * nrhs;
    if (status_has_stopped(stop_status[i])) return;
    const double* pj = p + jj * p_stride;
    const int64_t step = static_cast<int64_t>(gridDim.x) * block;
    double acc = 0.0;
    for (int64_t ind = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; ind < n; ind += step) {
        acc += pj[ind] * w[ind * w_stride + i];
    }
    const double total = block_reduce_sum<block>(acc, smem);
    if (threadIdx.x == 0) part[y * gridDim.x + blockIdx.x] = total;
}
// one wave per dot: out[jj * out_stride + i] = sum of its partials (/ div[i] if given)
__global__ __launch_bounds__(wave_size) void idr_multidot_finish_kernel(int64_t nrhs, int nparts,
                                                                        const double* __restrict__ part,
                                                                        double* __restrict__ out, int64_t out_stride,
                                                                        const double* __restrict__ div,
                                                                        const uint8_t* __restrict__ stop_status)
{
    const int64_t y = blockIdx.x, jj = y / nrhs, i = y - jj * nrhs;
    if (status_has_stopped(stop_status[i])) return;
    double acc = 0.0;
    for (int b = threadIdx.x; b < nparts; b += wave_size) acc += part[y * nparts + b];
    acc = wave_reduce_sum(acc);
    if (threadIdx.x == 0) out[jj * out_stride + i] = div != nullptr ? acc / div[i] : acc;
}

// g_k -= alpha g_j, u_k -= alpha u_j (update_g_and_u, idr_kernels.cpp:102-105)
__global__ __launch_bounds__(block) void idr_update_g_and_u_kernel(int64_t n, int64_t nrhs, int64_t k, int64_t j,
                                                                   const double* __restrict__ alpha,
                                                                   const double* g, int64_t g_stride,
                                                                   double* __restrict__ g_k, int64_t g_k_stride,
                                                                   double* u, int64_t u_stride,
                                                                   const uint8_t* __restrict__ stop_status)
{
    GKOMI_IDR_ELEMENT(row, i);
    g_k[row * g_k_stride + i] -= alpha[i] * g[row * g_stride + j * nrhs + i];
    u[row * u_stride + k * nrhs + i] -= alpha[i] * u[row * u_stride + j * nrhs + i];
}

// g(:, k) = g_k, residual -= beta g_k, x += beta u_k (idr_kernels.cpp:108-110, 273-278)
__global__ __launch_bounds__(block) void idr_step_3_update_kernel(int64_t n, int64_t nrhs, int64_t k,
                                                                  const double* __restrict__ f, int64_t f_stride,
                                                                  const double* __restrict__ m, int64_t m_stride,
                                                                  double* __restrict__ g, int64_t g_stride,
                                                                  const double* __restrict__ g_k, int64_t g_k_stride,
                                                                  const double* __restrict__ u, int64_t u_stride,
                                                                  double* __restrict__ residual, int64_t r_stride,
                                                                  double* __restrict__ x, int64_t x_stride,
                                                                  const uint8_t* __restrict__ stop_status)
{
    GKOMI_IDR_ELEMENT(row, i);
    const double beta = f[k * f_stride + i] / m[k * m_stride + k * nrhs + i];
    const double gk = g_k[row * g_k_stride + i];
    g[row * g_stride + k * nrhs + i] = gk;
    residual[row * r_stride + i] -= beta * gk;
    x[row * x_stride + i] += beta * u[row * u_stride + k * nrhs + i];
}

// f = (0, ..., 0, f_{k+1} - beta m_{k+1,k}, ...) (idr_kernels.cpp:280-285); after the update kernel, which reads f_k
__global__ __launch_bounds__(block) void idr_step_3_f_kernel(int64_t nrhs, int64_t sdim, int64_t k,
                                                             double* __restrict__ f, int64_t f_stride,
                                                             const double* __restrict__ m, int64_t m_stride,
                                                             const uint8_t* __restrict__ stop_status)
{
    const int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x;
    if (i >= nrhs || status_has_stopped(stop_status[i]) || k + 1 >= sdim) return;
    const double beta = f[k * f_stride + i] / m[k * m_stride + k * nrhs + i];
    f[k * f_stride + i] = 0.0;
    for (int64_t j = k + 1; j < sdim; ++j) f[j * f_stride + i] -= beta * m[j * m_stride + k * nrhs + i];
}

// residual -= omega t, x += omega helper at the end of an outer iteration (core/solver/idr.cpp:287-289).  The
// reference's add_scaled also moves the columns that have stopped; a stopped column keeps its x and residual here.
// helper may be the residual itself (Identity): it is read before the residual is stored.
__global__ __launch_bounds__(block) void idr_closing_kernel(int64_t n, int64_t nrhs, const double* __restrict__ omega,
                                                            const double* __restrict__ t, const double* helper,
                                                            double* residual, double* __restrict__ x,
                                                            const uint8_t* __restrict__ stop_status)
{
    GKOMI_IDR_ELEMENT(row, i);
    const int64_t at = row * nrhs + i;
    const double h = helper[at];
    residual[at] += omega[i] * -t[at];
    x[at] += omega[i] * h;
}

dim3 cols_grid(int64_t nrhs) { return dim3(static_cast<unsigned>(ceildiv(std::max<int64_t>(nrhs, 1), block))); }

// out(jj, i) = P_jj . w(:, i), jj < nj; `ws` holds dot_blocks * nj * nrhs doubles
int multidot(hipStream_t stream, int64_t n, int64_t nrhs, int64_t nj, const double* p, int64_t p_stride,
             const double* w, int64_t w_stride, double* out, int64_t out_stride, const double* div, double* ws,
             const uint8_t* stop_status)
{
    if (nj <= 0 || nrhs <= 0) return GKOMI_SUCCESS;
    if (nj * nrhs > 65535) return GKOMI_ENOTSUPPORTED;
    const int nblk = grid_for(n, block, dot_blocks);
    hipLaunchKernelGGL(idr_multidot_partials_kernel, dim3(nblk, static_cast<unsigned>(nj * nrhs)), dim3(block), 0, stream, n,
                       nrhs, p, p_stride, w, w_stride, ws, stop_status);
    hipLaunchKernelGGL(idr_multidot_finish_kernel, dim3(static_cast<unsigned>(nj * nrhs)), dim3(wave_size), 0, stream, nrhs,
                       nblk, ws, out, out_stride, div, stop_status);
    return check_launch();
}

// ---- workspace ----------------------------------------------------------------------------------------------------
struct idr_layout {
    solver_layout base;  // 5 vectors (residual, v, t, helper, contiguous u_k), the scalars, the reductions, SpMV partials
    size_t g, u, m, f, c, dots, pcopy, parts, total;
    int64_t ld;          // leading dimension of the fused driver's column-major g, u and copy of P
};

idr_layout make_idr_layout(int64_t n, int64_t nrhs, int64_t sdim)
{
    idr_layout l{};
    l.base = make_solver_layout(n, nrhs, 5);
    l.ld = n + (n & 1);
    size_t off = l.base.total;
    auto take = [&](size_t doubles) {
        const size_t at = off;
        off += align256(sizeof(double) * doubles);
        return at;
    };
    const size_t wide = static_cast<size_t>(std::max(l.ld * sdim, n * sdim * nrhs)) + 2;
    l.g = take(wide);
    l.u = take(wide);
    l.m = take(static_cast<size_t>(std::max<int64_t>(sdim * sdim * nrhs, 64)));
    l.f = take(static_cast<size_t>(std::max<int64_t>(sdim * nrhs, 16)));
    l.c = take(static_cast<size_t>(sdim * nrhs));
    l.dots = take(static_cast<size_t>(dot_blocks * sdim * nrhs));
    const bool fusable = nrhs == 1 && sdim <= fused_max_subspace;
    l.pcopy = take(fusable ? static_cast<size_t>(l.ld * sdim) + 2 : 0);
    l.parts = take(fusable ? static_cast<size_t>(2 * sdim + 2) * max_parts : 0);
    l.total = off;
    return l;
}

struct idr_params {
    int64_t sdim;
    double kappa;
    double* subspace;
};

// ---- the reference's kernel sequence (core/solver/idr.cpp:157-290) -------------------------------------------------
int idr_solve_impl(const solve_request& req, const idr_params& prm)
{
    const gkomi_stream_t s = req.s;
    const int64_t n = req.n, nrhs = req.nrhs, sdim = prm.sdim;
    if (n < 0 || nrhs <= 0 || sdim < 1 || sdim > max_subspace || sdim > n || prm.subspace == nullptr) return GKOMI_EINVAL;
    const idr_layout l = make_idr_layout(n, nrhs, sdim);
    driver_common c;
    GKOMI_TRY(c.init(req, static_cast<int>(2 * sdim + 6), l.base, l.total));
    char* ws = c.ws;
    double *x = req.x, *sc = c.scalars;
    auto D = [&](size_t at) { return reinterpret_cast<double*>(ws + at); };
    double *r = c.vec(0), *v = c.vec(1), *t = c.vec(2), *helper = c.vec(3), *u_k = c.vec(4);
    double *g = D(l.g), *u = D(l.u), *m = D(l.m), *f = D(l.f), *cc = D(l.c), *dots = D(l.dots);
    double *omega = sc, *tht = sc + nrhs, *alpha = sc + 2 * nrhs, *residual_norm = sc + 3 * nrhs;
    double* p = prm.subspace;
    const int64_t wide = sdim * nrhs;
    hipStream_t stream = c.stream;
    GKOMI_TRY(gkomi_idr_initialize_f64(s, n, nrhs, sdim, m, wide, p, n, c.stop_status));
    GKOMI_TRY(gkomi_dense_fill_f64(s, 1, nrhs, omega, nrhs, 1.0));
    GKOMI_TRY(gkomi_dense_copy_f64(s, n, nrhs, req.b, nrhs, r, nrhs));
    GKOMI_TRY(c.start(req, r));
    GKOMI_TRY(static_cast<int>(hipMemsetAsync(g, 0, sizeof(double) * n * wide, stream)));
    GKOMI_TRY(static_cast<int>(hipMemsetAsync(u, 0, sizeof(double) * n * wide, stream)));
    const bool ident = c.precond == nullptr;  // Identity: helper is v, then the residual, without the copies
    int64_t iter = -1;
    while (true) {
        ++iter;
        // The reference hands its criterion the norm taken before the omega step (idr.cpp:273 -> :211-216); here the
        // criterion sees the residual it is about to return, so the reported norm is the true one.
        bool stop = false;
        GKOMI_TRY(c.check(iter, r, true, 1, &stop));
        if (stop) break;
        GKOMI_TRY(multidot(stream, n, nrhs, sdim, p, n, r, nrhs, f, nrhs, nullptr, dots, c.stop_status));  // f = P r
        for (int64_t k = 0; k < sdim; ++k) {
            GKOMI_TRY(gkomi_idr_step_1_f64(s, n, nrhs, sdim, k, m, wide, f, nrhs, r, nrhs, g, wide, cc, nrhs, v, nrhs,
                                           c.stop_status));
            if (!ident) GKOMI_TRY(c.apply_precond(v, helper));
            GKOMI_TRY(gkomi_idr_step_2_f64(s, n, nrhs, sdim, k, omega, ident ? v : helper, nrhs, cc, nrhs, u, wide,
                                           c.stop_status));
            // g_k = A u_k: the operators take contiguous vectors, u_k is a column block of u
            GKOMI_TRY(gkomi_dense_copy_f64(s, n, nrhs, u + k * nrhs, wide, u_k, nrhs));
            GKOMI_TRY(c.spmv(u_k, helper));
            GKOMI_TRY(gkomi_idr_step_3_f64(s, n, nrhs, sdim, k, p, n, g, wide, helper, nrhs, u, wide, m, wide, f, nrhs,
                                           alpha, r, nrhs, x, nrhs, c.stop_status, dots,
                                           sizeof(double) * dot_blocks * sdim * nrhs));
        }
        if (!ident) GKOMI_TRY(c.apply_precond(r, helper));
        GKOMI_TRY(c.spmv(ident ? r : helper, t));
        GKOMI_TRY(c.dot(t, r, omega));
        GKOMI_TRY(c.dot(t, t, tht));
        GKOMI_TRY(gkomi_dense_compute_norm2_f64(s, n, nrhs, r, nrhs, residual_norm, c.red, c.red_bytes));
        GKOMI_TRY(gkomi_idr_compute_omega_f64(s, nrhs, prm.kappa, tht, residual_norm, omega, c.stop_status));
        // x += omega * helper, the preconditioned residual (idr.cpp:289; the comment above it says v)
        hipLaunchKernelGGL(idr_closing_kernel, grid_of(n, nrhs), dim3(block), 0, stream, n, nrhs, omega, t, ident ? r : helper, r, x,
                           c.stop_status);
        GKOMI_TRY(check_launch());
    }
    return c.finish(c.stop_iter(), r, req.host_info);
}

// ---- fused IDR(s), one right-hand side, s <= 8 -----------------------------------------------------------------------
//
// g, u and a copy of the orthonormalised P are column-major with an even leading dimension, so that every sweep moves
// 16 B per lane whatever n is, and g_k = A u_k is written in place (no copy of a strided column).  m is s x s with
// row stride `ms`, f is double-buffered (inner step k reads f[k & 1] and leaves f[(k + 1) & 1]: workgroup 0 may store
// while a late workgroup still reads).  Per outer iteration, Identity preconditioner:
//   S12(0)  re-adds |r|^2 and f = P r left by the closing sweep, criterion; c = M \ f; v = r - sum c_j g_j and
//           u_0 = omega v + sum c_j u_j in one pass (v is never stored)
//   then for k = 0 .. s-1:  [S12(k) for k > 0]   g_k = A u_k   DOTS: d = P g_k, s sums in one pass
//           PROJ(k): every workgroup re-adds d, alpha_j = (d_j - sum_{i<j} m_ji alpha_i) / m_jj (j < k),
//                    m_jk = d_j - sum_{i<k} m_ji alpha_i (j >= k), beta = f_k / m_kk, then ONE update sweep
//                    g_k -= sum alpha_i g_i, u_k -= sum alpha_i u_i, r -= beta g_k, x += beta u_k (+ partials of |r|^2)
//   t = A r with the partials of t.r and t.t in the SpMV's epilogue
//   CLOSE   omega (compute_omega), r -= omega t, x += omega r_old, partials of |r|^2 and of f = P r
// = 4 s + 2 launches.  With a preconditioner S12 splits into S1 (v) - apply - S2 (u_k), and helper = M^-1 r precedes
// the last SpMV.  p_j . g_i = m_ji is already stored, which is why the k sequential dot/update pairs of the reference
// collapse into one sweep and a triangular solve: an identity in exact arithmetic.
struct idr_scalars : fused_scalars {
    double omega;
};

template <int N>
struct ptr_list {
    const double* p[N];
    __device__ const double* const (&get() const)[N] { return reinterpret_cast<const double* const(&)[N]>(p); }
};

__device__ __forceinline__ bool idr_stopped(const idr_scalars* scal) { return status_has_stopped(scal->status); }

// thread 0: c = M \ f in the reference's order (solve_lower_triangular)
__device__ __forceinline__ void solve_lower(int s, const double* m, int ms, const double* f, double* c)
{
    for (int row = 0; row < s; ++row) {
        double temp = f[row];
        for (int col = 0; col < row; ++col) temp -= m[row * ms + col] * c[col];
        c[row] = temp / m[row * ms + row];
    }
}

// part[0] = sum r^2, part[1 + j] = P_j . r: the state the first S12 of a solve re-adds
template <int S>
__global__ __launch_bounds__(fblock) void idr_fused_start_kernel(int64_t n, const double* __restrict__ r,
                                                                 const double* __restrict__ p, int64_t ld,
                                                                 idr_scalars* scal, const double* orig_tau,
                                                                 double* __restrict__ part)
{
    __shared__ double smem[fblock / wave_size];
    if (fused_leader()) {
        init_fused_scalars(scal, 0.0, orig_tau[0]);
        scal->omega = 1.0;
    }
    const pair_sweep sw(n);
    ptr_list<1 + S> in;
    in.p[0] = r;
#pragma unroll
    for (int j = 0; j < S; ++j) in.p[1 + j] = p + j * ld;
    double acc[1 + S] = {};
    auto body = [&](int, const double* e) {
        acc[0] += e[0] * e[0];
#pragma unroll
        for (int j = 0; j < S; ++j) acc[1 + j] += e[1 + j] * e[0];
    };
    sw.loop(sw.i0, in.get(), body);
    sw.tail(in.get(), body);
    double* out[1 + S];
#pragma unroll
    for (int j = 0; j <= S; ++j) out[j] = part + j * max_parts;
    store_block_sums(false, acc, reinterpret_cast<double* const(&)[1 + S]>(out), smem);
}

// S12 / S1: NJ = s - k vectors take part.  WITH_U: u_k too (Identity), else v is stored for the preconditioner.
template <int NJ, bool WITH_U>
__global__ __launch_bounds__(fblock) void idr_fused_step_1_kernel(int64_t n, int s, int k, const double* __restrict__ r,
                                                                  const double* __restrict__ g, double* __restrict__ u,
                                                                  int64_t ld, double* __restrict__ v, const double* m,
                                                                  int ms, double* f, const double* __restrict__ part,
                                                                  int nparts, idr_scalars* scal, long long it,
                                                                  long long max_iters, double goal, host_watch_line* watch)
{
    __shared__ double smem[fblock / wave_size];
    __shared__ double sf[fused_max_subspace], sc[fused_max_subspace];
    if (k == 0) {
        if (fused_stopped_before(idr_stopped(scal), scal, watch, it)) return;
        const double tau = sqrt(sum_partials(part, nparts, smem));
        for (int j = 0; j < s; ++j) {
            const double fj = sum_partials(part + (1 + j) * max_parts, nparts, smem);
            if (threadIdx.x == 0) sf[j] = fj;
        }
        if (fused_criterion(scal, watch, it, max_iters, 0.0, tau, goal, 1, 1)) return;
        if (fused_leader()) {
            for (int j = 0; j < s; ++j) f[j] = sf[j];
        }
    } else {
        if (idr_stopped(scal)) return;
        if (threadIdx.x == 0) {
            for (int j = 0; j < s; ++j) sf[j] = f[j];
        }
    }
    if (threadIdx.x == 0) solve_lower(s, m, ms, sf, sc);
    __syncthreads();
    double c[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) c[j] = sc[k + j];
    const double omega = scal->omega;
    const pair_sweep sw(n);
    ptr_list<WITH_U ? 1 + 2 * NJ : 1 + NJ> in;
    in.p[0] = r;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        in.p[1 + j] = g + (k + j) * ld;
        if (WITH_U) in.p[1 + NJ + j] = u + (k + j) * ld;
    }
    double* const out[] = {WITH_U ? u + k * ld : v};
    sw.run(in.get(), out, true, [&](int, const double* e, double* o) {
        // idr::step_1: j = k .. s-1 left to right
        double temp = e[0];
#pragma unroll
        for (int j = 0; j < NJ; ++j) temp -= c[j] * e[1 + j];
        if (WITH_U) {  // idr::step_2 on helper = v
            double t2 = omega * temp;
#pragma unroll
            for (int j = 0; j < NJ; ++j) t2 += c[j] * e[1 + NJ + j];
            temp = t2;
        }
        o[0] = temp;
    });
}

// S2: u_k = omega helper + sum c_j u_j (idr::step_2)
template <int NJ>
__global__ __launch_bounds__(fblock) void idr_fused_step_2_kernel(int64_t n, int s, int k, const double* __restrict__ helper,
                                                                  double* __restrict__ u, int64_t ld, const double* m,
                                                                  int ms, const double* f, const idr_scalars* scal)
{
    __shared__ double sc[fused_max_subspace];
    if (idr_stopped(scal)) return;
    if (threadIdx.x == 0) solve_lower(s, m, ms, f, sc);
    __syncthreads();
    double c[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) c[j] = sc[k + j];
    const double omega = scal->omega;
    const pair_sweep sw(n);
    ptr_list<1 + NJ> in;
    in.p[0] = helper;
#pragma unroll
    for (int j = 0; j < NJ; ++j) in.p[1 + j] = u + (k + j) * ld;
    double* const out[] = {u + k * ld};
    sw.run(in.get(), out, true, [&](int, const double* e, double* o) {
        double temp = omega * e[0];
#pragma unroll
        for (int j = 0; j < NJ; ++j) temp += c[j] * e[1 + j];
        o[0] = temp;
    });
}

// DOTS: part[j] = P_j . g_k, j < S
template <int S>
__global__ __launch_bounds__(fblock) void idr_fused_dots_kernel(int64_t n, const double* __restrict__ g_k,
                                                                const double* __restrict__ p, int64_t ld,
                                                                const idr_scalars* scal, double* __restrict__ part)
{
    __shared__ double smem[fblock / wave_size];
    if (idr_stopped(scal)) return;
    const pair_sweep sw(n);
    ptr_list<1 + S> in;
    in.p[0] = g_k;
#pragma unroll
    for (int j = 0; j < S; ++j) in.p[1 + j] = p + j * ld;
    double acc[S] = {};
    auto body = [&](int, const double* e) {
#pragma unroll
        for (int j = 0; j < S; ++j) acc[j] += e[1 + j] * e[0];
    };
    sw.loop(sw.i0, in.get(), body);
    sw.tail(in.get(), body);
    double* out[S];
#pragma unroll
    for (int j = 0; j < S; ++j) out[j] = part + j * max_parts;
    store_block_sums(false, acc, reinterpret_cast<double* const(&)[S]>(out), smem);
}

// PROJ(K)
template <int K>
__global__ __launch_bounds__(fblock) void idr_fused_project_kernel(int64_t n, int s, double* __restrict__ g,
                                                                   double* __restrict__ u, int64_t ld, double* m, int ms,
                                                                   const double* f_in, double* f_out,
                                                                   double* __restrict__ r, double* __restrict__ x,
                                                                   const double* __restrict__ d_part, int nparts,
                                                                   const idr_scalars* scal, double* __restrict__ rr_part)
{
    __shared__ double smem[fblock / wave_size];
    __shared__ double sd[fused_max_subspace], sa[fused_max_subspace], sbeta;
    if (idr_stopped(scal)) return;
    for (int j = 0; j < s; ++j) {
        const double dj = sum_partials(d_part + j * max_parts, nparts, smem);
        if (threadIdx.x == 0) sd[j] = dj;
    }
    if (threadIdx.x == 0) {
        for (int j = 0; j < K; ++j) {
            double a = sd[j];
            for (int i = 0; i < j; ++i) a -= m[j * ms + i] * sa[i];
            sa[j] = a / m[j * ms + j];
        }
        for (int j = K; j < s; ++j) {
            double mj = sd[j];
            for (int i = 0; i < K; ++i) mj -= m[j * ms + i] * sa[i];
            sd[j] = mj;
        }
        const double beta = f_in[K] / sd[K];
        sbeta = beta;
        if (blockIdx.x == 0) {
            // column K of m and the next f (idr_kernels.cpp:265-285); nobody reads either in this launch
            for (int j = K; j < s; ++j) m[j * ms + K] = sd[j];
            for (int j = 0; j < s; ++j) {
                f_out[j] = j < K || K + 1 >= s ? f_in[j] : (j == K ? 0.0 : f_in[j] - beta * sd[j]);
            }
        }
    }
    __syncthreads();
    double a[K > 0 ? K : 1];
#pragma unroll
    for (int i = 0; i < K; ++i) a[i] = sa[i];
    const double beta = sbeta;
    const pair_sweep sw(n);
    double acc[1] = {0.0};
    if constexpr (K == 0) {
        const double* const in[] = {g, u, r, x};
        double* const out[] = {r, x};
        sw.run(in, out, true, [&](int, const double* e, double* o) {
            o[0] = e[2] - beta * e[0];
            o[1] = e[3] + beta * e[1];
            acc[0] += o[0] * o[0];
        });
    } else {
        ptr_list<4 + 2 * K> in;
        in.p[0] = g + K * ld;
        in.p[1] = u + K * ld;
        in.p[2] = r;
        in.p[3] = x;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            in.p[4 + i] = g + i * ld;
            in.p[4 + K + i] = u + i * ld;
        }
        double* const out[] = {g + K * ld, u + K * ld, r, x};
        sw.run(in.get(), out, true, [&](int, const double* e, double* o) {
            double gk = e[0], uk = e[1];
#pragma unroll
            for (int i = 0; i < K; ++i) {
                gk -= a[i] * e[4 + i];
                uk -= a[i] * e[4 + K + i];
            }
            o[0] = gk;
            o[1] = uk;
            o[2] = e[2] - beta * gk;
            o[3] = e[3] + beta * uk;
            acc[0] += o[2] * o[2];
        });
    }
    double* const part[] = {rr_part};
    store_block_sums(true, acc, part, smem);
}

// CLOSE: IDENT = the preconditioned residual is r itself
template <int S, bool IDENT>
__global__ __launch_bounds__(fblock) void idr_fused_close_kernel(int64_t n, double* __restrict__ r,
                                                                 const double* __restrict__ t, double* __restrict__ x,
                                                                 const double* __restrict__ helper,
                                                                 const double* __restrict__ p, int64_t ld, double kappa,
                                                                 const double* __restrict__ tr_part,
                                                                 const double* __restrict__ tt_part, int nb,
                                                                 const double* __restrict__ rr_part, int nparts,
                                                                 idr_scalars* scal, double* __restrict__ part)
{
    __shared__ double smem[fblock / wave_size];
    if (idr_stopped(scal)) return;
    // idr::compute_omega
    const double thr = sum_partials(tr_part, nb, smem);
    const double tht = sum_partials(tt_part, nb, smem);
    const double residual_norm = sqrt(sum_partials(rr_part, nparts, smem));
    const double normt = sqrt(tht);
    double om = thr / tht;
    const double absrho = fabs(thr / (normt * residual_norm));
    if (absrho < kappa) om *= kappa / absrho;
    if (fused_leader()) scal->omega = om;
    const pair_sweep sw(n);
    constexpr int first_p = IDENT ? 3 : 4;
    ptr_list<first_p + S> in;
    in.p[0] = r;
    in.p[1] = t;
    in.p[2] = x;
    if (!IDENT) in.p[3] = helper;
#pragma unroll
    for (int j = 0; j < S; ++j) in.p[first_p + j] = p + j * ld;
    double acc[1 + S] = {};
    double* const out[] = {r, x};
    sw.run(in.get(), out, true, [&](int, const double* e, double* o) {
        o[0] = e[0] - om * e[1];
        o[1] = e[2] + om * (IDENT ? e[0] : e[3]);
        acc[0] += o[0] * o[0];
#pragma unroll
        for (int j = 0; j < S; ++j) acc[1 + j] += e[first_p + j] * o[0];
    });
    double* parts[1 + S];
#pragma unroll
    for (int j = 0; j <= S; ++j) parts[j] = part + j * max_parts;
    store_block_sums(true, acc, reinterpret_cast<double* const(&)[1 + S]>(parts), smem);
}

// pa[block] = sum a b, pb[block] = sum b b: after an apply of an operator without the dot epilogue
__global__ __launch_bounds__(fblock) void idr_fused_dot2_kernel(int64_t n, const double* __restrict__ a,
                                                                const double* __restrict__ b, const idr_scalars* scal,
                                                                double* __restrict__ pa, double* __restrict__ pb)
{
    __shared__ double smem[fblock / wave_size];
    if (idr_stopped(scal)) return;
    const pair_sweep sw(n);
    const double* const in[] = {a, b};
    double acc[2] = {0.0, 0.0};
    auto body = [&](int, const double* e) {
        acc[0] += e[0] * e[1];
        acc[1] += e[1] * e[1];
    };
    sw.loop(sw.i0, in, body);
    sw.tail(in, body);
    double* const part[] = {pa, pb};
    store_block_sums(false, acc, part, smem);
}

// f(std::integral_constant<int, v>) for 1 <= v <= 8
template <class F>
int dispatch_1_to_8(int v, F&& f)
{
    switch (v) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return GKOMI_ENOTSUPPORTED;
    }
}

// DOTS + PROJ(k) on column-major g, u, p: step 3 of the fused driver (also gkomi_idr_fused_step_3_f64)
int fused_step_3(hipStream_t stream, int grid, int64_t n, int s, int k, const double* p, double* g, double* u,
                 int64_t ld, double* m, int ms, const double* f_in, double* f_out, double* r, double* x,
                 const idr_scalars* scal, double* d_part, double* rr_part)
{
    GKOMI_TRY(dispatch_1_to_8(s, [&](auto S) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(idr_fused_dots_kernel<decltype(S)::value>), dim3(grid), dim3(fblock), 0, stream,
                           n, g + k * ld, p, ld, scal, d_part);
        return check_launch();
    }));
    return dispatch_1_to_8(k + 1, [&](auto K1) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(idr_fused_project_kernel<decltype(K1)::value - 1>), dim3(grid), dim3(fblock), 0,
                           stream, n, s, g, u, ld, m, ms, f_in, f_out, r, x, d_part, grid, scal, rr_part);
        return check_launch();
    });
}

int idr_fused_impl(const solve_request& req, const idr_params& prm)
{
    const gkomi_stream_t s = req.s;
    const int64_t n = req.n;
    if (prm.sdim > fused_max_subspace) return GKOMI_ENOTSUPPORTED;
    if (n < 0 || prm.sdim < 1 || prm.sdim > n || prm.subspace == nullptr) return GKOMI_EINVAL;
    bool reference;
    GKOMI_TRY(fused_preflight(req, &reference));
    if (reference) return idr_solve_impl(req, prm);
    const int sdim = static_cast<int>(prm.sdim);
    const idr_layout l = make_idr_layout(n, 1, sdim);
    driver_common c;
    GKOMI_TRY(c.init(req, 2 * sdim + 6, l.base, l.total));
    // every vector in the workspace is read 16 B per lane
    if (reinterpret_cast<uintptr_t>(req.workspace) % 16 != 0) return GKOMI_EINVAL;
    char* ws = c.ws;
    const sysmat& A = c.A;
    double* x = req.x;
    auto D = [&](size_t at) { return reinterpret_cast<double*>(ws + at); };
    double *r = c.vec(0), *v = c.vec(1), *t = c.vec(2), *helper = c.vec(3);
    double *g = D(l.g), *u = D(l.u), *m = D(l.m), *f = D(l.f), *p = D(l.pcopy);
    double *part_f = D(l.parts), *part_d = part_f + (sdim + 1) * max_parts, *part_rr = part_d + sdim * max_parts;
    const int64_t ld = l.ld;
    const int ms = fused_max_subspace;
    hipStream_t stream = c.stream;
    // m = I (row stride ms), P orthonormalised in place as the caller will find it, then copied to the even stride
    GKOMI_TRY(gkomi_idr_initialize_f64(s, n, 1, sdim, m, ms, prm.subspace, n, c.stop_status));
    GKOMI_TRY(gkomi_dense_copy_f64(s, sdim, n, prm.subspace, n, p, ld));
    GKOMI_TRY(gkomi_dense_copy_f64(s, n, 1, req.b, 1, r, 1));
    GKOMI_TRY(c.start(req, r));
    GKOMI_TRY(static_cast<int>(hipMemsetAsync(g, 0, sizeof(double) * ld * sdim, stream)));
    GKOMI_TRY(static_cast<int>(hipMemsetAsync(u, 0, sizeof(double) * ld * sdim, stream)));
    fused_driver<idr_scalars> fd(c);
    idr_scalars* scal = fd.scal;
    double *part_tr = fd.spmv_partials(), *part_tt = fd.spmv_partials();
    const int grid = fd.g, nb = fd.nb;
    const spmv_dot_plan& spmv = fd.spmv;
    const bool ident = c.precond == nullptr;
    GKOMI_TRY(dispatch_1_to_8(sdim, [&](auto S) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(idr_fused_start_kernel<decltype(S)::value>), dim3(grid), dim3(fblock), 0, stream,
                           n, r, p, ld, scal, c.orig_tau, part_f);
        return check_launch();
    }));
    host_watch& watch = fd.watch;
    const long long limit = static_cast<long long>(c.max_iters);
    auto step_1 = [&](int k, long long it) {
        return dispatch_1_to_8(sdim - k, [&](auto NJ) {
            constexpr int nj = decltype(NJ)::value;
            if (ident) {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(idr_fused_step_1_kernel<nj, true>), dim3(grid), dim3(fblock), 0, stream,
                                   n, sdim, k, r, g, u, ld, v, m, ms, f + (k & 1) * ms, part_f, grid, scal, it, limit,
                                   c.reduction, watch.dev);
            } else {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(idr_fused_step_1_kernel<nj, false>), dim3(grid), dim3(fblock), 0, stream,
                                   n, sdim, k, r, g, u, ld, v, m, ms, f + (k & 1) * ms, part_f, grid, scal, it, limit,
                                   c.reduction, watch.dev);
            }
            return check_launch();
        });
    };
    auto issue = [&](long long it, bool last) -> int {
        GKOMI_TRY(step_1(0, it));
        if (last) return 0;
        for (int k = 0; k < sdim; ++k) {
            if (k > 0) GKOMI_TRY(step_1(k, it));
            if (!ident) {
                GKOMI_TRY(c.apply_precond(v, helper));
                GKOMI_TRY(dispatch_1_to_8(sdim - k, [&](auto NJ) {
                    hipLaunchKernelGGL(HIP_KERNEL_NAME(idr_fused_step_2_kernel<decltype(NJ)::value>), dim3(grid),
                                       dim3(fblock), 0, stream, n, sdim, k, helper, u, ld, m, ms, f + (k & 1) * ms, scal);
                    return check_launch();
                }));
            }
            GKOMI_TRY(A.apply(s, 1, nullptr, u + k * ld, nullptr, g + k * ld));
            GKOMI_TRY(fused_step_3(stream, grid, n, sdim, k, p, g, u, ld, m, ms, f + (k & 1) * ms, f + ((k + 1) & 1) * ms,
                                   r, x, scal, part_d, part_rr));
        }
        const double* pr = r;
        if (!ident) {
            GKOMI_TRY(c.apply_precond(r, helper));
            pr = helper;
        }
        if (spmv.fused()) {
            GKOMI_TRY(spmv.launch(stream, pr, t, part_tr, &scal->status, r, part_tt));
        } else {
            GKOMI_TRY(A.apply(s, 1, nullptr, pr, nullptr, t));
            hipLaunchKernelGGL(idr_fused_dot2_kernel, dim3(grid), dim3(fblock), 0, stream, n, r, t, scal, part_tr, part_tt);
            GKOMI_TRY(check_launch());
        }
        return dispatch_1_to_8(sdim, [&](auto S) {
            constexpr int sv = decltype(S)::value;
            if (ident) {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(idr_fused_close_kernel<sv, true>), dim3(grid), dim3(fblock), 0, stream, n,
                                   r, t, x, helper, p, ld, prm.kappa, part_tr, part_tt, nb, part_rr, grid, scal, part_f);
            } else {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(idr_fused_close_kernel<sv, false>), dim3(grid), dim3(fblock), 0, stream,
                                   n, r, t, x, helper, p, ld, prm.kappa, part_tr, part_tt, nb, part_rr, grid, scal, part_f);
            }
            return check_launch();
        });
    };
    return fd.solve(issue, req.host_info);
}

}  // namespace
}  // namespace gkomi

using namespace gkomi;

// ---- kernel entry points --------------------------------------------------------------------------------------------
extern "C" int gkomi_idr_initialize_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, int64_t subspace_dim, double* m,
                                        int64_t m_stride, double* subspace_vectors, int64_t subspace_stride,
                                        uint8_t* stop_status)
{
    if (bad_idr_dims(n, nrhs, subspace_dim, 0) || subspace_dim > n) return GKOMI_EINVAL;
    hipStream_t stream = to_stream(s);
    if (nrhs > 0) {
        hipLaunchKernelGGL(idr_initialize_m_kernel, grid_of(subspace_dim * subspace_dim, nrhs), dim3(block), 0, stream, nrhs,
                           subspace_dim, m, m_stride, stop_status);
    }
    hipLaunchKernelGGL(idr_orthonormalize_kernel, dim3(1), dim3(fblock), 0, stream, subspace_dim, n, subspace_vectors,
                       subspace_stride);
    return check_launch();
}

extern "C" int gkomi_idr_step_1_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, int64_t subspace_dim, int64_t k,
                                    const double* m, int64_t m_stride, const double* f, int64_t f_stride,
                                    const double* residual, int64_t residual_stride, const double* g, int64_t g_stride,
                                    double* c, int64_t c_stride, double* v, int64_t v_stride, const uint8_t* stop_status)
{
    if (bad_idr_dims(n, nrhs, subspace_dim, k)) return GKOMI_EINVAL;
    if (nrhs == 0) return GKOMI_SUCCESS;
    hipStream_t stream = to_stream(s);
    hipLaunchKernelGGL(idr_solve_lower_kernel, cols_grid(nrhs), dim3(block), 0, stream, nrhs, subspace_dim, m, m_stride, f,
                       f_stride, c, c_stride, stop_status);
    if (n > 0) {
        hipLaunchKernelGGL(idr_step_1_kernel, grid_of(n, nrhs), dim3(block), 0, stream, n, nrhs, subspace_dim, k, residual,
                           residual_stride, g, g_stride, c, c_stride, v, v_stride, stop_status);
    }
    return check_launch();
}

extern "C" int gkomi_idr_step_2_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, int64_t subspace_dim, int64_t k,
                                    const double* omega, const double* preconditioned_vector, int64_t pv_stride,
                                    const double* c, int64_t c_stride, double* u, int64_t u_stride,
                                    const uint8_t* stop_status)
{
    if (bad_idr_dims(n, nrhs, subspace_dim, k)) return GKOMI_EINVAL;
    if (n == 0 || nrhs == 0) return GKOMI_SUCCESS;
    hipLaunchKernelGGL(idr_step_2_kernel, grid_of(n, nrhs), dim3(block), 0, to_stream(s), n, nrhs, subspace_dim, k, omega,
                       preconditioned_vector, pv_stride, c, c_stride, u, u_stride, stop_status);
    return check_launch();
}

extern "C" size_t gkomi_idr_step_3_workspace_bytes(int64_t nrhs, int64_t subspace_dim)
{
    if (nrhs < 0 || subspace_dim < 1 || subspace_dim > max_subspace) return 0;
    return sizeof(double) * dot_blocks * static_cast<size_t>(subspace_dim) * static_cast<size_t>(nrhs);
}

extern "C" int gkomi_idr_step_3_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, int64_t subspace_dim, int64_t k,
                                    const double* subspace_vectors, int64_t subspace_stride, double* g, int64_t g_stride,
                                    double* g_k, int64_t g_k_stride, double* u, int64_t u_stride, double* m,
                                    int64_t m_stride, double* f, int64_t f_stride, double* alpha, double* residual,
                                    int64_t residual_stride, double* x, int64_t x_stride, const uint8_t* stop_status,
                                    void* workspace, size_t workspace_bytes)
{
    if (bad_idr_dims(n, nrhs, subspace_dim, k)) return GKOMI_EINVAL;
    if (nrhs == 0) return GKOMI_SUCCESS;
    if (workspace == nullptr || workspace_bytes < gkomi_idr_step_3_workspace_bytes(nrhs, subspace_dim)) {
        return GKOMI_EWORKSPACE;
    }
    hipStream_t stream = to_stream(s);
    double* ws = static_cast<double*>(workspace);
    const double* p = subspace_vectors;
    // update_g_and_u: k sequential dot / update pairs
    for (int64_t j = 0; j < k; ++j) {
        GKOMI_TRY(multidot(stream, n, nrhs, 1, p + j * subspace_stride, subspace_stride, g_k, g_k_stride, alpha, nrhs,
                           m + j * m_stride + j * nrhs, ws, stop_status));
        if (n > 0) {
            hipLaunchKernelGGL(idr_update_g_and_u_kernel, grid_of(n, nrhs), dim3(block), 0, stream, n, nrhs, k, j, alpha, g,
                               g_stride, g_k, g_k_stride, u, u_stride, stop_status);
        }
    }
    // m_jk = p_j . g_k for j >= k
    GKOMI_TRY(multidot(stream, n, nrhs, subspace_dim - k, p + k * subspace_stride, subspace_stride, g_k, g_k_stride,
                       m + k * m_stride + k * nrhs, m_stride, nullptr, ws, stop_status));
    if (n > 0) {
        hipLaunchKernelGGL(idr_step_3_update_kernel, grid_of(n, nrhs), dim3(block), 0, stream, n, nrhs, k, f, f_stride, m,
                           m_stride, g, g_stride, g_k, g_k_stride, u, u_stride, residual, residual_stride, x, x_stride,
                           stop_status);
    }
    hipLaunchKernelGGL(idr_step_3_f_kernel, cols_grid(nrhs), dim3(block), 0, stream, nrhs, subspace_dim, k, f, f_stride, m,
                       m_stride, stop_status);
    return check_launch();
}

extern "C" int gkomi_idr_compute_omega_f64(gkomi_stream_t s, int64_t nrhs, double kappa, const double* tht,
                                           const double* residual_norm, double* omega, const uint8_t* stop_status)
{
    if (nrhs < 0) return GKOMI_EINVAL;
    if (nrhs == 0) return GKOMI_SUCCESS;
    hipLaunchKernelGGL(idr_compute_omega_kernel, cols_grid(nrhs), dim3(block), 0, to_stream(s), nrhs, kappa, tht,
                       residual_norm, omega, stop_status);
    return check_launch();
}

extern "C" size_t gkomi_idr_fused_step_3_workspace_bytes(int64_t subspace_dim)
{
    if (subspace_dim < 1 || subspace_dim > fused_max_subspace) return 0;
    return 256 + sizeof(double) * static_cast<size_t>(subspace_dim + 1) * max_parts;
}

extern "C" int gkomi_idr_fused_step_3_f64(gkomi_stream_t s, int64_t n, int64_t subspace_dim, int64_t k,
                                          const double* subspace_vectors, double* g, double* u, int64_t ld, double* m,
                                          const double* f_in, double* f_out, double* residual, double* x, void* workspace,
                                          size_t workspace_bytes)
{
    if (subspace_dim > fused_max_subspace) return GKOMI_ENOTSUPPORTED;
    if (bad_idr_dims(n, 1, subspace_dim, k) || ld < n || (ld & 1) || n > INT32_MAX - 1024) return GKOMI_EINVAL;
    for (const void* ptr : {static_cast<const void*>(subspace_vectors), static_cast<const void*>(g),
                            static_cast<const void*>(u), static_cast<const void*>(residual), static_cast<const void*>(x)}) {
        if (reinterpret_cast<uintptr_t>(ptr) % 16 != 0) return GKOMI_EINVAL;
    }
    if (workspace == nullptr || reinterpret_cast<uintptr_t>(workspace) % 8 != 0 ||
        workspace_bytes < gkomi_idr_fused_step_3_workspace_bytes(subspace_dim)) {
        return GKOMI_EWORKSPACE;
    }
    hipStream_t stream = to_stream(s);
    GKOMI_TRY(static_cast<int>(hipMemsetAsync(workspace, 0, 256, stream)));  // scalars: not stopped
    auto* scal = static_cast<idr_scalars*>(workspace);
    double* d_part = reinterpret_cast<double*>(static_cast<char*>(workspace) + 256);
    const int sdim = static_cast<int>(subspace_dim);
    return fused_step_3(stream, fused_vec_grid(n), n, sdim, static_cast<int>(k), subspace_vectors, g, u, ld, m, sdim, f_in,
                        f_out, residual, x, scal, d_part, d_part + subspace_dim * max_parts);
}

// ---- drivers ----------------------------------------------------------------------------------------------------------
extern "C" size_t gkomi_idr_workspace_bytes(int64_t n, int64_t nrhs, int64_t subspace_dim)
{
    if (n < 0 || nrhs <= 0 || subspace_dim < 1 || subspace_dim > max_subspace) return 0;
    return make_idr_layout(n, nrhs, subspace_dim).total;
}

extern "C" int gkomi_idr_solve_f64_i32(gkomi_stream_t s, int64_t n, int64_t nrhs, int64_t nnz, const int32_t* row_ptrs,
                                       const int32_t* col_idxs, const double* vals, int spmv_strategy,
                                       int64_t max_row_nnz_hint, gkomi_apply_fn precond, void* precond_ctx,
                                       int64_t subspace_dim, double kappa, double* subspace, const double* b, double* x,
                                       int64_t max_iters, double reduction_factor, int baseline, int64_t check_every,
                                       void* workspace, size_t workspace_bytes, double* host_info)
{
    return idr_solve_impl({s, n, nrhs, make_csr_sysmat(n, nnz, row_ptrs, col_idxs, vals, spmv_strategy, max_row_nnz_hint),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, check_every, workspace, workspace_bytes,
        host_info}, {subspace_dim, kappa, subspace});
}

extern "C" int gkomi_idr_solve_op_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, gkomi_matrix_apply_fn matrix,
                                      void* matrix_ctx, gkomi_apply_fn precond, void* precond_ctx, int64_t subspace_dim,
                                      double kappa, double* subspace, const double* b, double* x, int64_t max_iters,
                                      double reduction_factor, int baseline, int64_t check_every, void* workspace,
                                      size_t workspace_bytes, double* host_info)
{
    if (matrix == nullptr) return GKOMI_EINVAL;
    return idr_solve_impl({s, n, nrhs, make_op_sysmat(n, matrix, matrix_ctx),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, check_every, workspace, workspace_bytes,
        host_info}, {subspace_dim, kappa, subspace});
}

extern "C" int gkomi_idr_solve_fused_f64_i32(gkomi_stream_t s, int64_t n, int64_t nrhs, int64_t nnz,
                                             const int32_t* row_ptrs, const int32_t* col_idxs, const double* vals,
                                             int spmv_strategy, int64_t max_row_nnz_hint, gkomi_apply_fn precond,
                                             void* precond_ctx, int64_t subspace_dim, double kappa, double* subspace,
                                             const double* b, double* x, int64_t max_iters, double reduction_factor,
                                             int baseline, int64_t check_every, void* workspace, size_t workspace_bytes,
                                             double* host_info)
{
    if (nrhs != 1) return GKOMI_ENOTSUPPORTED;
    return idr_fused_impl({s, n, nrhs, make_csr_sysmat(n, nnz, row_ptrs, col_idxs, vals, spmv_strategy, max_row_nnz_hint),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, check_every, workspace, workspace_bytes,
        host_info}, {subspace_dim, kappa, subspace});
}

extern "C" int gkomi_idr_solve_fused_op_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, gkomi_matrix_apply_fn matrix,
                                            void* matrix_ctx, gkomi_apply_fn precond, void* precond_ctx,
                                            int64_t subspace_dim, double kappa, double* subspace, const double* b,
                                            double* x, int64_t max_iters, double reduction_factor, int baseline,
                                            int64_t check_every, void* workspace, size_t workspace_bytes, double* host_info)
{
    if (nrhs != 1) return GKOMI_ENOTSUPPORTED;
    if (matrix == nullptr) return GKOMI_EINVAL;
    return idr_fused_impl({s, n, nrhs, make_op_sysmat(n, matrix, matrix_ctx),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, check_every, workspace, workspace_bytes,
        host_info}, {subspace_dim, kappa, subspace});
}
