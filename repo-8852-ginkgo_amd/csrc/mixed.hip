// Mixed precision: components::convert_precision<double <-> float> (core/components/precision_conversion_kernels.hpp:53,
// common/unified/components/precision_conversion_kernels.cpp), a device-resident Cg<float> (the three-launch iteration of
// cg_solver.hip's mode 1 on float vectors and a float matrix) and Ir<double> with that Cg<float> as its inner solver
// (core/solver/ir.cpp:188-277 behind precision_dispatch, include/ginkgo/core/base/precision_dispatch.hpp:73-96).
//
// Fused float CG, one right-hand side, Identity preconditioner, Combined(Iteration, ResidualNorm):
//   K1 : re-adds the r.r partials (double), evaluates the criterion, p = r + (rho/prev_rho) p
//   K2 : q = A p (float row-cut LDS SpMV, f32.hip's design, grid-strided over row blocks) + p.q partials (double)
//   K3 : re-adds the p.q partials, x += (rho/beta) p, r -= (rho/beta) q, leaves the r.r partials
// Vectors and matrix are float, every partial sum a double.  Bytes per iteration (n rows, nnz nonzeros): matrix 8 nnz +
// row pointers 4 n, vectors K1 3 n + K2 (gathers of p) n + q n + K3 6 n = 11 n floats -- 0.58x the double iteration.
//
// MPIR, per outer iteration: r = b - A x in double (the automatic CSR apply), one kernel converts r to float into the
// inner right-hand side AND the inner initial guess and leaves the ||r||^2 partials, one single-workgroup kernel
// evaluates the outer criterion (and folds the last inner solve's iteration count into the device totals), one look of
// the host at that state, the inner fused CG (no look of its own: it follows the host_watch line), then one kernel
// x += relaxation * (double) d.
#include "cg_fused.hpp"

#include <algorithm>
#include <cmath>

namespace gkomi {
namespace {

// ---- convert_precision --------------------------------------------------------------------------------------------
constexpr int cblock = 256;

// contiguous, both sides 16-B aligned: four values per lane and sweep (f64 -> f32: 32 B in, 16 B out)
template <typename In, typename Out>
__global__ __launch_bounds__(cblock) void convert_quad_kernel(int64_t total, const In* __restrict__ in, Out* __restrict__ out)
{
    const int64_t nquads = total / 4;
    const int64_t step = static_cast<int64_t>(gridDim.x) * cblock;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(cblock) + threadIdx.x; i < nquads; i += step) {
        if constexpr (sizeof(In) == 8) {
            const double2 a = reinterpret_cast<const double2*>(in)[2 * i];
            const double2 b = reinterpret_cast<const double2*>(in)[2 * i + 1];
            reinterpret_cast<float4*>(out)[i] =
                make_float4(static_cast<float>(a.x), static_cast<float>(a.y), static_cast<float>(b.x), static_cast<float>(b.y));
        } else {
            const float4 a = reinterpret_cast<const float4*>(in)[i];
            reinterpret_cast<double2*>(out)[2 * i] = make_double2(a.x, a.y);
            reinterpret_cast<double2*>(out)[2 * i + 1] = make_double2(a.z, a.w);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < total - 4 * nquads) {
        const int64_t k = 4 * nquads + threadIdx.x;
        out[k] = static_cast<Out>(in[k]);
    }
}

// any strides: one lane per entry, the padding between rows untouched
template <typename In, typename Out>
__global__ __launch_bounds__(cblock) void convert_strided_kernel(int64_t nrows, int64_t ncols, const In* __restrict__ in,
                                                                 int64_t in_stride, Out* __restrict__ out, int64_t out_stride)
{
    const int64_t total = nrows * ncols;
    const int64_t step = static_cast<int64_t>(gridDim.x) * cblock;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(cblock) + threadIdx.x; i < total; i += step) {
        const int64_t row = i / ncols, col = i - row * ncols;
        out[row * out_stride + col] = static_cast<Out>(in[row * in_stride + col]);
    }
}

template <typename In, typename Out>
int convert(gkomi_stream_t s, int64_t nrows, int64_t ncols, const In* in, int64_t in_stride, Out* out, int64_t out_stride)
{
    if (nrows < 0 || ncols < 0) return GKOMI_EINVAL;
    if (nrows == 0 || ncols == 0) return GKOMI_SUCCESS;
    if (in == nullptr || out == nullptr || in_stride < ncols || out_stride < ncols) return GKOMI_EINVAL;
    const bool contiguous = nrows == 1 || (in_stride == ncols && out_stride == ncols);
    const bool aligned = reinterpret_cast<uintptr_t>(in) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const int64_t total = nrows * ncols;
    if (contiguous && aligned) {
        hipLaunchKernelGGL((convert_quad_kernel<In, Out>), dim3(grid_for(total / 4 + 1, cblock)), dim3(cblock), 0, to_stream(s), total,
                           in, out);
    } else {
        hipLaunchKernelGGL((convert_strided_kernel<In, Out>), dim3(grid_for(total, cblock)), dim3(cblock), 0, to_stream(s), nrows, ncols,
                           in, in_stride, out, out_stride);
    }
    return check_launch();
}

// ---- fused Cg<float> ----------------------------------------------------------------------------------------------
constexpr int sblock = 256;       // SpMV: rows per row block = threads per workgroup
constexpr int stile = 2048;       // nonzeros per LDS tile
constexpr int spmv_max_grid = 2048;  // row blocks beyond that are grid-strided: at most this many p.q partials

int f32_vec_grid(int64_t n)
{
    static const int64_t resident = 2 * static_cast<int64_t>(device_cu_count());
    int64_t g = ceildiv(n / 4 + 1, fblock);
    if (g > max_parts) g = max_parts;
    if (resident > 0 && g > resident) g = resident;
    return static_cast<int>(std::max<int64_t>(g, 1));
}

int f32_spmv_grid(int64_t n) { return static_cast<int>(std::min<int64_t>(std::max<int64_t>(ceildiv(n, sblock), 1), spmv_max_grid)); }

__global__ __launch_bounds__(fblock) void cgf_sq_partials_kernel(int64_t n, const float* __restrict__ v, double* __restrict__ part)
{
    __shared__ double smem[fblock / wave_size];
    double acc = 0.0;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(fblock) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * fblock) {
        const double x = v[i];
        acc += x * x;
    }
    const double t = block_reduce_sum<fblock>(acc, smem);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// scalars of a new solve: baseline norm from `base_part` (rhs or initial residual) or 1 (absolute)
__global__ __launch_bounds__(fblock) void cgf_init_kernel(cg_scalars* scal, const double* __restrict__ base_part, int nparts,
                                                          int baseline_absolute)
{
    __shared__ double smem[fblock / wave_size];
    const double orig = baseline_absolute ? 1.0 : sqrt(sum_partials(base_part, nparts, smem));
    if (threadIdx.x == 0) {
        init_fused_scalars(scal, 0.0, orig);
        scal->beta = 0.0;
    }
}

// K1 (Identity: rho = r.r = tau^2)
__global__ __launch_bounds__(fblock) void cgf_step1_kernel(int64_t n, float* __restrict__ p, const float* __restrict__ r,
                                                           const double* __restrict__ rr_part, int nparts, cg_scalars* scal,
                                                           long long it, long long max_iters, double goal,
                                                           host_watch_line* watch)
{
    __shared__ double smem[fblock / wave_size];
    if (fused_stopped_before(status_has_stopped(scal->status), scal, watch, it)) return;
    const double rho = sum_partials(rr_part, nparts, smem);
    if (fused_criterion(scal, watch, it, max_iters, rho, sqrt(rho), goal, id_iteration, id_residual)) return;
    const double prev = scal->rho[(it + 1) & 1];
    const bool restart = prev == 0.0;
    const float tmp = restart ? 0.0f : static_cast<float>(rho / prev);
    const int64_t n4 = n / 4;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* r4 = reinterpret_cast<const float4*>(r);
    for (int64_t i = blockIdx.x * static_cast<int64_t>(fblock) + threadIdx.x; i < n4; i += static_cast<int64_t>(gridDim.x) * fblock) {
        float4 v = r4[i];
        if (!restart) {
            const float4 pv = p4[i];
            v.x = v.x + tmp * pv.x;
            v.y = v.y + tmp * pv.y;
            v.z = v.z + tmp * pv.z;
            v.w = v.w + tmp * pv.w;
        }
        p4[i] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x < n - 4 * n4) {
        const int64_t k = 4 * n4 + threadIdx.x;
        p[k] = restart ? r[k] : r[k] + tmp * p[k];
    }
}

// K2: q = A p, partial[blockIdx.x] = sum of p * q over the workgroup's row blocks
__global__ __launch_bounds__(sblock) void cgf_spmv_dot_kernel(int nrows, const int32_t* __restrict__ row_ptrs,
                                                              const int32_t* __restrict__ col_idxs, const float* __restrict__ vals,
                                                              const float* __restrict__ p, float* __restrict__ q,
                                                              double* __restrict__ part, const uint8_t* __restrict__ status)
{
    __shared__ float prod[stile];
    __shared__ double smem[sblock / wave_size];
    if (status_has_stopped_uniform(status)) return;
    double acc = 0.0;
    for (int64_t blk = blockIdx.x; blk * sblock < nrows; blk += gridDim.x) {
        const int r0 = static_cast<int>(blk * sblock);
        const int r1 = min(r0 + sblock, nrows);
        const int row = r0 + threadIdx.x;
        const bool mine = row < r1;
        const int ra = mine ? row_ptrs[row] : 0;
        const int rb = mine ? row_ptrs[row + 1] : 0;
        const int p0 = row_ptrs[r0], p1 = row_ptrs[r1];
        float sum = 0.0f;
        for (int base = p0; base < p1; base += stile) {
            const int count = min(stile, p1 - base);
            for (int i = threadIdx.x; i < count; i += sblock) prod[i] = vals[base + i] * p[col_idxs[base + i]];
            __syncthreads();
            const int lo = max(ra, base) - base, hi = min(rb, base + count) - base;
            for (int k = lo; k < hi; ++k) sum = sum + prod[k];
            __syncthreads();
        }
        if (mine) {
            q[row] = sum;
            acc += static_cast<double>(p[row]) * static_cast<double>(sum);
        }
    }
    const double t = block_reduce_sum<sblock>(acc, smem);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// K3
__global__ __launch_bounds__(fblock) void cgf_step2_kernel(int64_t n, float* __restrict__ x, float* __restrict__ r,
                                                           const float* __restrict__ p, const float* __restrict__ q,
                                                           const double* __restrict__ pq_part, int npq, cg_scalars* scal,
                                                           long long it, double* __restrict__ rr_part)
{
    __shared__ double smem[fblock / wave_size];
    if (status_has_stopped(scal->status)) return;
    const double beta = sum_partials(pq_part, npq, smem);
    const double rho = scal->rho[it & 1];
    const bool update = beta != 0.0;
    const float tmp = update ? static_cast<float>(rho / beta) : 0.0f;
    if (blockIdx.x == 0 && threadIdx.x == 0) scal->beta = beta;
    const int64_t n4 = n / 4;
    float4* x4 = reinterpret_cast<float4*>(x);
    float4* r4 = reinterpret_cast<float4*>(r);
    const float4* p4 = reinterpret_cast<const float4*>(p);
    const float4* q4 = reinterpret_cast<const float4*>(q);
    double acc = 0.0;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(fblock) + threadIdx.x; i < n4; i += static_cast<int64_t>(gridDim.x) * fblock) {
        float4 rv = r4[i];
        if (update) {
            float4 xv = x4[i];
            const float4 pv = p4[i], qv = q4[i];
            xv.x = xv.x + tmp * pv.x;
            xv.y = xv.y + tmp * pv.y;
            xv.z = xv.z + tmp * pv.z;
            xv.w = xv.w + tmp * pv.w;
            rv.x = rv.x - tmp * qv.x;
            rv.y = rv.y - tmp * qv.y;
            rv.z = rv.z - tmp * qv.z;
            rv.w = rv.w - tmp * qv.w;
            x4[i] = xv;
            r4[i] = rv;
        }
        acc += static_cast<double>(rv.x) * rv.x + static_cast<double>(rv.y) * rv.y + static_cast<double>(rv.z) * rv.z +
               static_cast<double>(rv.w) * rv.w;
    }
    if (blockIdx.x == 0 && threadIdx.x < n - 4 * n4) {
        const int64_t k = 4 * n4 + threadIdx.x;
        if (update) {
            x[k] = x[k] + tmp * p[k];
            r[k] = r[k] - tmp * q[k];
        }
        const double rk = r[k];
        acc += rk * rk;
    }
    __syncthreads();  // smem of sum_partials is read by every thread above
    const double t = block_reduce_sum<fblock>(acc, smem);
    if (threadIdx.x == 0) rr_part[blockIdx.x] = t;
}

struct cgf_layout {
    size_t r, p, q, scal, part_rr, part_pq, part_base, small, total;
};

cgf_layout make_cgf_layout(int64_t n)
{
    cgf_layout l{};
    const size_t vec = align256(sizeof(float) * static_cast<size_t>(n > 0 ? n : 1));
    const size_t parts = align256(sizeof(double) * std::max(max_parts, spmv_max_grid));
    size_t off = 0;
    l.r = off; off += vec;
    l.p = off; off += vec;
    l.q = off; off += vec;
    l.scal = off; off += 256;
    l.part_rr = off; off += parts;
    l.part_pq = off; off += parts;
    l.part_base = off; off += parts;
    l.small = off; off += 256;  // the float scalars 1 and -1 of r = b - A x
    l.total = off;
    return l;
}

// The whole inner solve issued on `s`; returns once the host knows that it has stopped (the host_watch line, or a look
// every 16 iterations when the line is not available).  The final state stays in the device scalars *scal_out: the caller
// looks at them when it needs them.
int cgf_run(gkomi_stream_t s, int64_t n, int64_t nnz, const int32_t* row_ptrs, const int32_t* col_idxs, const float* vals,
            const float* b, float* x, int64_t max_iters, double reduction, int baseline, char* ws, cg_scalars** scal_out)
{
    const cgf_layout l = make_cgf_layout(n);
    hipStream_t stream = to_stream(s);
    float* r = reinterpret_cast<float*>(ws + l.r);
    float* p = reinterpret_cast<float*>(ws + l.p);
    float* q = reinterpret_cast<float*>(ws + l.q);
    cg_scalars* scal = reinterpret_cast<cg_scalars*>(ws + l.scal);
    double* part_rr = reinterpret_cast<double*>(ws + l.part_rr);
    double* part_pq = reinterpret_cast<double*>(ws + l.part_pq);
    double* part_base = reinterpret_cast<double*>(ws + l.part_base);
    float* one = reinterpret_cast<float*>(ws + l.small);
    float* neg = one + 1;
    *scal_out = scal;
    const int g = f32_vec_grid(n), gs = f32_spmv_grid(n);
    // cg::initialize (r = b, p = 0, prev_rho = 1) and r = b - A x (cg.cpp:137-142)
    GKOMI_TRY(gkomi_dense_copy_f32(s, n, 1, b, 1, r, 1));
    GKOMI_TRY(gkomi_dense_fill_f32(s, n, 1, p, 1, 0.0f));
    GKOMI_TRY(gkomi_dense_fill_f32(s, 1, 1, one, 1, 1.0f));
    GKOMI_TRY(gkomi_dense_fill_f32(s, 1, 1, neg, 1, -1.0f));
    GKOMI_TRY(gkomi_csr_spmv_f32_i32(s, n, n, 1, nnz, row_ptrs, col_idxs, vals, x, 1, r, 1, neg, one));
    hipLaunchKernelGGL(cgf_sq_partials_kernel, dim3(g), dim3(fblock), 0, stream, n, r, part_rr);
    if (baseline == 0) hipLaunchKernelGGL(cgf_sq_partials_kernel, dim3(g), dim3(fblock), 0, stream, n, b, part_base);
    hipLaunchKernelGGL(cgf_init_kernel, dim3(1), dim3(fblock), 0, stream, scal, baseline == 0 ? part_base : part_rr, g,
                       baseline == 2 ? 1 : 0);
    GKOMI_TRY(check_launch());
    host_watch watch;
    auto issue = [&](long long i, bool) -> int {
        hipLaunchKernelGGL(cgf_step1_kernel, dim3(g), dim3(fblock), 0, stream, n, p, r, part_rr, g, scal, i,
                           static_cast<long long>(max_iters), reduction, watch.dev);
        hipLaunchKernelGGL(cgf_spmv_dot_kernel, dim3(gs), dim3(sblock), 0, stream, static_cast<int>(n), row_ptrs, col_idxs, vals,
                           p, q, part_pq, &scal->status);
        hipLaunchKernelGGL(cgf_step2_kernel, dim3(g), dim3(fblock), 0, stream, n, x, r, p, q, part_pq, gs, scal, i, part_rr);
        return check_launch();
    };
    auto look = [&]() -> int {  // (only without the line: the status byte alone)
        uint8_t st = 0;
        const int err = read_scalars(stream, &st, &scal->status);
        return err ? -err : (st & GKOMI_STATUS_ID_MASK) != 0;
    };
    bool looked = false;  // (not needed: the callers read the scalars themselves)
    return pace_fused_solve(stream, &watch, max_iters, /*check_every=*/16, /*lag=*/4 * host_watch_lag, issue, look, &looked);
}

int cgf_check_args(int64_t n, int64_t nnz, int64_t max_iters, int baseline, const float* b, const float* x)
{
    if (n < 0 || nnz < 0 || max_iters < 0 || baseline < 0 || baseline > 2) return GKOMI_EINVAL;
    if (n > INT32_MAX - 1024 || nnz > INT32_MAX) return GKOMI_ENOTSUPPORTED;
    // K1 / K3 move 16 B per lane through x (the workspace vectors are 256-B aligned)
    if (reinterpret_cast<uintptr_t>(x) % 16 != 0) return GKOMI_ENOTSUPPORTED;
    (void)b;
    return GKOMI_SUCCESS;
}

// ---- Ir<double> over the fused Cg<float> ---------------------------------------------------------------------------
struct ir_state {
    double tau;        // ||b - A x|| at the last check
    double orig_tau;   // baseline norm
    long long inner_iters, inner_capped;
    long long stop_iter;
    unsigned char status;
    unsigned char pad[7];
};

// rf = df = (float) r, partial[blockIdx.x] = sum of r^2 (double)
__global__ __launch_bounds__(fblock) void ir_demote_kernel(int64_t n, const double* __restrict__ r, float* __restrict__ rf,
                                                           float* __restrict__ df, double* __restrict__ part)
{
    __shared__ double smem[fblock / wave_size];
    double acc = 0.0;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(fblock) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * fblock) {
        const double v = r[i];
        const float f = static_cast<float>(v);
        rf[i] = f;
        df[i] = f;
        acc += v * v;
    }
    const double t = block_reduce_sum<fblock>(acc, smem);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ __launch_bounds__(fblock) void ir_sq_partials_kernel(int64_t n, const double* __restrict__ v, double* __restrict__ part)
{
    __shared__ double smem[fblock / wave_size];
    double acc = 0.0;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(fblock) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * fblock) {
        acc += v[i] * v[i];
    }
    const double t = block_reduce_sum<fblock>(acc, smem);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// the outer criterion (Combined(Iteration, ResidualNorm), ir.cpp:218-257) on ||r||; before that, the inner solve that
// ran since the last check (if any) is counted
__global__ __launch_bounds__(fblock) void ir_check_kernel(ir_state* st, const double* __restrict__ r_part,
                                                          const double* __restrict__ b_part, int nparts, long long it,
                                                          long long max_iters, double goal, int baseline,
                                                          const cg_scalars* inner)
{
    __shared__ double smem[fblock / wave_size];
    const double tau = sqrt(sum_partials(r_part, nparts, smem));
    double bnorm = 0.0;
    if (it == 0 && baseline == 0) bnorm = sqrt(sum_partials(b_part, nparts, smem));
    if (threadIdx.x != 0) return;
    if (it == 0) {
        st->orig_tau = baseline == 0 ? bnorm : (baseline == 1 ? tau : 1.0);
        st->inner_iters = 0;
        st->inner_capped = 0;
        st->stop_iter = -1;
        st->status = 0;
    } else {
        st->inner_iters += inner->stop_iter;
        if (!(inner->status & GKOMI_STATUS_CONVERGED)) st->inner_capped += 1;
    }
    st->tau = tau;
    uint8_t s = 0;
    if (it >= max_iters) {
        s = id_iteration | GKOMI_STATUS_FINALIZED;
    } else if (tau < goal * st->orig_tau) {
        s = GKOMI_STATUS_CONVERGED | id_residual | GKOMI_STATUS_FINALIZED;
    }
    if (s) {
        st->status = s;
        st->stop_iter = it;
    }
}

// x += relaxation * (double) d
__global__ __launch_bounds__(fblock) void ir_promote_axpy_kernel(int64_t n, double* __restrict__ x, const float* __restrict__ d,
                                                                 double relaxation)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(fblock) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * fblock) {
        x[i] = x[i] + relaxation * static_cast<double>(d[i]);
    }
}

struct ir_layout {
    size_t r, rf, df, inner, state, part_r, part_b, small, total;
};

ir_layout make_ir_layout(int64_t n)
{
    ir_layout l{};
    const size_t n1 = static_cast<size_t>(n > 0 ? n : 1);
    const size_t parts = align256(sizeof(double) * max_parts);
    size_t off = 0;
    l.r = off; off += align256(sizeof(double) * n1);
    l.rf = off; off += align256(sizeof(float) * n1);
    l.df = off; off += align256(sizeof(float) * n1);
    l.inner = off; off += make_cgf_layout(n).total;
    l.state = off; off += 256;
    l.part_r = off; off += parts;
    l.part_b = off; off += parts;
    l.small = off; off += 256;  // the double scalars 1 and -1 of r = b - A x
    l.total = off;
    return l;
}

}  // namespace
}  // namespace gkomi

using namespace gkomi;

extern "C" int gkomi_dense_convert_f64_to_f32(gkomi_stream_t s, int64_t nrows, int64_t ncols, const double* in, int64_t in_stride,
                                              float* out, int64_t out_stride)
{
    return convert(s, nrows, ncols, in, in_stride, out, out_stride);
}

extern "C" int gkomi_dense_convert_f32_to_f64(gkomi_stream_t s, int64_t nrows, int64_t ncols, const float* in, int64_t in_stride,
                                              double* out, int64_t out_stride)
{
    return convert(s, nrows, ncols, in, in_stride, out, out_stride);
}

extern "C" size_t gkomi_cg_fused_workspace_bytes_f32(int64_t n)
{
    if (n < 0) return 0;
    return make_cgf_layout(n).total;
}

extern "C" int gkomi_cg_solve_fused_f32_i32(gkomi_stream_t s, int64_t n, int64_t nnz, const int32_t* row_ptrs,
                                            const int32_t* col_idxs, const float* vals, const float* b, float* x,
                                            int64_t max_iters, double reduction, int baseline, void* workspace,
                                            size_t workspace_bytes, double* host_info)
{
    GKOMI_TRY(cgf_check_args(n, nnz, max_iters, baseline, b, x));
    if (workspace == nullptr || workspace_bytes < gkomi_cg_fused_workspace_bytes_f32(n)) return GKOMI_EWORKSPACE;
    cg_scalars* scal = nullptr;
    GKOMI_TRY(cgf_run(s, n, nnz, row_ptrs, col_idxs, vals, b, x, max_iters, reduction, baseline, static_cast<char*>(workspace),
                      &scal));
    cg_scalars h{};
    hipStream_t stream = to_stream(s);
    GKOMI_TRY(read_scalars(stream, &h, scal));
    fill_host_info(host_info, h.stop_iter, h.status, h.tau, h.orig_tau);
    return GKOMI_SUCCESS;
}

extern "C" size_t gkomi_ir_mixed_workspace_bytes(int64_t n)
{
    if (n < 0) return 0;
    return make_ir_layout(n).total;
}

extern "C" int gkomi_ir_mixed_solve_f64_i32(gkomi_stream_t s, int64_t n, int64_t nrhs, int64_t nnz, const int32_t* row_ptrs,
                                            const int32_t* col_idxs, const double* vals, const float* vals_f32,
                                            int spmv_strategy, int64_t max_row_nnz_hint, const double* b, double* x,
                                            int64_t max_iters, double reduction, int baseline, int64_t inner_max_iters,
                                            double inner_reduction, int inner_baseline, double relaxation_factor,
                                            void* workspace, size_t workspace_bytes, double* host_info)
{
    if (n < 0 || nrhs < 0 || nnz < 0 || max_iters < 0 || inner_max_iters < 0) return GKOMI_EINVAL;
    if (baseline < 0 || baseline > 2 || inner_baseline < 0 || inner_baseline > 2) return GKOMI_EINVAL;
    if (nrhs != 1) return GKOMI_ENOTSUPPORTED;
    if (n > INT32_MAX - 1024 || nnz > INT32_MAX) return GKOMI_ENOTSUPPORTED;
    const ir_layout l = make_ir_layout(n);
    if (workspace == nullptr || workspace_bytes < l.total) return GKOMI_EWORKSPACE;
    hipStream_t stream = to_stream(s);
    char* ws = static_cast<char*>(workspace);
    double* r = reinterpret_cast<double*>(ws + l.r);
    float* rf = reinterpret_cast<float*>(ws + l.rf);
    float* df = reinterpret_cast<float*>(ws + l.df);
    ir_state* st = reinterpret_cast<ir_state*>(ws + l.state);
    double* part_r = reinterpret_cast<double*>(ws + l.part_r);
    double* part_b = reinterpret_cast<double*>(ws + l.part_b);
    double* one = reinterpret_cast<double*>(ws + l.small);
    double* neg_one = one + 1;
    sysmat A = make_csr_sysmat(n, nnz, row_ptrs, col_idxs, vals, spmv_strategy, max_row_nnz_hint);
    A.note_working_set(static_cast<int64_t>(sizeof(double)) * n * 3 + static_cast<int64_t>(sizeof(float)) * (8 * nnz + 11 * n));
    const int g = f32_vec_grid(n);
    GKOMI_TRY(gkomi_dense_fill_f64(s, 1, 1, one, 1, 1.0));
    GKOMI_TRY(gkomi_dense_fill_f64(s, 1, 1, neg_one, 1, -1.0));
    auto residual = [&]() -> int {  // r = b - A x
        GKOMI_TRY(gkomi_dense_copy_f64(s, n, 1, b, 1, r, 1));
        return A.apply(s, 1, neg_one, x, one, r);
    };
    GKOMI_TRY(residual());
    if (baseline == 0) hipLaunchKernelGGL(ir_sq_partials_kernel, dim3(g), dim3(fblock), 0, stream, n, b, part_b);
    const cg_scalars* inner = nullptr;
    ir_state h{};
    for (long long it = 0;; ++it) {
        hipLaunchKernelGGL(ir_demote_kernel, dim3(g), dim3(fblock), 0, stream, n, r, rf, df, part_r);
        hipLaunchKernelGGL(ir_check_kernel, dim3(1), dim3(fblock), 0, stream, st, part_r, part_b, g, it,
                           static_cast<long long>(max_iters), reduction, baseline, inner);
        GKOMI_TRY(check_launch());
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(&h, st, sizeof(ir_state), hipMemcpyDeviceToHost, stream)));
        GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
        if (h.status & GKOMI_STATUS_ID_MASK) break;
        // the inner Cg<float> on (float) r, with (float) r as its initial guess (ir.cpp:259-266)
        cg_scalars* scal = nullptr;
        GKOMI_TRY(cgf_run(s, n, nnz, row_ptrs, col_idxs, vals_f32, rf, df, inner_max_iters, inner_reduction, inner_baseline,
                          ws + l.inner, &scal));
        inner = scal;
        hipLaunchKernelGGL(ir_promote_axpy_kernel, dim3(grid_for(n, fblock, max_parts)), dim3(fblock), 0, stream, n, x, df,
                           relaxation_factor);
        GKOMI_TRY(check_launch());
        GKOMI_TRY(residual());
    }
    fill_host_info(host_info, h.stop_iter, h.status, h.tau, h.orig_tau);
    if (host_info != nullptr) {
        host_info[4] = static_cast<double>(h.inner_iters);
        host_info[5] = static_cast<double>(h.inner_capped);
    }
    return GKOMI_SUCCESS;
}
