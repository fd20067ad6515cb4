// Host side of the Krylov drivers (cg_solver.hip: CG; krylov.hip: BiCGSTAB, FCG, CGS, BiCG, IR; idr.hip: IDR(s);
// gmres.hip: GMRES; cb_gmres.hip: CB-GMRES): what a caller asks for, the workspace layout, what every
// reference-sequence driver shares (r = b - A x, the baseline norm, the deferred criterion, the report), and what the
// fused single-rhs drivers share on the host.  Included by the sources that hold a driver; everything is file-local.
// The GMRES family takes the frame without check(): its criterion is handed the implicit residual norm (`tau`).
#pragma once
#include <algorithm>

#include "common.hpp"
#include "fused_krylov.hpp"
#include "internal.hpp"

namespace gkomi {
namespace {

// deferred criterion: the device remembers where every column had stopped; the
// host looks only every few iterations (the step kernels skip stopped columns,
// so the extra iterations launched meanwhile change nothing)
struct stop_record {
    long long iter;
    int phase;
    int pad_;
};

__global__ void record_stop_kernel(const uint8_t* __restrict__ flags, long long iter, int phase,
                                   stop_record* __restrict__ rec)
{
    if (flags[0] != 0 && rec->iter < 0) {
        rec->iter = iter;
        rec->phase = phase;
    }
}

// ---- drivers ------------------------------------------------------------------
// what every solve entry point is asked for; the entry point fills it in once and the drivers hand it on whole
struct solve_request {
    gkomi_stream_t s;
    int64_t n, nrhs;
    sysmat A;
    gkomi_apply_fn precond;
    void* precond_ctx;
    const double* b;
    double* x;
    int64_t max_iters;
    double reduction_factor;
    int baseline;
    int64_t check_every;
    void* workspace;
    size_t workspace_bytes;
    double* host_info;
};

// The fused single-rhs drivers move 16 B per lane through x: a view at an odd offset takes the driver's reference
// sequence instead (*reference), and more rows than the kernels' 32-bit indices reach are refused.
inline int fused_preflight(const solve_request& req, bool* reference)
{
    *reference = reinterpret_cast<uintptr_t>(req.x) % 16 != 0;
    return req.n > INT32_MAX - 1024 ? GKOMI_ENOTSUPPORTED : 0;
}

struct solver_layout {
    size_t vec[8], small, red, parts, total;
};

solver_layout make_solver_layout(int64_t n, int64_t nrhs, int nvec)
{
    solver_layout l{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) / 256 * 256;
        return at;
    };
    for (int k = 0; k < nvec; ++k) l.vec[k] = take(sizeof(double) * static_cast<size_t>(n) * nrhs + 8);
    // 10 scalar rows + statuses + flags
    l.small = take(sizeof(double) * 10 * nrhs + 2 * static_cast<size_t>(nrhs) + 128);
    l.red = take(gkomi_dense_reduction_workspace_bytes(n, nrhs) + 8);
    // fused single-rhs drivers: 3 x <=1024 partials of the vector kernels and
    // 3 x one partial per SpMV row block, plus the device scalars
    l.parts = take(sizeof(double) * (3 * 1024 + 3 * (spmv_dot_partials_room(n))) + 256);
    l.total = off;
    return l;
}

// what the drivers share: the carved workspace, r = b - A x, the baseline norm, the criterion
struct driver_common {
    gkomi_stream_t s;
    hipStream_t stream;
    int64_t n, nrhs;
    sysmat A;
    gkomi_apply_fn precond;
    void* precond_ctx;
    int64_t max_iters;
    double reduction;
    char* ws;
    solver_layout l;
    double *tau, *orig_tau, *one, *neg_one;
    double* scalars;  // 6 rows of nrhs for the solver's own
    uint8_t *stop_status, *dev_flags;
    void* red;
    size_t red_bytes;
    int converged = 0;
    // Combined(Iteration, ResidualNorm): what check() reports; CG numbers them 1 and 2 (fused_krylov.hpp)
    uint8_t iteration_id = 1, residual_id = 1;

    // Checks the request and carves the workspace: `layout` for the shared part, `total` with the solver's own areas
    // behind it.  working_vectors: what the solve moves between two applies of A decides how A is read (internal.hpp);
    // 0 leaves A as the caller set it.
    int init(const solve_request& req, int working_vectors, const solver_layout& layout, size_t total)
    {
        if (req.n < 0 || req.nrhs <= 0) return GKOMI_EINVAL;
        if (req.workspace == nullptr || req.workspace_bytes < total) return GKOMI_EWORKSPACE;
        if (req.max_iters < 0 || req.baseline < 0 || req.baseline > 2) return GKOMI_EINVAL;
        s = req.s;
        stream = to_stream(s);
        n = req.n; nrhs = req.nrhs;
        A = req.A;
        if (working_vectors > 0) A.note_working_set(static_cast<int64_t>(sizeof(double)) * n * nrhs * working_vectors);
        precond = req.precond; precond_ctx = req.precond_ctx;
        max_iters = req.max_iters; reduction = req.reduction_factor;
        ws = static_cast<char*>(req.workspace);
        l = layout;
        double* small = reinterpret_cast<double*>(ws + l.small);
        tau = small;
        orig_tau = small + nrhs;
        one = small + 2 * nrhs;
        neg_one = small + 3 * nrhs;
        scalars = small + 4 * nrhs;
        stop_status = reinterpret_cast<uint8_t*>(small + 10 * nrhs);
        dev_flags = stop_status + nrhs + (8 - nrhs % 8) % 8;
        record = reinterpret_cast<stop_record*>(dev_flags + 16);
        check_every = req.check_every < 1 ? 1 : req.check_every;
        red = ws + l.red;
        red_bytes = gkomi_dense_reduction_workspace_bytes(n, nrhs) + 8;
        const stop_record init{-1, 0, 0};
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(record, &init, sizeof(init), hipMemcpyHostToDevice, stream)));
        return static_cast<int>(hipStreamSynchronize(stream));  // `init` is a stack object
    }
    // a driver with no areas of its own: eight vectors
    int init(const solve_request& req, int working_vectors)
    {
        if (req.n < 0 || req.nrhs <= 0) return GKOMI_EINVAL;
        const solver_layout layout = make_solver_layout(req.n, req.nrhs, 8);
        return init(req, working_vectors, layout, layout.total);
    }
    double* vec(int k) const { return reinterpret_cast<double*>(ws + l.vec[k]); }

    int spmv(const double* in, double* out) const
    {
        return A.apply(s, nrhs, nullptr, in, nullptr, out);
    }
    int apply_precond(const double* in, double* out) const
    {
        if (precond == nullptr) return gkomi_dense_copy_f64(s, n, nrhs, in, nrhs, out, nrhs);
        return precond(precond_ctx, s, in, out);
    }
    int dot(const double* a, const double* b2, double* result) const
    {
        return gkomi_dense_compute_dot_f64(s, n, nrhs, a, nrhs, b2, nrhs, result, red, red_bytes);
    }
    int fill_ones() const
    {
        GKOMI_TRY(gkomi_dense_fill_f64(s, 1, nrhs, one, nrhs, 1.0));
        return gkomi_dense_fill_f64(s, 1, nrhs, neg_one, nrhs, -1.0);
    }
    // r = b - A x
    int residual(const solve_request& req, double* r) const
    {
        GKOMI_TRY(gkomi_dense_copy_f64(s, n, nrhs, req.b, nrhs, r, nrhs));
        return A.apply(s, nrhs, neg_one, req.x, one, r);
    }
    // orig_tau; r_norm: the norm of r where the driver has it already (the GMRES family), else nullptr
    int baseline(const solve_request& req, const double* r, const double* r_norm) const
    {
        if (req.baseline == 0) {
            return gkomi_dense_compute_norm2_f64(s, n, nrhs, req.b, nrhs, orig_tau, red, red_bytes);
        }
        if (req.baseline == 1) {
            if (r_norm != nullptr) return gkomi_dense_copy_f64(s, 1, nrhs, r_norm, nrhs, orig_tau, nrhs);
            return gkomi_dense_compute_norm2_f64(s, n, nrhs, r, nrhs, orig_tau, red, red_bytes);
        }
        return gkomi_dense_fill_f64(s, 1, nrhs, orig_tau, nrhs, 1.0);
    }
    int start(const solve_request& req, double* r)
    {
        GKOMI_TRY(fill_ones());
        // r = b - A x (r already holds b)
        GKOMI_TRY(A.apply(s, nrhs, neg_one, req.x, one, r));
        return baseline(req, r, nullptr);
    }
    stop_record* record = nullptr;  // device
    int64_t check_every = 1;
    int64_t unpolled = 0;
    stop_record host_record{-1, 0, 0};

    int poll()
    {
        unpolled = 0;
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(&host_record, record, sizeof(stop_record),
                                                  hipMemcpyDeviceToHost, stream)));
        return static_cast<int>(hipStreamSynchronize(stream));
    }
    // Combined(Iteration [iteration_id], ResidualNorm [residual_id]) on `residual`; *stop = every
    // column has stopped.  The criterion itself is evaluated on the device at
    // every call, exactly where the reference evaluates it; the host learns the
    // outcome every `check_every` calls (stop_iter() is then the iteration the
    // device recorded, not the current one).
    int check(int64_t iter, const double* residual, bool set_finalized, int phase, bool* stop)
    {
        *stop = false;
        if (iter >= max_iters) {
            GKOMI_TRY(poll());  // converged during the iterations not looked at yet?
            if (host_record.iter < 0) {
                GKOMI_TRY(gkomi_set_all_statuses(s, nrhs, iteration_id, set_finalized ? 1 : 0, stop_status));
                converged = 0;
                host_record.iter = iter;
                host_record.phase = phase;
            } else {
                converged = 1;
            }
            *stop = true;
            return 0;
        }
        GKOMI_TRY(gkomi_dense_compute_norm2_f64(s, n, nrhs, residual, nrhs, tau, red, red_bytes));
        GKOMI_TRY(gkomi_residual_norm_f64(s, nrhs, tau, orig_tau, reduction, residual_id,
                                          set_finalized ? 1 : 0, stop_status, dev_flags, nullptr));
        hipLaunchKernelGGL(record_stop_kernel, dim3(1), dim3(1), 0, stream, dev_flags,
                           static_cast<long long>(iter), phase, record);
        if (++unpolled >= check_every) {
            GKOMI_TRY(poll());
            if (host_record.iter >= 0) {
                converged = 1;
                *stop = true;
            }
        }
        return 0;
    }
    int64_t stop_iter() const { return static_cast<int64_t>(host_record.iter); }
    // host_info = {iterations, converged, (tau, orig_tau) per column}; the wait; the preconditioner's health
    int report(int64_t iter, double* host_info) const
    {
        if (host_info != nullptr) {
            for (int64_t j = 0; j < nrhs; ++j) {
                GKOMI_TRY(static_cast<int>(hipMemcpyAsync(host_info + 2 + 2 * j, tau + j,
                                                          sizeof(double), hipMemcpyDeviceToHost, stream)));
                GKOMI_TRY(static_cast<int>(hipMemcpyAsync(host_info + 3 + 2 * j, orig_tau + j,
                                                          sizeof(double), hipMemcpyDeviceToHost, stream)));
            }
            host_info[0] = static_cast<double>(iter);
            host_info[1] = static_cast<double>(converged);
        }
        GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
        return precond_status(precond, precond_ctx, s);
    }
    int finish(int64_t iter, const double* residual, double* host_info)
    {
        // report the norm of the final residual
        if (host_info != nullptr) GKOMI_TRY(gkomi_dense_compute_norm2_f64(s, n, nrhs, residual, nrhs, tau, red, red_bytes));
        return report(iter, host_info);
    }
};

// what the fused single-rhs drivers share on the host: the device scalars in front of the partial arrays
// (solver_layout::parts), the grid of the vector kernels, how A leaves its dot partials, the pacing and the report
template <class Scalars>
struct fused_driver {
    static_assert(sizeof(Scalars) <= 32 * sizeof(double), "the scalars have 32 doubles in front of the partials");
    const driver_common& c;
    Scalars* scal;
    int g;                // workgroups of the vector kernels = partials they leave, 16 B per lane (internal.hpp)
    spmv_dot_plan spmv;   // the dots in the SpMV's epilogue for CSR / ELL / SELL-P (internal.hpp)
    int nb;               // partials of an apply of A: the epilogue's, or those of the partials kernel after it
    size_t per_spmv;
    host_watch watch;
    explicit fused_driver(const driver_common& c_)
        : c(c_), scal(reinterpret_cast<Scalars*>(c_.ws + c_.l.parts)), g(fused_vec_grid(c_.n)), spmv(c_.A),
          nb(spmv.fused() ? spmv.num_partials : g), per_spmv(spmv_dot_partials_room(c_.n)),
          next(reinterpret_cast<double*>(c_.ws + c_.l.parts) + 32)
    {}
    // the arrays are handed out in order; the layout has room for three of each kind
    double* vec_partials() { return take(fused_vec_max_parts); }
    double* spmv_partials() { return take(per_spmv); }
    // issue(it, last): pace_fused_solve's (internal.hpp); of the last iteration the drivers enqueue only step 1
    template <class Issue>
    int solve(Issue&& issue, double* host_info)
    {
        Scalars h{};
        const long long lag = std::min<long long>(c.check_every, c.precond == nullptr ? 4 * host_watch_lag : host_watch_lag);
        auto look = [&]() -> int {
            const int err = read_scalars(c.stream, &h, scal);
            return err ? -err : h.stop_iter >= 0;
        };
        bool looked = false;
        GKOMI_TRY(pace_fused_solve(c.stream, &watch, c.max_iters, c.check_every, lag, issue, look, &looked));
        return finish_fused(c.s, looked, &h, scal, host_info, c.precond, c.precond_ctx);
    }

private:
    double* next;
    double* take(size_t count)
    {
        double* at = next;
        next += count;
        return at;
    }
};

}  // namespace
}  // namespace gkomi
