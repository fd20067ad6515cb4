// Native CG driver for gfx950: Cg::apply_dense_impl (core/solver/cg.cpp:107-193)
// with the criteria Combined(Iteration, ResidualNorm)
// (core/stop/combined.cpp:40, core/stop/residual_norm.cpp:119-228).
//
// mode 0 replays the reference's kernel sequence one launch per kernel on the
// shared driver (krylov_driver.hpp) and looks at the criterion's outcome on the
// host every iteration, as hip/stop/residual_norm_kernels.hip.cpp:119-120 does.
//
// mode 1 is the MI355X design: three launches per iteration, every scalar on
// the device, no per-iteration host round trip.
//   K1 step1 : every workgroup re-adds the <=1024 partials of rho = r.z and
//              tau^2 = r.r left by K3 (same order in every workgroup, so all
//              agree bit for bit), evaluates the criterion, and -- unless
//              stopped -- p = z + (rho/prev_rho) p.
//   K2 spmv  : q = A p (stream kernel) + partials of beta = p.q.
//   K3 step2 : re-adds the beta partials, x += (rho/beta) p, r -= (rho/beta) q,
//              and leaves the partials of r.r for the next K1.
// Once the criterion fires, K1 records the iteration and sets the
// stopping_status; all later launches return immediately, so x, r and the
// iteration count are exactly those of the iteration that stopped.  The host
// polls the status every `check_every` iterations.
// HBM traffic per iteration (n rows, Identity): K1 3n, K2 matrix + 2n (+n
// for p in the epilogue, L2-resident), K3 6n values -- vs 18n + matrix in the
// reference's accounting (core/solver/cg.cpp:148-156).
#include "cg_persistent.hpp"
#include "krylov_driver.hpp"

#include <atomic>
#include <cstdio>
#include <cstdlib>

namespace gkomi {
namespace {

// the shared layout with four vectors (r, z, p, q), then the persistent single-launch solve's areas: its control word
// and two banks of one slot per workgroup
struct cg_layout {
    solver_layout base;
    size_t pcg_ctl, pcg_slots, total;
};

cg_layout make_cg_layout(int64_t n, int64_t nrhs)
{
    cg_layout l{};
    l.base = make_solver_layout(n, nrhs, 4);
    auto align256 = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
    l.pcg_ctl = l.base.total;
    l.pcg_slots = l.pcg_ctl + align256(sizeof(pcg_control));
    l.total = l.pcg_slots + align256(sizeof(pcg_slot) * 2 * (max_parts + pcg_copies) * pcg_max_stride);
    return l;
}

std::atomic<int64_t> pcg_solves{0};  // solves finished by the single-launch kernel (diagnostics, tests)
// GKOMI_CG_PERSISTENT at start-up, gkomi_cg_persistent_enable afterwards
std::atomic<int> pcg_mode{[] {
    const char* e = std::getenv("GKOMI_CG_PERSISTENT");
    return e == nullptr ? 1 : std::atoi(e);
}()};

}  // namespace
}  // namespace gkomi

using namespace gkomi;

extern "C" int64_t gkomi_cg_persistent_solves(void) { return pcg_solves.load(); }
extern "C" int gkomi_cg_persistent_enable(int mode)
{
    if (mode < 0 || mode > 2) return GKOMI_EINVAL;
    pcg_mode.store(mode);
    return GKOMI_SUCCESS;
}

extern "C" size_t gkomi_cg_workspace_bytes(int64_t n, int64_t nrhs)
{
    if (n < 0 || nrhs <= 0) return 0;
    return make_cg_layout(n, nrhs).total;
}

namespace {
// The whole solve in one launch (cg_persistent.hpp) when the vectors AND the matrix fit the
// register files.  Returns 1 when the solve is finished (*result = the final scalars), 0 when the
// path does not apply or gave up (state restored for the three-launch iteration: r = b - A x from
// whatever x the kernel left, p = 0, scalars re-initialised), -(1000 + code) on a HIP / library error.
#define PCG_TRY(expr)                        \
    do {                                     \
        const int err_ = (expr);             \
        if (err_) return -(1000 + err_);     \
    } while (0)
int persistent_cg(const driver_common& c, const solve_request& req, const spmv_dot_plan& spmv, double* r, double* p,
                  double* q, cg_scalars* scal, void* ctl_mem, void* slot_mem, cg_scalars* result)
{
    const gkomi_stream_t s = c.s;
    hipStream_t stream = c.stream;
    const int64_t n = c.n;
    const sysmat& A = c.A;
    double* x = req.x;
    cg_scalars polled{};
    // The whole solve in one launch (cg_persistent.hpp) when the vectors AND the matrix fit the
    // register files: Identity preconditioner, aligned CSR, rows of at most 7 nonzeros (the
    // caller's max_row_nnz_hint says so; the kernel checks), one workgroup per CU.
    // GKOMI_CG_PERSISTENT=0 turns it off, =2 also takes matrices that do not fit (they stream
    // from memory every iteration: 33 vs 34.8 us per iteration on P2, not worth the rendezvous).
    const int persistent_mode = pcg_mode.load();
    static const int cus = device_cu_count();
    const int64_t pcg_chunk = cus > 0 ? ceildiv(n, cus) : 0;
    // an ELL system matrix behind the library's callback: its rows go into the registers just the same
    const gkomi_ell_ctx* ell = !A.is_csr() && A.op == &gkomi_ell_matrix_apply_cb && A.ctx != nullptr
                                   ? static_cast<const gkomi_ell_ctx*>(A.ctx)
                                   : nullptr;
    if (ell != nullptr && (ell->nrows != n || ell->ncols != n || ell->stride < n)) ell = nullptr;
    const int64_t pcg_hint = ell != nullptr ? ell->num_stored_per_row
                                            : spmv.A.hint;  // (a CSR matrix behind its callback carries its own)
    const bool pcg_fits_matrix =
        pcg_hint >= 1 && pcg_hint <= 7 && ceildiv(pcg_chunk, 512) <= 8;
    const bool pcg_fits_vectors = ceildiv(pcg_chunk, pcg_block) <= pcg_max_rows_per_thread;
    if (persistent_mode >= 1 && c.precond == nullptr && (spmv.csr || ell != nullptr) && cus >= 8 &&
        cus <= max_parts &&
        n >= 64 * static_cast<int64_t>(cus) &&
        (pcg_fits_matrix || (persistent_mode >= 2 && pcg_fits_vectors && ell == nullptr)) &&
        persistent_try_acquire()) {  // one persistent solve at a time per process
        struct release_guard {
            ~release_guard() { persistent_release(); }
        } release;
        const sysmat& M = spmv.A;
        const int32_t* m_row_ptrs = ell != nullptr ? nullptr : M.row_ptrs;
        const int32_t* m_col_idxs = ell != nullptr ? ell->col_idxs : M.col_idxs;
        const double* m_vals = ell != nullptr ? ell->vals : M.vals;
        const int ell_stored = ell != nullptr ? static_cast<int>(ell->num_stored_per_row) : 0;
        const int64_t ell_stride = ell != nullptr ? ell->stride : 0;
        pcg_control* ctl = static_cast<pcg_control*>(ctl_mem);
        pcg_slot* slots = static_cast<pcg_slot*>(slot_mem);
        const int chunk = static_cast<int>(ceildiv(n, cus));
        const int rows_per_thread = static_cast<int>(ceildiv(chunk, pcg_block));
        const long long max_polls = [] {
            const char* e = std::getenv("GKOMI_MEET_MAX_POLLS");  // test hook: how long a meeting waits
            return e != nullptr && e[0] != 0 ? std::max(1ll, atoll(e)) : 1ll << 22;
        }();
        static const int stride = [] {
            const char* e = std::getenv("GKOMI_PCG_STRIDE");  // slot spacing in 16-B units (tuning)
            const int v = e != nullptr ? std::atoi(e) : pcg_default_stride;
            return v >= 1 && v <= pcg_max_stride ? v : pcg_default_stride;
        }();
        static const bool resident_on = [] {
            const char* e = std::getenv("GKOMI_PCG_RESIDENT");
            return e == nullptr || e[0] != '0';
        }();
        static const int nap = [] {
            const char* e = std::getenv("GKOMI_PCG_NAP");
            const int v = e != nullptr ? std::atoi(e) : 1;
            return v >= 0 && v <= 64 ? v : 1;
        }();
        hipLaunchKernelGGL(pcg_clear_kernel, dim3(1), dim3(256), 0, stream, slots, stride, 2 * (cus + pcg_copies), ctl);
#define GKOMI_PCG(R, KR, BLOCK)                                                                        \
hipLaunchKernelGGL((cg_persistent_kernel<R, KR, BLOCK, (KR == 7 && R == 8)>), dim3(cus), dim3(BLOCK), 0, stream, \
                   static_cast<int>(n), chunk, m_row_ptrs, m_col_idxs, m_vals, x, r, p, q, slots,  \
                   stride, nap, ctl, scal, static_cast<long long>(c.max_iters), c.reduction,       \
                   max_polls, ell_stored, ell_stride)
        // rows of at most 5 nonzeros, up to 8 rows per thread of a 512-thread workgroup (256
        // registers each): the matrix stays in registers
        const int rows_per_thread_512 = static_cast<int>(ceildiv(chunk, 512));
        const bool resident = pcg_fits_matrix && resident_on;
        if (resident && pcg_hint <= 5) {
            if (rows_per_thread_512 <= 2) {
                GKOMI_PCG(2, 5, 512);
            } else if (rows_per_thread_512 <= 4) {
                GKOMI_PCG(4, 5, 512);
            } else {
                GKOMI_PCG(8, 5, 512);
            }
        } else if (resident) {
            if (rows_per_thread_512 <= 2) {
                GKOMI_PCG(2, 7, 512);
            } else if (rows_per_thread_512 <= 4) {
                GKOMI_PCG(4, 7, 512);
            } else {
                GKOMI_PCG(8, 7, 512);  // x in LDS: 7 nonzeros x 8 rows of values fill the registers
            }
        } else if (rows_per_thread <= 1) {
            GKOMI_PCG(1, 0, 1024);
        } else if (rows_per_thread <= 2) {
            GKOMI_PCG(2, 0, 1024);
        } else if (rows_per_thread <= 4) {
            GKOMI_PCG(4, 0, 1024);
        } else {
            GKOMI_PCG(8, 0, 1024);
        }
#undef GKOMI_PCG
        PCG_TRY(check_launch());
        pcg_control hctl{};
        PCG_TRY(static_cast<int>(hipMemcpyAsync(&hctl, ctl, sizeof(pcg_control), hipMemcpyDeviceToHost, stream)));
        PCG_TRY(static_cast<int>(hipMemcpyAsync(&polled, scal, sizeof(cg_scalars), hipMemcpyDeviceToHost, stream)));
        PCG_TRY(static_cast<int>(hipStreamSynchronize(stream)));
#ifdef GKOMI_PCG_PROFILE
        fprintf(stderr, "pcg phases (us per iteration, workgroup 0): meet rho %.2f | p + barrier %.2f | inv %.2f | "
                        "spmv %.2f | meet pq %.2f | update %.2f over %lld iterations\n",
                hctl.ticks[0] * 0.01 / (polled.stop_iter + 1), hctl.ticks[1] * 0.01 / (polled.stop_iter + 1),
                hctl.ticks[2] * 0.01 / (polled.stop_iter + 1), hctl.ticks[3] * 0.01 / (polled.stop_iter + 1),
                hctl.ticks[4] * 0.01 / (polled.stop_iter + 1), hctl.ticks[5] * 0.01 / (polled.stop_iter + 1),
                polled.stop_iter);
        fprintf(stderr, "pcg meeting (us, mean over %llu meetings): own slot seen %.2f | last slot seen %.2f | total "
                        "published %.2f | workgroup 101 has the total %.2f\n",
                hctl.pad2_[4], hctl.pad2_[0] * 0.01 / hctl.pad2_[4], hctl.pad2_[1] * 0.01 / hctl.pad2_[4],
                hctl.pad2_[2] * 0.01 / hctl.pad2_[4], hctl.pad2_[3] * 0.01 / hctl.pad2_[4]);
#endif
        if (hctl.overrun == 0 && (polled.status & GKOMI_STATUS_ID_MASK)) {
            pcg_solves.fetch_add(1);
            *result = polled;
            return 1;
        } else {
            // a meeting timed out (workgroups not resident together?): x is a valid guess, start over
            // from r = b - A x with the three-launch iteration
            PCG_TRY(gkomi_dense_copy_f64(s, n, 1, req.b, 1, r, 1));
            PCG_TRY(A.apply(s, 1, c.neg_one, x, c.one, r));
            PCG_TRY(gkomi_dense_fill_f64(s, n, 1, p, 1, 0.0));
            hipLaunchKernelGGL(cg_init_scalars_kernel, dim3(1), dim3(1), 0, stream, scal, c.orig_tau,
                               req.baseline == 2 ? 1 : 0);
        }
    }
    return 0;
}
#undef PCG_TRY

int cg_solve_impl(const solve_request& req, int mode)
{
    const gkomi_stream_t s = req.s;
    const int64_t n = req.n, nrhs = req.nrhs;
    if (mode == 1 && n == 0) mode = 0;  // the fused path needs rows
    // the fused kernels move 16 B per lane through x and the workspace vectors: anything else
    // (a view at an odd offset) takes the reference sequence, like the other fused drivers
    bool reference = false;
    const int too_many_rows = fused_preflight(req, &reference);  // (answered below, after the argument checks)
    if (mode == 1 && nrhs == 1 && (reference || reinterpret_cast<uintptr_t>(req.workspace) % 16 != 0)) mode = 0;
    if (n < 0 || nrhs <= 0 || req.max_iters < 0) return GKOMI_EINVAL;
    if (req.baseline < 0 || req.baseline > 2 || (mode != 0 && mode != 1)) return GKOMI_EINVAL;
    if (mode == 1 && nrhs != 1) return GKOMI_ENOTSUPPORTED;
    GKOMI_TRY(too_many_rows);
    const cg_layout l = make_cg_layout(n, nrhs);
    driver_common c;
    GKOMI_TRY(c.init(req, 6, l.base, l.total));
    c.iteration_id = id_iteration;
    c.residual_id = id_residual;
    hipStream_t stream = c.stream;
    const sysmat& A = c.A;
    double *x = req.x, *r = c.vec(0), *z = c.vec(1), *p = c.vec(2), *q = c.vec(3);
    double *prev_rho = c.scalars, *rho = prev_rho + nrhs, *beta = rho + nrhs;
    // cg::initialize, then r = b - A x (advanced apply) and the criterion's baseline norm, cg.cpp:137-142
    GKOMI_TRY(gkomi_cg_initialize_f64(s, n, nrhs, req.b, nrhs, r, nrhs, z, nrhs, p,
                                      nrhs, q, nrhs, prev_rho, rho, c.stop_status));
    GKOMI_TRY(c.start(req, r));

    if (mode == 0) {
        c.check_every = 1;  // the reference asks the host every iteration, whatever the caller's check_every
        int64_t iter = -1;
        while (true) {
            GKOMI_TRY(c.apply_precond(r, z));  // (matrix::Identity::apply copies, core/matrix/identity.cpp)
            GKOMI_TRY(c.dot(r, z, rho));
            ++iter;
            bool stop = false;
            GKOMI_TRY(c.check(iter, r, true, 1, &stop));
            if (stop) break;
            GKOMI_TRY(gkomi_cg_step_1_f64(s, n, nrhs, p, nrhs, z, nrhs, rho, prev_rho, c.stop_status));
            GKOMI_TRY(c.spmv(p, q));
            GKOMI_TRY(c.dot(p, q, beta));
            GKOMI_TRY(gkomi_cg_step_2_f64(s, n, nrhs, x, nrhs, r, nrhs, p, nrhs, q, nrhs, beta, rho,
                                          c.stop_status));
            std::swap(prev_rho, rho);
        }
        return c.finish(c.stop_iter(), r, req.host_info);
    } else {
        // scal, the vector grid g, how A leaves its p.q partials (q = A p with them in the same launch for CSR / ELL /
        // SELL-P; any other operator, or misaligned CSR arrays: its apply, then a partials kernel) and their number nb.
        // Each partial array has room for one partial per workgroup of a block-Jacobi apply that carries the dots.
        fused_driver<cg_scalars> f(c);
        cg_scalars* scal = f.scal;
        double *part_a = f.spmv_partials(), *part_b = f.spmv_partials(), *part_c = f.spmv_partials();  // r.z | r.r | p.q
        const int g = f.g, nb = f.nb;
        const spmv_dot_plan& spmv = f.spmv;
        const gkomi_apply_fn precond = c.precond;
        hipLaunchKernelGGL(cg_init_scalars_kernel, dim3(1), dim3(1), 0, stream, scal, c.orig_tau,
                           req.baseline == 2 ? 1 : 0);
        GKOMI_TRY(check_launch());
        // The whole solve in one launch when vectors and matrix fit the register files (persistent_cg
        // above); otherwise, or when it gave up, the three-launch iteration below.
        {
            cg_scalars polled{};
            const int done = persistent_cg(c, req, spmv, r, p, q, scal, c.ws + l.pcg_ctl, c.ws + l.pcg_slots, &polled);
            if (done < 0) return -done - 1000;
            if (done == 1) {
                fill_host_info(req.host_info, polled.stop_iter, polled.status, polled.tau, polled.orig_tau);
                return precond_status(precond, c.precond_ctx, s);
            }
        }
        // partials of r.z (and r.r) for the first check
        const double* zz = precond == nullptr ? r : z;
        // The library's own block-Jacobi behind the callback: z = M^-1 r leaves the partials of r.z and r.r itself
        // (jacobi_apply_kernel<..., Dot>: every lane holds both factors of its row) -- one launch and a pass over
        // r and z less per iteration (profiles/r03_p3_cg_kernels.md).  `ng` = how many partials K1 re-adds: the
        // apply's workgroups then, the vector grid otherwise.
        const gkomi_jacobi_ctx* jac =
            precond == &gkomi_jacobi_apply_cb ? static_cast<const gkomi_jacobi_ctx*>(c.precond_ctx) : nullptr;
        int ng = g;
        auto precondition = [&](bool first) -> int {  // z = M^-1 r and the partials of r.z (and, first / fused, r.r)
            if (jac != nullptr) {
                const int got = jacobi_apply_dot_launch(s, jac, r, z, part_a, part_b, spmv_dot_partials_room(n),
                                                        &scal->status);
                if (got < 0) return -got - 1000;
                if (got > 0) {
                    ng = got;
                    return 0;
                }
                jac = nullptr;  // not for this one (scalar Jacobi): the general way from here on
            }
            GKOMI_TRY(c.apply_precond(r, z));
            hipLaunchKernelGGL(cg_dot2_partials_kernel, dim3(g), dim3(fblock), 0, stream, n, r, z,
                               first ? static_cast<const cg_scalars*>(nullptr) : static_cast<const cg_scalars*>(scal),
                               part_a, first ? part_b : static_cast<double*>(nullptr));
            return check_launch();
        };
        if (precond != nullptr) {
            GKOMI_TRY(precondition(true));
        } else {
            hipLaunchKernelGGL(cg_dot2_partials_kernel, dim3(g), dim3(fblock), 0, stream, n, r, zz,
                               static_cast<const cg_scalars*>(nullptr), part_a, static_cast<double*>(nullptr));
            GKOMI_TRY(check_launch());
        }
        const double* tau_part = precond == nullptr ? part_a : part_b;
        // launches issued after the criterion fired return at once -- unless a preconditioner's are among them
        host_watch& watch = f.watch;
        auto issue = [&](long long i, bool) -> int {  // (the last iteration is enqueued whole as well)
            // (with the Jacobi apply's partials both sums have ng terms; K3's r.r partials, g of them, otherwise)
            hipLaunchKernelGGL(cg_fused_step1_kernel, dim3(g), dim3(fblock), 0, stream, n, p, zz,
                               part_a, ng, tau_part, jac != nullptr ? ng : g, scal, i,
                               static_cast<long long>(c.max_iters), c.reduction, watch.dev);
            if (spmv.fused()) {
                GKOMI_TRY(spmv.launch(stream, p, q, part_c, &scal->status));
            } else {
                GKOMI_TRY(A.apply(s, 1, nullptr, p, nullptr, q));
                hipLaunchKernelGGL(cg_dot2_partials_kernel, dim3(g), dim3(fblock), 0, stream, n, p, q,
                                   static_cast<const cg_scalars*>(scal), part_c,
                                   static_cast<double*>(nullptr));
            }
            hipLaunchKernelGGL(cg_fused_step2_kernel, dim3(g), dim3(fblock), 0, stream, n, x, r, p,
                               q, part_c, nb, scal, i, precond == nullptr ? part_a : part_b);
            if (precond != nullptr) GKOMI_TRY(precondition(false));
            return check_launch();
        };
        return f.solve(issue, req.host_info);
    }
}
}  // namespace

extern "C" int gkomi_cg_solve_f64_i32(
    gkomi_stream_t s, int64_t n, int64_t nrhs, int64_t nnz,
    const int32_t* row_ptrs, const int32_t* col_idxs, const double* vals,
    int spmv_strategy, int64_t max_row_nnz_hint, gkomi_apply_fn precond,
    void* precond_ctx, const double* b, double* x, int64_t max_iters,
    double reduction_factor, int baseline, int mode, int check_every,
    void* workspace, size_t workspace_bytes, double* host_info)
{
    return cg_solve_impl({s, n, nrhs, make_csr_sysmat(n, nnz, row_ptrs, col_idxs, vals, spmv_strategy, max_row_nnz_hint),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, check_every, workspace, workspace_bytes,
        host_info}, mode);
}

// the system matrix behind a callback, fused (single rhs): three launches per
// iteration for ELL / SELL-P / CSR behind the library's callbacks (SpMV + dot
// epilogue), apply + 3 for any other operator
extern "C" int gkomi_cg_solve_fused_op_f64(gkomi_stream_t s, int64_t n, gkomi_matrix_apply_fn matrix,
                                           void* matrix_ctx, gkomi_apply_fn precond, void* precond_ctx,
                                           const double* b, double* x, int64_t max_iters,
                                           double reduction_factor, int baseline, int64_t check_every,
                                           void* workspace, size_t workspace_bytes, double* host_info)
{
    if (matrix == nullptr) return GKOMI_EINVAL;
    return cg_solve_impl({s, n, 1, make_op_sysmat(n, matrix, matrix_ctx),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, std::min<int64_t>(check_every, 1 << 20),
        workspace, workspace_bytes, host_info}, 1);
}

// the system matrix behind a callback: the reference kernel sequence (mode 0)
extern "C" int gkomi_cg_solve_op_f64(gkomi_stream_t s, int64_t n, int64_t nrhs,
                                     gkomi_matrix_apply_fn matrix, void* matrix_ctx,
                                     gkomi_apply_fn precond, void* precond_ctx, const double* b,
                                     double* x, int64_t max_iters, double reduction_factor,
                                     int baseline, void* workspace, size_t workspace_bytes,
                                     double* host_info)
{
    if (matrix == nullptr) return GKOMI_EINVAL;
    return cg_solve_impl({s, n, nrhs, make_op_sysmat(n, matrix, matrix_ctx),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, 1, workspace, workspace_bytes, host_info}, 0);
}
