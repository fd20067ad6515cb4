// Kernels of the fused CG drivers (one GPU: cg_solver.hip; row-partitioned:
// dist_cg.hip).  Included into each of them inside its own anonymous
// namespace: K1 = criterion + p update, K3 = x, r update + r.r partials, the
// two-output dot partials, the device-resident scalars.  See cg_solver.hip for
// the iteration they form.
#pragma once
#include "fused_krylov.hpp"

namespace gkomi {
namespace {

// device-resident solver scalars (the reference's 1x1 Dense workspace scalars)
struct cg_scalars : fused_scalars {
    double beta;
};

// K1.  rho_part/tau_part may alias (Identity preconditioner: z == r).
__global__ __launch_bounds__(fblock) void cg_fused_step1_kernel(
    int64_t n, double* __restrict__ p, const double* __restrict__ z,
    const double* __restrict__ rho_part, int n_rho,
    const double* __restrict__ tau_part, int n_tau, cg_scalars* scal,
    long long it, long long max_iters, double goal, host_watch_line* watch = nullptr)
{
    __shared__ double smem[fblock / wave_size];
    if (fused_stopped_before(status_has_stopped(scal->status), scal, watch, it)) return;
    const pair_sweep sw(n);
    const double* const in[] = {z, p};
    double* const out[] = {p};
    const auto first = sw.prefetch(in);
    const double rho = sum_partials(rho_part, n_rho, smem);
    const double tau2 = rho_part == tau_part ? rho : sum_partials(tau_part, n_tau, smem);
    if (fused_criterion(scal, watch, it, max_iters, rho, sqrt(tau2), goal, id_iteration, id_residual)) return;
    const double prev = scal->rho[(it + 1) & 1];
    const bool restart = prev == 0.0;
    const double tmp = restart ? 0.0 : rho / prev;
    // cg::step_1 (a restart reads p for nothing)
    sw.run(first, in, out, true, [&](int, const double* v, double* o) { o[0] = restart ? v[0] : v[0] + tmp * v[1]; });
}

// K3.  Leaves partial[blockIdx.x] = sum of r_new^2 over this workgroup's share.
__global__ __launch_bounds__(fblock) void cg_fused_step2_kernel(
    int64_t n, double* __restrict__ x, double* __restrict__ r,
    const double* __restrict__ p, const double* __restrict__ q,
    const double* __restrict__ beta_part, int n_beta, cg_scalars* scal,
    long long it, double* __restrict__ rr_part)
{
    __shared__ double smem[fblock / wave_size];
    if (status_has_stopped(scal->status)) return;
    const pair_sweep sw(n);
    const double* const in[] = {x, r, p, q};
    double* const out[] = {x, r};
    const auto first = sw.prefetch(in);
    const double beta = sum_partials(beta_part, n_beta, smem);
    const double rho = scal->rho[it & 1];
    const bool update = beta != 0.0;
    const double tmp = update ? rho / beta : 0.0;
    if (fused_leader()) scal->beta = beta;
    // cg::step_2; r.r of .x and of .y apart, the tail with .x (beta == 0: x and r stay, r.r all the same)
    double acc[2] = {0.0, 0.0};
    sw.run(first, in, out, update, [&](int half, const double* v, double* o) {
        double xv = v[0], rv = v[1];
        if (update) {
            xv += tmp * v[2];
            rv -= tmp * v[3];
        }
        o[0] = xv;
        o[1] = rv;
        acc[half] += rv * rv;
    });
    const double sum[] = {acc[0] + acc[1]};
    double* const part[] = {rr_part};
    store_block_sums(true, sum, part, smem);
}

// partial[blockIdx.x] = sum x*y over the workgroup's share; two outputs so that
// r.z and r.r come from one pass when a preconditioner is present.
// (Not fused_dot2_partials_kernel of krylov.hip: that one reads 8 B per lane into one accumulator per sum, this one
// 16 B into two -- the sums associate differently, and the iterates follow them.)
__global__ __launch_bounds__(fblock) void cg_dot2_partials_kernel(
    int64_t n, const double* __restrict__ r, const double* __restrict__ z,
    const cg_scalars* scal, double* __restrict__ rz_part,
    double* __restrict__ rr_part)
{
    __shared__ double smem[fblock / wave_size];
    if (scal != nullptr && status_has_stopped(scal->status)) return;
    // r and z are workspace vectors (256-B aligned): 16 B per lane
    const pair_sweep sw(n);
    const double* const in[] = {r, z};
    double a[2] = {0.0, 0.0}, bb[2] = {0.0, 0.0};
    auto dots = [&](int half, const double* v) {
        a[half] += v[0] * v[1];
        bb[half] += v[0] * v[0];
    };
    sw.loop(sw.i0, in, dots);
    // the halves are joined before the tail is added
    a[0] += a[1];
    bb[0] += bb[1];
    sw.tail(in, dots);
    const double sum[] = {a[0], bb[0]};
    double* const part[] = {rz_part, rr_part};
    store_block_sums(false, sum, part, smem);
}

__global__ void cg_init_scalars_kernel(cg_scalars* scal, const double* orig_tau,
                                       int baseline_absolute)
{
    init_fused_scalars(scal, 0.0, baseline_absolute ? 1.0 : orig_tau[0]);
    scal->beta = 0.0;
}

int vec_grid(int64_t n) { return fused_vec_grid(n); }  // internal.hpp

}  // namespace
}  // namespace gkomi
