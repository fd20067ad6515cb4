// Device side of the fused single-rhs Krylov drivers (CG: cg_fused.hpp; BiCGSTAB, FCG, CGS: krylov.hip), the parts
// every one of their kernels used to spell out:
//   sum_partials        every workgroup re-adds the partial sums of the launch before, all in the same order
//   pair_sweep          16 B per lane over n / 2 pairs: first pair (prefetched) - grid-stride loop - odd tail
//   fused_criterion     the stopping criterion of the first kernel of an iteration, its scalars, the host_watch line
//   store_block_sums    1-3 accumulators -> part[blockIdx.x]
//   fused_scalars       the device-resident scalars every solver's own struct starts with
// A kernel states its arithmetic once, as the `body` of a sweep.  Nothing here decides an order of additions for the
// kernel: which accumulator a half of a pair goes to, and when two accumulators are joined, is the body's and the
// kernel's business (they differ, and the iterates follow them bit for bit).
#pragma once
#include "internal.hpp"

#include <cmath>

namespace gkomi {
namespace {

// 1024-thread workgroups: same thread count on the chip, 4x fewer partials for every consumer workgroup to re-add
// (K3 of CG re-reads the ~3900 p.q partials of K2: 15 MB of L2 traffic instead of 61 MB).  internal.hpp's names,
// which fused_vec_grid depends on; the short ones are what the kernels of cg_fused.hpp's users say.
constexpr int fblock = fused_vec_block;
constexpr int max_parts = fused_vec_max_parts;
constexpr uint8_t id_iteration = 1;  // Combined: ids count from 1 in criteria order
constexpr uint8_t id_residual = 2;

struct fused_scalars {
    double rho[2];        // rho of iteration it lives in rho[it & 1]
    double tau;           // ||r|| at the last evaluated check
    double orig_tau;      // baseline norm
    long long stop_iter;  // iteration index at which the criterion fired, -1 before
    unsigned char status;
    unsigned char pad[7];
    unsigned final_status() const { return status; }  // what host_info's `converged` is read from
};

__device__ __forceinline__ void init_fused_scalars(fused_scalars* scal, double rho0, double orig_tau)
{
    scal->rho[0] = rho0;
    scal->rho[1] = 1.0;  // prev_rho = 1 (the reference's initialize)
    scal->tau = 0.0;
    scal->orig_tau = orig_tau;
    scal->stop_iter = -1;
    scal->status = 0;
}

__device__ __forceinline__ bool fused_leader() { return blockIdx.x == 0 && threadIdx.x == 0; }

__device__ __forceinline__ double sum_partials(const double* __restrict__ part, int nparts, double* smem)
{
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += fblock) acc += part[i];
    acc = wave_reduce_sum(acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) smem[wave] = acc;
    __syncthreads();
    double total = 0.0;
#pragma unroll
    for (int w = 0; w < fblock / wave_size; ++w) total += smem[w];
    return total;  // identical in every thread of every workgroup
}

__device__ __forceinline__ double2 ld2(const double* p, int64_t i)
{
    return reinterpret_cast<const double2*>(p)[i];
}
__device__ __forceinline__ void st2(double* p, int64_t i, double2 v)
{
    reinterpret_cast<double2*>(p)[i] = v;
}

template <int N>
struct pair_values {
    double2 v[N];
};

// The vector kernels move 16 B per lane and issue the loads of their first pair (which do not depend on the scalars)
// before re-adding the partials, so the reduction's latency hides behind them.
//   in[]  : the arrays a kernel reads, out[] : the ones it writes (an array may be in both)
//   body(half, v, o) : one element -- v[k] = in[k][i] -> o[k] = out[k][i].  half = 0 for .x of a pair and for the odd
//                      tail, 1 for .y; it is called for .x, then .y, in the order first pair, loop, tail.
//   store : false = write nothing (a step whose denominator is zero leaves its vectors alone)
struct pair_sweep {
    int64_t n, n2, step, i0;
    __device__ explicit pair_sweep(int64_t n_)
        : n(n_), n2(n_ / 2), step(static_cast<int64_t>(gridDim.x) * fblock),
          i0(blockIdx.x * static_cast<int64_t>(fblock) + threadIdx.x)
    {}

    template <int NI>
    __device__ pair_values<NI> prefetch(const double* const (&in)[NI]) const
    {
        pair_values<NI> f;
#pragma unroll
        for (int k = 0; k < NI; ++k) f.v[k] = i0 < n2 ? ld2(in[k], i0) : make_double2(0.0, 0.0);
        return f;
    }

    // first pair as prefetched, loop, tail
    template <int NI, int NO, class Body>
    __device__ void run(const pair_values<NI>& first, const double* const (&in)[NI], double* const (&out)[NO],
                        bool store, Body&& body) const
    {
        if (i0 < n2) pair(i0, first, out, store, body);
        loop(i0 + step, in, out, store, body);
        tail(in, out, store, body);
    }
    // without a prefetch: the first pair is loaded by the loop
    template <int NI, int NO, class Body>
    __device__ void run(const double* const (&in)[NI], double* const (&out)[NO], bool store, Body&& body) const
    {
        loop(i0, in, out, store, body);
        tail(in, out, store, body);
    }

    template <int NI, int NO, class Body>
    __device__ void loop(int64_t from, const double* const (&in)[NI], double* const (&out)[NO], bool store,
                         Body&& body) const
    {
        for (int64_t i = from; i < n2; i += step) {
            pair_values<NI> f;
#pragma unroll
            for (int k = 0; k < NI; ++k) f.v[k] = ld2(in[k], i);
            pair(i, f, out, store, body);
        }
    }
    // the last element of an odd n: workgroup 0, thread 0
    template <int NI, int NO, class Body>
    __device__ void tail(const double* const (&in)[NI], double* const (&out)[NO], bool store, Body&& body) const
    {
        if (!((n & 1) && fused_leader())) return;
        double v[NI], o[NO];
#pragma unroll
        for (int k = 0; k < NI; ++k) v[k] = in[k][n - 1];
        body(0, v, o);
        if (!store) return;
#pragma unroll
        for (int k = 0; k < NO; ++k) out[k][n - 1] = o[k];
    }
    // read-only sweeps (the dot kernels): body(half, v)
    template <int NI, class Body>
    __device__ void loop(int64_t from, const double* const (&in)[NI], Body&& body) const
    {
        double* const none[1] = {nullptr};
        loop(from, in, none, false, [&](int half, const double* v, double*) { body(half, v); });
    }
    template <int NI, class Body>
    __device__ void tail(const double* const (&in)[NI], Body&& body) const
    {
        double* const none[1] = {nullptr};
        tail(in, none, false, [&](int half, const double* v, double*) { body(half, v); });
    }

private:
    template <int NI, int NO, class Body>
    __device__ void pair(int64_t i, const pair_values<NI>& f, double* const (&out)[NO], bool store, Body&& body) const
    {
        double vx[NI], vy[NI], ox[NO], oy[NO];
#pragma unroll
        for (int k = 0; k < NI; ++k) {
            vx[k] = f.v[k].x;
            vy[k] = f.v[k].y;
        }
        body(0, vx, ox);
        body(1, vy, oy);
        if (!store) return;
#pragma unroll
        for (int k = 0; k < NO; ++k) st2(out[k], i, make_double2(ox[k], oy[k]));
    }
};

// The first kernel of an iteration, before anything else: an earlier launch has stopped the solve -> tell the host
// (internal.hpp: iteration reached, iteration stopped) and return.
__device__ __forceinline__ bool fused_stopped_before(bool stopped, const fused_scalars* scal, host_watch_line* watch,
                                                     long long it)
{
    if (stopped && fused_leader()) host_watch_publish(watch, it, scal->stop_iter);
    return stopped;
}

// ... and once rho and tau = ||r|| are re-added: Combined(Iteration [id_it], ResidualNorm [id_res]), Iteration asked
// first.  Workgroup 0 stores the scalars, then publishes; `also(st)` in between is the solver's own field that goes
// with them.  Returns the status: non-zero = the solve stops here and the kernel returns.
// (Between the two calls sit the kernel's prefetch and its re-adds, which a stopped launch must not pay for.)
template <class Also>
__device__ __forceinline__ uint8_t fused_criterion(fused_scalars* scal, host_watch_line* watch, long long it,
                                                   long long max_iters, double rho, double tau, double goal,
                                                   uint8_t id_it, uint8_t id_res, Also&& also)
{
    uint8_t st = 0;
    if (it >= max_iters) {
        st = id_it | GKOMI_STATUS_FINALIZED;
    } else if (tau < goal * scal->orig_tau) {
        st = GKOMI_STATUS_CONVERGED | id_res | GKOMI_STATUS_FINALIZED;
    }
    if (fused_leader()) {
        scal->rho[it & 1] = rho;
        scal->tau = tau;  // also at the iteration limit: the norm of the residual that is returned
        if (st) {
            scal->stop_iter = it;
            scal->status = st;
        }
        also(st);
        host_watch_publish(watch, it, st ? it : -1ll);
    }
    return st;
}
__device__ __forceinline__ uint8_t fused_criterion(fused_scalars* scal, host_watch_line* watch, long long it,
                                                   long long max_iters, double rho, double tau, double goal,
                                                   uint8_t id_it, uint8_t id_res)
{
    return fused_criterion(scal, watch, it, max_iters, rho, tau, goal, id_it, id_res, [](uint8_t) {});
}

// part[k][blockIdx.x] = the workgroup's sum of acc[k] (a null part[k] is reduced like the others and not stored).
// The barrier between two reductions is there because they share `smem`; `barrier_first` = the one in front of the
// first, for a kernel whose threads have all read `smem` before (sum_partials).
template <int N>
__device__ __forceinline__ void store_block_sums(bool barrier_first, const double (&acc)[N], double* const (&part)[N],
                                                 double* smem)
{
    double total[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (k > 0 || barrier_first) __syncthreads();
        total[k] = block_reduce_sum<fblock>(acc[k], smem);
    }
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (part[k] != nullptr) part[k][blockIdx.x] = total[k];
    }
}

}  // namespace
}  // namespace gkomi
