// CB-GMRES for gfx950: GMRES whose Krylov basis is stored as double, float, half or
// scaled 64/32/16-bit integers while the Hessenberg matrix, the Givens data and every
// sum stay in fp64 (core/solver/cb_gmres_kernels.hpp: initialize, restart, arnoldi,
// solve_krylov; semantics = reference/solver/cb_gmres_kernels.cpp:61-452, storage =
// accessor/{reduced_row_major,scaled_reduced_row_major}.hpp) and a native driver for
// CbGmres::apply_dense_impl (core/solver/cb_gmres.cpp:204-491).
//
// Basis entry (k, row, col) sits at (k n + row) nrhs + col; an integer basis has one
// fp64 scalar per (k, col) at k nrhs + col and reads double(stored) * scalar.  Half is
// written double -> float -> half, each round-to-nearest-even, subnormals kept.
//
// The orthogonalisation is the reference's classical Gram-Schmidt with up to two
// re-orthogonalisation passes.  It is a chain of launches; each ends in per-workgroup
// partial sums that EVERY workgroup of the next launch re-adds in the same fixed order
// (the arnoldi_sum_partials pattern of gmres.hip): no workgroup waits for another, no
// atomics, and the condition of the re-orthogonalisation loop is evaluated on the
// device, so the step needs no look from the host.  Products and sums are separate
// operations (-ffp-contract=off), so everything that is not a cross-lane sum equals the
// reference bit for bit given equal inputs.
#include "internal.hpp"
#include "krylov_driver.hpp"

#include <hip/hip_fp16.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <type_traits>
#include <vector>

namespace gkomi {
namespace {

constexpr int cb_block = 512;       // threads per workgroup of the sweeps
constexpr int cb_max_blocks = 512;  // workgroups per column: what every workgroup re-adds per sum
// Basis vectors whose dot products one pass accumulates together.  Per lane of the half
// instantiation: 8 x 2 registers of accumulators, 16 of `next`, 8 x 4 of raw basis data
// in flight, addresses and the decoded values in turn -- under 128 registers, the
// budget of 4 waves per SIMD (two 512-thread workgroups per CU).
constexpr int cb_dot_batch = 8;
// the element-by-element path keeps the same number of loads in flight: 16 per lane
template <class S, bool Vec>
constexpr int batch_of()
{
    return Vec ? cb_dot_batch : cb_dot_batch * 2 * static_cast<int>(sizeof(S)) / 16;
}
constexpr int cb_waves = cb_block / wave_size;
constexpr int64_t cb_max_krylov_dim = 4096;  // h of one step lives in LDS
constexpr int64_t cb_max_nrhs = 65535;        // the columns are the y dimension of the sweeps' grids

template <class S>
struct storage_traits {
    static constexpr bool scaled = std::is_integral<S>::value;
    static constexpr int per_lane = 16 / static_cast<int>(sizeof(S));  // elements of one 16-byte load
};

// write_scalar's correction (cb_gmres_accessor.hpp:165-179)
template <class S>
__host__ __device__ constexpr double scalar_correction()
{
    return storage_traits<S>::scaled ? 2 / static_cast<double>(std::numeric_limits<S>::max()) : 1.0;
}

template <class S>
__device__ __forceinline__ double decode(S stored, double scalar)
{
    if constexpr (storage_traits<S>::scaled) {
        return static_cast<double>(stored) * scalar;
    } else if constexpr (std::is_same<S, _Float16>::value) {
        return static_cast<double>(static_cast<float>(stored));
    } else {
        return static_cast<double>(stored);
    }
}

template <class S>
__device__ __forceinline__ S encode(double v, double scalar)
{
    if constexpr (storage_traits<S>::scaled) {
        return static_cast<S>(v / scalar);  // truncates toward zero
    } else if constexpr (std::is_same<S, _Float16>::value) {
        return static_cast<_Float16>(static_cast<float>(v));
    } else {
        return static_cast<S>(v);
    }
}

// E consecutive rows of one column: 16 bytes of storage per lane
template <class S>
struct alignas(16) chunk {
    S s[storage_traits<S>::per_lane];
};

// Vec: nrhs == 1 and every vector starts on a 16-byte boundary (then n is a multiple of
// E and there is no tail).  Otherwise element by element with the bound checked; rows
// past n read as 0.
template <class S, bool Vec>
__device__ __forceinline__ chunk<S> load_chunk(const S* __restrict__ vec, int64_t row0, int64_t n, int64_t nrhs,
                                               int64_t col)
{
    constexpr int E = storage_traits<S>::per_lane;
    chunk<S> c;
    if constexpr (Vec) {
        c = *reinterpret_cast<const chunk<S>*>(vec + row0);
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) c.s[e] = row0 + e < n ? vec[(row0 + e) * nrhs + col] : S{};
    }
    return c;
}

template <class S, bool Vec>
__device__ __forceinline__ void store_chunk(S* __restrict__ vec, int64_t row0, int64_t n, int64_t nrhs, int64_t col,
                                            const chunk<S>& c)
{
    constexpr int E = storage_traits<S>::per_lane;
    if constexpr (Vec) {
        *reinterpret_cast<chunk<S>*>(vec + row0) = c;
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (row0 + e < n) vec[(row0 + e) * nrhs + col] = c.s[e];
        }
    }
}

template <int E, bool Vec>
__device__ __forceinline__ void load_values(const double* __restrict__ v, int64_t row0, int64_t n, int64_t nrhs,
                                            int64_t col, double (&out)[E])
{
    if constexpr (Vec) {
#pragma unroll
        for (int e = 0; e < E; e += 2) {
            const double2 p = *reinterpret_cast<const double2*>(v + row0 + e);
            out[e] = p.x;
            out[e + 1] = p.y;
        }
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) out[e] = row0 + e < n ? v[(row0 + e) * nrhs + col] : 0.0;
    }
}

template <int E, bool Vec>
__device__ __forceinline__ void store_values(double* __restrict__ v, int64_t row0, int64_t n, int64_t nrhs,
                                             int64_t col, const double (&in)[E])
{
    if constexpr (Vec) {
#pragma unroll
        for (int e = 0; e < E; e += 2) *reinterpret_cast<double2*>(v + row0 + e) = make_double2(in[e], in[e + 1]);
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (row0 + e < n) v[(row0 + e) * nrhs + col] = in[e];
        }
    }
}

__device__ __forceinline__ double wave_reduce_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

// The sum (or maximum) of `count` partials, added in one fixed order by the whole
// workgroup; every thread of every workgroup gets the same bits.  smem: cb_waves doubles.
template <bool Max>
__device__ double cb_combine_partials(const double* __restrict__ partials, int count, double* smem)
{
    double acc = 0.0;
    for (int i = threadIdx.x; i < count; i += cb_block) acc = Max ? fmax(acc, partials[i]) : acc + partials[i];
    acc = Max ? wave_reduce_max(acc) : wave_reduce_sum(acc);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = acc;
    __syncthreads();
    double total = 0.0;
#pragma unroll
    for (int w = 0; w < cb_waves; ++w) total = Max ? fmax(total, smem[w]) : total + smem[w];
    return total;
}

// what the launches of one step hand to each other, per column
struct cb_state {
    double norm0[3];  // eta * norm before the update of pass r (arnoldi_norm row 0)
    int active[3];    // pass r runs (pass 0: the column has not stopped)
    int pad_;
};

// partial sums: [column][slot][workgroup].  The dots use slots 0..iter and iter + 1
// (sum of next^2); every update pass r has its own pair (sum of squares, maximum).
struct cb_partials {
    double* dots;
    double* upd;
    int64_t slots;  // krylov_dim + 2
    __device__ __host__ double* dot(int64_t col, int64_t slot) const { return dots + (col * slots + slot) * cb_max_blocks; }
    __device__ __host__ double* update(int64_t col, int pass, int which) const
    {
        return upd + ((col * 3 + pass) * 2 + which) * cb_max_blocks;
    }
};

// 1. dots: partials of next . basis(k) for k = 0..iter (pass > 0: the same for the
// re-orthogonalisation) and, in pass 0, of next . next.  A stopped column only gets the
// latter (cb_gmres_kernels.cpp:79-87).  Pass r > 0 first decides, in every workgroup
// alike, whether it runs: norm after pass r-1 < eta * norm before it (:122-124).
template <class S, bool Vec>
__global__ __launch_bounds__(cb_block) void cb_dots_kernel(
    int64_t n, int64_t nrhs, const double* __restrict__ next, const S* __restrict__ basis,
    const double* __restrict__ scalars, int iter, const uint8_t* __restrict__ stop_status, cb_state* state, int pass,
    cb_partials part, double eta)
{
    constexpr int E = storage_traits<S>::per_lane;
    constexpr int B = batch_of<S, Vec>();
    __shared__ double smem[cb_dot_batch * cb_waves];
    const int64_t col = blockIdx.y;
    const bool stopped = status_has_stopped(stop_status[col]);
    const int count = gridDim.x;
    if (pass > 0) {
        if (stopped || !state[col].active[pass - 1]) {
            if (blockIdx.x == 0 && threadIdx.x == 0) state[col].active[pass] = 0;
            return;
        }
        const double norm1 = sqrt(cb_combine_partials<false>(part.update(col, pass - 1, 0), count, smem));
        const bool active = norm1 < state[col].norm0[pass - 1];
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            state[col].active[pass] = active;
            state[col].norm0[pass] = eta * norm1;
        }
        if (!active) return;
        __syncthreads();
    }
    const int nvec = stopped ? 0 : iter + 1;
    const int64_t chunks = (n + E - 1) / E;
    const int64_t step = static_cast<int64_t>(gridDim.x) * cb_block;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k0 = 0; k0 < (nvec > 0 ? nvec : 1); k0 += B) {
        const int nb = nvec - k0 < B ? nvec - k0 : B;
        const bool with_norm = pass == 0 && k0 == 0;
        double acc[B];
        double sc[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            acc[b] = 0.0;
            sc[b] = storage_traits<S>::scaled && b < nb ? scalars[(k0 + b) * nrhs + col] : 1.0;
        }
        double nn = 0.0;
        for (int64_t c = blockIdx.x * static_cast<int64_t>(cb_block) + threadIdx.x; c < chunks; c += step) {
            const int64_t row0 = c * E;
            double v[E];
            load_values<E, Vec>(next, row0, n, nrhs, col, v);
            chunk<S> raw[B];
#pragma unroll
            for (int b = 0; b < B; ++b) {
                if (b < nb) raw[b] = load_chunk<S, Vec>(basis + (k0 + b) * n * nrhs, row0, n, nrhs, col);
            }
            if (with_norm) {
#pragma unroll
                for (int e = 0; e < E; ++e) nn += v[e] * v[e];
            }
#pragma unroll
            for (int b = 0; b < B; ++b) {
                if (b < nb) {
#pragma unroll
                    for (int e = 0; e < E; ++e) acc[b] += v[e] * decode<S>(raw[b].s[e], sc[b]);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const double w = wave_reduce_sum(acc[b]);
            if (lane == 0) smem[b * cb_waves + wave] = w;
        }
        __syncthreads();
        if (static_cast<int>(threadIdx.x) < nb) {
            double total = 0.0;
#pragma unroll
            for (int w = 0; w < cb_waves; ++w) total += smem[threadIdx.x * cb_waves + w];
            part.dot(col, k0 + threadIdx.x)[blockIdx.x] = total;
        }
        if (with_norm) {
            __syncthreads();
            const double w = wave_reduce_sum(nn);
            if (lane == 0) smem[wave] = w;
            __syncthreads();
            if (threadIdx.x == 0) {
                double total = 0.0;
#pragma unroll
                for (int w2 = 0; w2 < cb_waves; ++w2) total += smem[w2];
                part.dot(col, iter + 1)[blockIdx.x] = total;
            }
        }
    }
}

// 2. update: every workgroup finishes h (pass 0: hessenberg_iter, else buffer_iter, and
// hessenberg_iter += buffer_iter) from the partials, then next(j) -= h[k] * basis(k, j)
// for k ascending, per element as the reference does (:98-103, :137-144); partials of
// the sum of squares and of max |next| for whatever comes next.
template <class S, bool Vec>
__global__ __launch_bounds__(cb_block) void cb_update_kernel(
    int64_t n, int64_t nrhs, double* __restrict__ next, const S* __restrict__ basis,
    const double* __restrict__ scalars, int iter, const uint8_t* __restrict__ stop_status, cb_state* state, int pass,
    cb_partials part, double* __restrict__ hess_iter, int64_t h_stride, double* __restrict__ buffer_iter,
    double* __restrict__ arnoldi_norm, double eta)
{
    constexpr int E = storage_traits<S>::per_lane;
    constexpr int B = batch_of<S, Vec>();
    extern __shared__ double h[];  // iter + 1 values
    const int64_t col = blockIdx.y;
    const bool stopped = status_has_stopped(stop_status[col]);
    const int count = gridDim.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ double smem[cb_waves];
    if (pass == 0) {
        if (blockIdx.x == 0) {
            const double nn = cb_combine_partials<false>(part.dot(col, iter + 1), count, smem);
            if (threadIdx.x == 0) {
                const double norm0 = eta * sqrt(nn);
                arnoldi_norm[col] = norm0;
                state[col].norm0[0] = norm0;
                state[col].active[0] = !stopped;
            }
        }
        if (stopped) return;
    } else if (stopped || !state[col].active[pass]) {
        return;
    }
    for (int k = wave; k <= iter; k += cb_waves) {
        const double* p = part.dot(col, k);
        double acc = 0.0;
        for (int i = lane; i < count; i += 64) acc += p[i];
        acc = wave_reduce_sum(acc);
        if (lane == 0) h[k] = acc;
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        for (int k = threadIdx.x; k <= iter; k += cb_block) {
            if (pass == 0) {
                hess_iter[k * h_stride + col] = h[k];
            } else {
                buffer_iter[k * nrhs + col] = h[k];
                hess_iter[k * h_stride + col] += h[k];
            }
        }
        if (pass > 0 && threadIdx.x == 0) arnoldi_norm[col] = state[col].norm0[pass];
    }
    const int64_t chunks = (n + E - 1) / E;
    const int64_t step = static_cast<int64_t>(gridDim.x) * cb_block;
    double ss = 0.0, mx = 0.0;
    for (int64_t c = blockIdx.x * static_cast<int64_t>(cb_block) + threadIdx.x; c < chunks; c += step) {
        const int64_t row0 = c * E;
        double v[E];
        load_values<E, Vec>(next, row0, n, nrhs, col, v);
        for (int k0 = 0; k0 <= iter; k0 += B) {
            const int nb = iter + 1 - k0 < B ? iter + 1 - k0 : B;
            chunk<S> raw[B];
#pragma unroll
            for (int b = 0; b < B; ++b) {
                if (b < nb) raw[b] = load_chunk<S, Vec>(basis + (k0 + b) * n * nrhs, row0, n, nrhs, col);
            }
#pragma unroll
            for (int b = 0; b < B; ++b) {
                if (b < nb) {
                    const double hk = h[k0 + b];
                    const double sc = storage_traits<S>::scaled ? scalars[(k0 + b) * nrhs + col] : 1.0;
#pragma unroll
                    for (int e = 0; e < E; ++e) v[e] -= hk * decode<S>(raw[b].s[e], sc);
                }
            }
        }
        store_values<E, Vec>(next, row0, n, nrhs, col, v);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (Vec || row0 + e < n) {
                ss += v[e] * v[e];
                mx = mx >= fabs(v[e]) ? mx : fabs(v[e]);
            }
        }
    }
    ss = wave_reduce_sum(ss);
    mx = wave_reduce_max(mx);
    __shared__ double smax[cb_waves];
    __syncthreads();
    if (lane == 0) {
        smem[wave] = ss;
        smax[wave] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ts = 0.0, tm = 0.0;
#pragma unroll
        for (int w = 0; w < cb_waves; ++w) {
            ts += smem[w];
            tm = fmax(tm, smax[w]);
        }
        part.update(col, pass, 0)[blockIdx.x] = ts;
        part.update(col, pass, 1)[blockIdx.x] = tm;
    }
}

// 4. finalize: norm and max of the last pass that ran; hessenberg(iter + 1) = norm, the
// scalar of vector iter + 1, next /= norm, basis(iter + 1) = compress(next) (:162-170)
template <class S, bool Vec>
__global__ __launch_bounds__(cb_block) void cb_finalize_kernel(
    int64_t n, int64_t nrhs, double* __restrict__ next, S* __restrict__ basis, double* __restrict__ scalars, int iter,
    const uint8_t* __restrict__ stop_status, const cb_state* __restrict__ state, cb_partials part,
    double* __restrict__ hess_iter, int64_t h_stride, double* __restrict__ arnoldi_norm,
    uint64_t* __restrict__ num_reorth)
{
    constexpr int E = storage_traits<S>::per_lane;
    __shared__ double smem[cb_waves];
    const int64_t col = blockIdx.y;
    if (status_has_stopped(stop_status[col])) return;
    const int count = gridDim.x;
    const int last = state[col].active[2] ? 2 : (state[col].active[1] ? 1 : 0);
    const double norm = sqrt(cb_combine_partials<false>(part.update(col, last, 0), count, smem));
    const double mx = cb_combine_partials<true>(part.update(col, last, 1), count, smem);
    const double scalar = storage_traits<S>::scaled ? mx / norm * scalar_correction<S>() : 1.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        arnoldi_norm[nrhs + col] = norm;
        arnoldi_norm[2 * nrhs + col] = mx;
        hess_iter[(iter + 1) * h_stride + col] = norm;
        if (storage_traits<S>::scaled) scalars[(iter + 1) * nrhs + col] = scalar;
        if (num_reorth != nullptr) num_reorth[col] = last;
    }
    const int64_t chunks = (n + E - 1) / E;
    const int64_t step = static_cast<int64_t>(gridDim.x) * cb_block;
    S* out = basis + static_cast<int64_t>(iter + 1) * n * nrhs;
    for (int64_t c = blockIdx.x * static_cast<int64_t>(cb_block) + threadIdx.x; c < chunks; c += step) {
        const int64_t row0 = c * E;
        double v[E];
        load_values<E, Vec>(next, row0, n, nrhs, col, v);
        chunk<S> q;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            v[e] /= norm;
            q.s[e] = encode<S>(v[e], scalar);
        }
        store_values<E, Vec>(next, row0, n, nrhs, col, v);
        store_chunk<S, Vec>(out, row0, n, nrhs, col, q);
    }
}

// restart, first pass: partials of the sum of squares and of max |residual| per column
template <int E, bool Vec>
__global__ __launch_bounds__(cb_block) void cb_restart_norm_kernel(int64_t n, int64_t nrhs,
                                                                   const double* __restrict__ residual,
                                                                   cb_partials part)
{
    __shared__ double smem[cb_waves];
    __shared__ double smax[cb_waves];
    const int64_t col = blockIdx.y;
    const int64_t chunks = (n + E - 1) / E;
    const int64_t step = static_cast<int64_t>(gridDim.x) * cb_block;
    double ss = 0.0, mx = 0.0;
    for (int64_t c = blockIdx.x * static_cast<int64_t>(cb_block) + threadIdx.x; c < chunks; c += step) {
        double v[E];
        load_values<E, Vec>(residual, c * E, n, nrhs, col, v);
#pragma unroll
        for (int e = 0; e < E; ++e) {  // rows past n read as 0: they change neither value
            ss += v[e] * v[e];
            mx = mx >= fabs(v[e]) ? mx : fabs(v[e]);
        }
    }
    ss = wave_reduce_sum(ss);
    mx = wave_reduce_max(mx);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        smem[wave] = ss;
        smax[wave] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ts = 0.0, tm = 0.0;
#pragma unroll
        for (int w = 0; w < cb_waves; ++w) {
            ts += smem[w];
            tm = fmax(tm, smax[w]);
        }
        part.update(col, 0, 0)[blockIdx.x] = ts;
        part.update(col, 0, 1)[blockIdx.x] = tm;
    }
}

// restart, second pass (cb_gmres_kernels.cpp:365-383)
template <class S, bool Vec>
__global__ __launch_bounds__(cb_block) void cb_restart_kernel(
    int64_t n, int64_t nrhs, int64_t krylov_dim, const double* __restrict__ residual,
    double* __restrict__ residual_norm, double* __restrict__ rnc, double* __restrict__ arnoldi_norm,
    S* __restrict__ basis, double* __restrict__ scalars, double* __restrict__ next,
    uint64_t* __restrict__ final_iter_nums, cb_partials part)
{
    constexpr int E = storage_traits<S>::per_lane;
    __shared__ double smem[cb_waves];
    const int64_t col = blockIdx.y;
    const int count = gridDim.x;
    const double norm = sqrt(cb_combine_partials<false>(part.update(col, 0, 0), count, smem));
    const double mx = cb_combine_partials<true>(part.update(col, 0, 1), count, smem);
    const double scalar = storage_traits<S>::scaled ? mx / norm * scalar_correction<S>() : 1.0;
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) {
            residual_norm[col] = norm;
            if (storage_traits<S>::scaled) {
                arnoldi_norm[2 * nrhs + col] = mx;
                scalars[col] = scalar;
            }
            final_iter_nums[col] = 0;
        }
        for (int64_t i = threadIdx.x; i <= krylov_dim; i += cb_block) rnc[i * nrhs + col] = i == 0 ? norm : 0.0;
    }
    const int64_t chunks = (n + E - 1) / E;
    const int64_t step = static_cast<int64_t>(gridDim.x) * cb_block;
    for (int64_t c = blockIdx.x * static_cast<int64_t>(cb_block) + threadIdx.x; c < chunks; c += step) {
        const int64_t row0 = c * E;
        double v[E];
        load_values<E, Vec>(residual, row0, n, nrhs, col, v);
        chunk<S> q;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            v[e] /= norm;
            q.s[e] = encode<S>(v[e], scalar);
        }
        store_values<E, Vec>(next, row0, n, nrhs, col, v);
        store_chunk<S, Vec>(basis, row0, n, nrhs, col, q);
    }
}

// restart, what the reference does to vectors 1..krylov_dim (:386-394): zeros, write_scalar(one)
template <class S>
__global__ __launch_bounds__(256) void cb_restart_clear_kernel(int64_t n, int64_t nrhs, int64_t krylov_dim,
                                                               S* __restrict__ basis, double* __restrict__ scalars)
{
    const int64_t gid = blockIdx.x * static_cast<int64_t>(256) + threadIdx.x;
    const int64_t step = static_cast<int64_t>(gridDim.x) * 256;
    const int64_t first = n * nrhs, total = (krylov_dim + 1) * n * nrhs;
    for (int64_t i = first + gid; i < total; i += step) basis[i] = S{};
    if (storage_traits<S>::scaled) {
        for (int64_t i = nrhs + gid; i < (krylov_dim + 1) * nrhs; i += step) scalars[i] = 1.0 * scalar_correction<S>();
    }
}

// calculate_qy (:282-302): each lane owns its rows and adds the vectors in index order
template <class S, bool Vec>
__global__ __launch_bounds__(cb_block) void cb_qy_kernel(int64_t n, int64_t nrhs, const S* __restrict__ basis,
                                                         const double* __restrict__ scalars,
                                                         const double* __restrict__ y, double* __restrict__ before,
                                                         const uint64_t* __restrict__ final_iter_nums)
{
    constexpr int E = storage_traits<S>::per_lane;
    constexpr int B = batch_of<S, Vec>();
    const int64_t col = blockIdx.y;
    const int m = static_cast<int>(final_iter_nums[col]);
    const int64_t chunks = (n + E - 1) / E;
    const int64_t step = static_cast<int64_t>(gridDim.x) * cb_block;
    for (int64_t c = blockIdx.x * static_cast<int64_t>(cb_block) + threadIdx.x; c < chunks; c += step) {
        const int64_t row0 = c * E;
        double v[E];
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = 0.0;
        for (int k0 = 0; k0 < m; k0 += B) {
            const int nb = m - k0 < B ? m - k0 : B;
            chunk<S> raw[B];
#pragma unroll
            for (int b = 0; b < B; ++b) {
                if (b < nb) raw[b] = load_chunk<S, Vec>(basis + (k0 + b) * n * nrhs, row0, n, nrhs, col);
            }
#pragma unroll
            for (int b = 0; b < B; ++b) {
                if (b < nb) {
                    const double yk = y[(k0 + b) * nrhs + col];
                    const double sc = storage_traits<S>::scaled ? scalars[(k0 + b) * nrhs + col] : 1.0;
#pragma unroll
                    for (int e = 0; e < E; ++e) v[e] += decode<S>(raw[b].s[e], sc) * yk;
                }
            }
        }
        store_values<E, Vec>(before, row0, n, nrhs, col, v);
    }
}

inline size_t storage_size(int storage)
{
    switch (storage) {
    case 0: case 3: return 8;
    case 1: case 4: return 4;
    case 2: case 5: return 2;
    default: return 0;
    }
}

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// f(S{}, std::bool_constant<Vec>{}) for the storage type behind `storage` (the order of
// cb_gmres::storage_precision: keep, reduce1, reduce2, integer, ireduce1, ireduce2)
template <class F>
int dispatch_storage(int storage, bool vec, F&& f)
{
#define GKOMI_CB_CASE(id, type)                                \
    case id:                                                   \
        return vec ? f(type{}, std::true_type{}) : f(type{}, std::false_type{})
    switch (storage) {
        GKOMI_CB_CASE(0, double);
        GKOMI_CB_CASE(1, float);
        GKOMI_CB_CASE(2, _Float16);
        GKOMI_CB_CASE(3, int64_t);
        GKOMI_CB_CASE(4, int32_t);
        GKOMI_CB_CASE(5, int16_t);
    default:
        return GKOMI_EINVAL;
    }
#undef GKOMI_CB_CASE
}

// the 16-byte path: one column, every basis vector and every fp64 vector on a 16-byte boundary
inline bool vector_path(int64_t n, int64_t nrhs, int storage, const void* basis, const void* v0, const void* v1)
{
    return nrhs == 1 && n > 0 && (static_cast<size_t>(n) * storage_size(storage)) % 16 == 0 && aligned16(basis) &&
           aligned16(v0) && aligned16(v1);
}

inline int sweep_blocks(int64_t n, int storage)
{
    const int64_t per = 16 / static_cast<int64_t>(storage_size(storage));
    return static_cast<int>(std::min<int64_t>(cb_max_blocks, std::max<int64_t>(1, ceildiv(ceildiv(n, per), cb_block))));
}

struct step_workspace {
    cb_state* state;
    cb_partials part;
};

inline size_t step_workspace_bytes(int64_t nrhs, int64_t krylov_dim)
{
    return align256(sizeof(cb_state) * static_cast<size_t>(nrhs)) +
           align256(sizeof(double) * static_cast<size_t>(nrhs) * (krylov_dim + 2) * cb_max_blocks) +
           align256(sizeof(double) * static_cast<size_t>(nrhs) * 6 * cb_max_blocks);
}

inline step_workspace carve(void* workspace, int64_t nrhs, int64_t krylov_dim)
{
    char* p = static_cast<char*>(workspace);
    step_workspace w{};
    w.state = reinterpret_cast<cb_state*>(p);
    p += align256(sizeof(cb_state) * static_cast<size_t>(nrhs));
    w.part.dots = reinterpret_cast<double*>(p);
    p += align256(sizeof(double) * static_cast<size_t>(nrhs) * (krylov_dim + 2) * cb_max_blocks);
    w.part.upd = reinterpret_cast<double*>(p);
    w.part.slots = krylov_dim + 2;
    return w;
}

}  // namespace
}  // namespace gkomi

using namespace gkomi;

extern "C" size_t gkomi_cb_gmres_basis_bytes(int64_t n, int64_t nrhs, int64_t krylov_dim, int storage)
{
    if (n < 0 || nrhs < 0 || krylov_dim < 0) return 0;
    return storage_size(storage) * static_cast<size_t>(n) * nrhs * (krylov_dim + 1);
}

extern "C" size_t gkomi_cb_gmres_step_workspace_bytes(int64_t nrhs, int64_t krylov_dim)
{
    if (nrhs <= 0 || krylov_dim <= 0) return 0;
    return step_workspace_bytes(nrhs, krylov_dim);
}

extern "C" int gkomi_cb_gmres_geometry(int storage, int64_t* block_size, int64_t* block_cap,
                                       int64_t* elements_per_lane, int64_t* dot_batch)
{
    if (storage_size(storage) == 0) return GKOMI_EINVAL;
    if (block_size != nullptr) *block_size = cb_block;
    if (block_cap != nullptr) *block_cap = cb_max_blocks;
    if (elements_per_lane != nullptr) *elements_per_lane = 16 / static_cast<int64_t>(storage_size(storage));
    if (dot_batch != nullptr) *dot_batch = cb_dot_batch;
    return GKOMI_SUCCESS;
}

extern "C" int gkomi_cb_gmres_initialize_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, int64_t krylov_dim,
                                             const double* b, int64_t b_stride, double* residual,
                                             int64_t r_stride, double* givens_sin, double* givens_cos,
                                             uint8_t* stop_status)
{
    return gmres_initialize_launch(s, n, nrhs, krylov_dim, b, b_stride, residual, r_stride, givens_sin, givens_cos,
                                   stop_status);
}

extern "C" int gkomi_cb_gmres_restart_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, int64_t krylov_dim,
                                          int storage, const double* residual, double* residual_norm,
                                          double* residual_norm_collection, double* arnoldi_norm,
                                          void* krylov_bases, double* scalars, double* next_krylov_basis,
                                          uint64_t* final_iter_nums, int clear_rest, void* workspace,
                                          size_t workspace_bytes)
{
    if (n < 0 || nrhs < 0 || nrhs > cb_max_nrhs || krylov_dim <= 0 || krylov_dim > cb_max_krylov_dim ||
        storage_size(storage) == 0) {
        return GKOMI_EINVAL;
    }
    if (nrhs == 0) return GKOMI_SUCCESS;
    if (workspace == nullptr || workspace_bytes < step_workspace_bytes(nrhs, krylov_dim)) return GKOMI_EWORKSPACE;
    const step_workspace w = carve(workspace, nrhs, krylov_dim);
    hipStream_t stream = to_stream(s);
    const bool vec = vector_path(n, nrhs, storage, krylov_bases, residual, next_krylov_basis);
    const dim3 grid(sweep_blocks(n, storage), static_cast<unsigned>(nrhs));
    return dispatch_storage(storage, vec, [&](auto tag, auto vtag) {
        using S = decltype(tag);
        constexpr bool Vec = decltype(vtag)::value;
        constexpr int E = storage_traits<S>::per_lane;
        S* basis = static_cast<S*>(krylov_bases);
        hipLaunchKernelGGL((cb_restart_norm_kernel<E, Vec>), grid, dim3(cb_block), 0, stream, n, nrhs, residual,
                           w.part);
        hipLaunchKernelGGL((cb_restart_kernel<S, Vec>), grid, dim3(cb_block), 0, stream, n, nrhs, krylov_dim, residual,
                           residual_norm, residual_norm_collection, arnoldi_norm, basis, scalars, next_krylov_basis,
                           final_iter_nums, w.part);
        if (clear_rest) {
            hipLaunchKernelGGL((cb_restart_clear_kernel<S>), dim3(grid_for(n * nrhs * krylov_dim + nrhs, 256)),
                               dim3(256), 0, stream, n, nrhs, krylov_dim, basis, scalars);
        }
        return check_launch();
    });
}

extern "C" int gkomi_cb_gmres_finish_arnoldi_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, int64_t krylov_dim,
                                                 int storage, double* next_krylov_basis, void* krylov_bases,
                                                 double* scalars, double* hessenberg_iter, int64_t h_stride,
                                                 double* buffer_iter, double* arnoldi_norm, int64_t iter,
                                                 const uint8_t* stop_status, uint64_t* num_reorth,
                                                 void* workspace, size_t workspace_bytes)
{
    if (n < 0 || nrhs < 0 || nrhs > cb_max_nrhs || krylov_dim <= 0 || krylov_dim > cb_max_krylov_dim || iter < 0 ||
        iter >= krylov_dim || storage_size(storage) == 0) {
        return GKOMI_EINVAL;
    }
    if (nrhs == 0) return GKOMI_SUCCESS;
    if (workspace == nullptr || workspace_bytes < step_workspace_bytes(nrhs, krylov_dim)) return GKOMI_EWORKSPACE;
    const step_workspace w = carve(workspace, nrhs, krylov_dim);
    hipStream_t stream = to_stream(s);
    const bool vec = vector_path(n, nrhs, storage, krylov_bases, next_krylov_basis, next_krylov_basis);
    const dim3 grid(sweep_blocks(n, storage), static_cast<unsigned>(nrhs));
    const double eta = 1.0 / std::sqrt(2.0);
    const int it = static_cast<int>(iter);
    const size_t lds = sizeof(double) * static_cast<size_t>(iter + 1);
    return dispatch_storage(storage, vec, [&](auto tag, auto vtag) {
        using S = decltype(tag);
        constexpr bool Vec = decltype(vtag)::value;
        S* basis = static_cast<S*>(krylov_bases);
        for (int pass = 0; pass < 3; ++pass) {
            hipLaunchKernelGGL((cb_dots_kernel<S, Vec>), grid, dim3(cb_block), 0, stream, n, nrhs, next_krylov_basis,
                               basis, scalars, it, stop_status, w.state, pass, w.part, eta);
            hipLaunchKernelGGL((cb_update_kernel<S, Vec>), grid, dim3(cb_block), lds, stream, n, nrhs,
                               next_krylov_basis, basis, scalars, it, stop_status, w.state, pass, w.part,
                               hessenberg_iter, h_stride, buffer_iter, arnoldi_norm, eta);
        }
        hipLaunchKernelGGL((cb_finalize_kernel<S, Vec>), grid, dim3(cb_block), 0, stream, n, nrhs, next_krylov_basis,
                           basis, scalars, it, stop_status, w.state, w.part, hessenberg_iter, h_stride, arnoldi_norm,
                           num_reorth);
        return check_launch();
    });
}

extern "C" int gkomi_cb_gmres_givens_f64(gkomi_stream_t s, int64_t nrhs, double* givens_sin, double* givens_cos,
                                         double* residual_norm, double* residual_norm_collection,
                                         double* hessenberg_iter, int64_t h_stride, int64_t iter,
                                         const uint8_t* stop_status)
{
    return gmres_givens_launch(s, nrhs, givens_sin, givens_cos, residual_norm, residual_norm_collection,
                               hessenberg_iter, h_stride, iter, nullptr, stop_status);
}

extern "C" int gkomi_cb_gmres_arnoldi_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, int64_t krylov_dim,
                                          int storage, double* next_krylov_basis, double* givens_sin,
                                          double* givens_cos, double* residual_norm,
                                          double* residual_norm_collection, void* krylov_bases, double* scalars,
                                          double* hessenberg_iter, int64_t h_stride, double* buffer_iter,
                                          double* arnoldi_norm, int64_t iter, uint64_t* final_iter_nums,
                                          const uint8_t* stop_status, uint64_t* num_reorth, void* workspace,
                                          size_t workspace_bytes)
{
    GKOMI_TRY(gkomi_cb_gmres_finish_arnoldi_f64(s, n, nrhs, krylov_dim, storage, next_krylov_basis, krylov_bases,
                                                scalars, hessenberg_iter, h_stride, buffer_iter, arnoldi_norm, iter,
                                                stop_status, num_reorth, workspace, workspace_bytes));
    return gmres_givens_launch(s, nrhs, givens_sin, givens_cos, residual_norm, residual_norm_collection,
                               hessenberg_iter, h_stride, iter, final_iter_nums, stop_status);
}

extern "C" int gkomi_cb_gmres_solve_krylov_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, int storage,
                                               const double* residual_norm_collection, const void* krylov_bases,
                                               const double* scalars, const double* hessenberg, int64_t h_stride,
                                               double* y, double* before_preconditioner,
                                               const uint64_t* final_iter_nums)
{
    if (n < 0 || nrhs < 0 || nrhs > cb_max_nrhs || storage_size(storage) == 0) return GKOMI_EINVAL;
    if (nrhs == 0) return GKOMI_SUCCESS;
    // every column (the statuses are finalized by now); the restart length is at most the columns of a Hessenberg row
    GKOMI_TRY(gmres_solve_triangular_launch(s, nrhs, h_stride / nrhs, residual_norm_collection, hessenberg, h_stride, y,
                                            final_iter_nums, nullptr));
    if (n == 0) return GKOMI_SUCCESS;
    hipStream_t stream = to_stream(s);
    const bool vec = vector_path(n, nrhs, storage, krylov_bases, before_preconditioner, before_preconditioner);
    const dim3 grid(sweep_blocks(n, storage), static_cast<unsigned>(nrhs));
    return dispatch_storage(storage, vec, [&](auto tag, auto vtag) {
        using S = decltype(tag);
        constexpr bool Vec = decltype(vtag)::value;
        hipLaunchKernelGGL((cb_qy_kernel<S, Vec>), grid, dim3(cb_block), 0, stream, n, nrhs,
                           static_cast<const S*>(krylov_bases), scalars, y, before_preconditioner, final_iter_nums);
        return check_launch();
    });
}

namespace {

struct cb_layout {
    // 5 vectors (residual, next, pv, before, after); tau is the implicit residual norm, of the scalars row 0 is
    // final_iter_nums and rows 1-3 are arnoldi_norm
    solver_layout base;
    size_t basis, scalars, hess, buffer, gsin, gcos, rnc, y, step, total;
};

cb_layout make_cb_layout(int64_t n, int64_t nrhs, int64_t d, int storage)
{
    cb_layout l{};
    l.base = make_solver_layout(n, nrhs, 5);
    size_t off = l.base.total;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += align256(bytes);
        return at;
    };
    const size_t row = sizeof(double) * static_cast<size_t>(nrhs);
    l.basis = take(gkomi_cb_gmres_basis_bytes(n, nrhs, d, storage));
    l.scalars = take(row * (d + 1));
    l.hess = take(row * (d + 1) * d);
    l.buffer = take(row * (d + 1));
    l.gsin = take(row * d);
    l.gcos = take(row * d);
    l.rnc = take(row * (d + 1));
    l.y = take(row * d);
    l.step = take(step_workspace_bytes(nrhs, d));
    l.total = off;
    return l;
}

struct cb_gmres_params {
    int64_t krylov_dim;
    int storage;
};

// CbGmres::apply_dense_impl (core/solver/cb_gmres.cpp:204-487) as the reference's kernel
// sequence.  Of the shared frame the criterion is not used: it is handed the implicit residual norm (c.tau), sets
// finalized, and the host looks at its two flags once per check and at the statuses when one of them is set, which
// is where the reference looks (:336-344) and what the forced iterations hang on.
int cb_gmres_solve_impl(const solve_request& req, const cb_gmres_params& prm)
{
    const gkomi_stream_t s = req.s;
    const int64_t n = req.n, nrhs = req.nrhs, krylov_dim = prm.krylov_dim;
    const int storage = prm.storage;
    if (n < 0 || nrhs <= 0 || nrhs > cb_max_nrhs || krylov_dim <= 0 || krylov_dim > cb_max_krylov_dim ||
        req.max_iters < 0 || req.baseline < 0 || req.baseline > 2 || storage_size(storage) == 0) {
        return GKOMI_EINVAL;
    }
    const cb_layout l = make_cb_layout(n, nrhs, krylov_dim, storage);
    driver_common c;
    GKOMI_TRY(c.init(req, 0, l.base, l.total));
    if (!aligned16(req.workspace)) return GKOMI_EINVAL;
    c.residual_id = 2;
    c.A.note_working_set(static_cast<int64_t>(sizeof(double)) * n * nrhs * 6 +
                         static_cast<int64_t>(gkomi_cb_gmres_basis_bytes(n, nrhs, krylov_dim, storage)));
    hipStream_t stream = c.stream;
    auto D = [&](size_t at) { return reinterpret_cast<double*>(c.ws + at); };
    double *residual = c.vec(0), *next = c.vec(1), *pv = c.vec(2), *before = c.vec(3), *after = c.vec(4);
    void* basis = c.ws + l.basis;
    double *scalars = D(l.scalars), *hess = D(l.hess), *buffer = D(l.buffer), *gsin = D(l.gsin), *gcos = D(l.gcos);
    double *rnc = D(l.rnc), *y = D(l.y);
    double *residual_norm = c.tau, *arnoldi_norm = c.scalars + nrhs;
    uint64_t* final_iter_nums = reinterpret_cast<uint64_t*>(c.scalars);
    uint8_t* stop_status = c.stop_status;
    void* step_ws = c.ws + l.step;
    const size_t step_bytes = step_workspace_bytes(nrhs, krylov_dim);
    const int64_t h_stride = krylov_dim * nrhs;

    auto residual_and_restart = [&]() -> int {
        // residual = b - A x; restart, which takes the norm itself (cb_gmres.cpp:280-287 / 405-414)
        GKOMI_TRY(c.residual(req, residual));
        return gkomi_cb_gmres_restart_f64(s, n, nrhs, krylov_dim, storage, residual, residual_norm, rnc, arnoldi_norm,
                                          basis, scalars, next, final_iter_nums, 0, step_ws, step_bytes);
    };
    auto update_solution = [&]() -> int {
        // x += M^-1 V y (:392-402 / 475-484)
        GKOMI_TRY(gkomi_cb_gmres_solve_krylov_f64(s, n, nrhs, storage, rnc, basis, scalars, hess, h_stride, y, before,
                                                  final_iter_nums));
        GKOMI_TRY(c.apply_precond(before, after));
        return gkomi_dense_add_scaled_f64(s, n, nrhs, c.one, 1, after, nrhs, req.x, nrhs);
    };

    GKOMI_TRY(c.fill_ones());
    GKOMI_TRY(gkomi_dense_fill_f64(s, krylov_dim + 1, h_stride, hess, h_stride, 0.0));
    GKOMI_TRY(gkomi_dense_fill_f64(s, krylov_dim + 1, nrhs, scalars, nrhs, 1.0));
    GKOMI_TRY(gmres_initialize_launch(s, n, nrhs, krylov_dim, req.b, nrhs, residual, nrhs, gsin, gcos, stop_status));
    GKOMI_TRY(residual_and_restart());
    GKOMI_TRY(c.baseline(req, residual, residual_norm));

    long long total_iter = -1;
    int64_t restart_iter = 0;
    std::vector<uint8_t> host_status(nrhs, 0), stop_encountered(nrhs, 0), fully_converged(nrhs, 0);
    // forced iterations after a detected convergence (:315-325)
    constexpr long long start_force_reset = 10;
    constexpr int64_t forced_iteration_fraction = 10;
    const int64_t forced_limit = krylov_dim / forced_iteration_fraction;
    int64_t forced_iterations = forced_limit;
    bool perform_reset = false;
    int64_t forced_resets = 0;
    while (true) {
        ++total_iter;
        if (forced_iterations < forced_limit && forced_iterations < total_iter / forced_iteration_fraction) {
            ++forced_iterations;
        } else {
            // Combined(Iteration, ResidualNorm).check(RelativeStoppingId, true, ...): set_finalized
            uint8_t flags[2] = {0, 0};  // all stopped, one changed
            if (total_iter >= c.max_iters) {
                GKOMI_TRY(gkomi_set_all_statuses(s, nrhs, c.iteration_id, 1, stop_status));
                flags[0] = flags[1] = 1;
            } else {
                GKOMI_TRY(gkomi_residual_norm_f64(s, nrhs, residual_norm, c.orig_tau, c.reduction, c.residual_id, 1,
                                                  stop_status, c.dev_flags, flags));
            }
            if (flags[0] || flags[1]) {
                GKOMI_TRY(static_cast<int>(hipMemcpyAsync(host_status.data(), stop_status, nrhs,
                                                          hipMemcpyDeviceToHost, stream)));
                GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
                bool host_array_changed = false;
                for (int64_t i = 0; i < nrhs; ++i) {
                    if (fully_converged[i]) continue;
                    if (host_status[i] & GKOMI_STATUS_CONVERGED) {
                        if (stop_encountered[i] || total_iter < start_force_reset) {
                            fully_converged[i] = 1;
                        } else {
                            stop_encountered[i] = 1;
                            host_status[i] = 0;
                            host_array_changed = true;
                        }
                    }
                }
                if (host_array_changed) {
                    perform_reset = true;
                    ++forced_resets;
                    GKOMI_TRY(static_cast<int>(hipMemcpyAsync(stop_status, host_status.data(), nrhs,
                                                              hipMemcpyHostToDevice, stream)));
                    GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
                } else {
                    break;
                }
                forced_iterations = 0;
            } else {
                std::fill(stop_encountered.begin(), stop_encountered.end(), 0);
            }
        }
        if (perform_reset || restart_iter == krylov_dim) {
            perform_reset = false;
            GKOMI_TRY(update_solution());
            GKOMI_TRY(residual_and_restart());
            restart_iter = 0;
        }
        GKOMI_TRY(c.apply_precond(next, pv));
        GKOMI_TRY(c.spmv(pv, next));
        GKOMI_TRY(gkomi_cb_gmres_arnoldi_f64(s, n, nrhs, krylov_dim, storage, next, gsin, gcos, residual_norm, rnc,
                                             basis, scalars, hess + nrhs * restart_iter, h_stride, buffer,
                                             arnoldi_norm, restart_iter, final_iter_nums, stop_status, nullptr,
                                             step_ws, step_bytes));
        restart_iter++;
    }
    GKOMI_TRY(update_solution());
    c.converged = 1;
    for (int64_t j = 0; j < nrhs; ++j) c.converged &= (host_status[j] & GKOMI_STATUS_CONVERGED) != 0;
    if (req.host_info != nullptr) req.host_info[2 + 2 * nrhs] = static_cast<double>(forced_resets);
    return c.report(total_iter, req.host_info);
}

}  // namespace

extern "C" size_t gkomi_cb_gmres_workspace_bytes(int64_t n, int64_t nrhs, int64_t krylov_dim, int storage)
{
    if (n < 0 || nrhs <= 0 || krylov_dim <= 0 || storage_size(storage) == 0) return 0;
    return make_cb_layout(n, nrhs, krylov_dim, storage).total;
}

extern "C" int gkomi_cb_gmres_solve_f64_i32(gkomi_stream_t s, int64_t n, int64_t nrhs, int64_t nnz,
                                            const int32_t* row_ptrs, const int32_t* col_idxs, const double* vals,
                                            int spmv_strategy, int64_t max_row_nnz_hint, gkomi_apply_fn precond,
                                            void* precond_ctx, const double* b, double* x, int64_t krylov_dim,
                                            int storage, int64_t max_iters, double reduction_factor, int baseline,
                                            void* workspace, size_t workspace_bytes, double* host_info)
{
    return cb_gmres_solve_impl({s, n, nrhs, make_csr_sysmat(n, nnz, row_ptrs, col_idxs, vals, spmv_strategy, max_row_nnz_hint),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, 1, workspace, workspace_bytes, host_info},
        {krylov_dim, storage});
}

extern "C" int gkomi_cb_gmres_solve_op_f64(gkomi_stream_t s, int64_t n, int64_t nrhs, gkomi_matrix_apply_fn matrix,
                                           void* matrix_ctx, gkomi_apply_fn precond, void* precond_ctx,
                                           const double* b, double* x, int64_t krylov_dim, int storage,
                                           int64_t max_iters, double reduction_factor, int baseline, void* workspace,
                                           size_t workspace_bytes, double* host_info)
{
    if (matrix == nullptr) return GKOMI_EINVAL;
    return cb_gmres_solve_impl({s, n, nrhs, make_op_sysmat(n, matrix, matrix_ctx),
        precond, precond_ctx, b, x, max_iters, reduction_factor, baseline, 1, workspace, workspace_bytes, host_info},
        {krylov_dim, storage});
}
