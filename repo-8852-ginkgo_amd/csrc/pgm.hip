// multigrid::Pgm for gfx950: gko::kernels::hip::pgm::* (core/multigrid/pgm_kernels.hpp) and the whole of
// Pgm::generate (core/multigrid/pgm.cpp:147-236) as a native driver.  Semantics = reference/multigrid/pgm_kernels.cpp:67-348.
//
// The reference executor walks the rows in order.  On a weight matrix with a symmetric pattern (W = 0.5 |A| + 0.5 |A|^T
// always has one) that order does not matter, except in one step that has a closed form (tests/test_pgm_reference.py
// checks the argument on every case and on seeded random matrices):
//   find_strongest_neighbor  a row changes agg only if no neighbour is unaggregated, so by symmetry no unaggregated row
//                            reads an entry this sweep writes, and the entry a changing row copies was set before it.
//   match_edge               the smaller index of a mutual pair is the only writer of both entries.
//   assign_to_exist_agg      deterministic: reads a snapshot.  Default: row r sees the unaggregated rows below it as
//                            assigned; every one of them does get a value, so r's choice p(r) -- the greatest
//                            (weight, col) among neighbours that are aggregated or unaggregated with col < r -- is
//                            static, and agg[r] = agg[p(r)] once p(r) is final.  Chains r -> p(r) -> ... strictly
//                            decrease; they are resolved by ceil(log2 n) rounds of pointer jumping between two
//                            buffers, the count fixed before the first launch.
// No kernel waits for another workgroup, every loop has a bound known before it starts, and the only atomics are
// integer adds, which are order-free.  Sums of the coarse matrix run left to right over a stably sorted run, every
// add rounded once (-ffp-contract=off): the reference's bits.  <double, int32> only.
#include "internal.hpp"
#include "sort_scan.hpp"

namespace gkomi {
namespace {

constexpr int block = 256;

// std::tie(aw, ac) > std::tie(bw, bc) as std::tuple spells it (pgm_kernels.cpp:217, :222, :276)
__device__ __forceinline__ bool tie_greater(double aw, int32_t ac, double bw, int32_t bc)
{
    return (bw < aw) || (!(aw < bw) && bc < ac);
}

struct best {
    double w;
    int32_t c;
    __device__ __forceinline__ void take(double weight, int32_t col)
    {
        if (tie_greater(weight, col, w, c)) {
            w = weight;
            c = col;
        }
    }
};

// the greatest (w, c) of the Width lanes of a sub-wave, in every lane; (w, c) is a total order on finite weights, so
// the tree's shape does not matter
template <int Width>
__device__ __forceinline__ best subwave_best(best b)
{
#pragma unroll
    for (int off = Width / 2; off > 0; off >>= 1) {
        const double ow = __shfl_xor(b.w, off, 64);
        const int32_t oc = __shfl_xor(b.c, off, 64);
        b.take(ow, oc);
    }
    return b;
}

// gko::max(abs(d_row), abs(d_col)) and the one IEEE division of pgm_kernels.cpp:214-215
__device__ __forceinline__ double edge_weight(double val, double abs_d_row, double d_col)
{
    const double b = fabs(d_col);
    return val / (abs_d_row >= b ? abs_d_row : b);
}

__global__ __launch_bounds__(block) void fill_i32_kernel(int64_t n, int32_t value, int32_t* __restrict__ out)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * block) {
        out[i] = value;
    }
}

__global__ __launch_bounds__(block) void absolute_kernel(int64_t nnz, const double* __restrict__ in,
                                                         double* __restrict__ out)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i < nnz;
         i += static_cast<int64_t>(gridDim.x) * block) {
        out[i] = fabs(in[i]);
    }
}

// One sub-wave per row, lanes stride the row; lane 0 writes.  agg is read and written: see the head of the file for why
// no lane reads an entry another row writes in the same launch.  assigned += rows absorbed.
template <int Width>
__global__ __launch_bounds__(block) void find_strongest_neighbor_kernel(
    int n, const int32_t* __restrict__ row_ptrs, const int32_t* __restrict__ col_idxs, const double* __restrict__ vals,
    const double* __restrict__ diag, int32_t* agg, int32_t* __restrict__ strongest, int32_t* __restrict__ assigned)
{
    const int64_t gid = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x;
    const int lane = threadIdx.x % Width;
    const int64_t row64 = gid / Width;
    const int row = row64 < n ? static_cast<int>(row64) : 0;
    const bool live = row64 < n && agg[row] == -1;
    best unagg{0.0, -1}, aggd{0.0, -1};
    if (live) {
        const double dr = fabs(diag[row]);
        const int32_t end = row_ptrs[row + 1];
        for (int32_t idx = row_ptrs[row] + lane; idx < end; idx += Width) {
            const int32_t col = col_idxs[idx];
            if (col == row) continue;
            const double weight = edge_weight(vals[idx], dr, diag[col]);
            if (agg[col] == -1) {
                unagg.take(weight, col);
            } else {
                aggd.take(weight, col);
            }
        }
    }
    unagg = subwave_best<Width>(unagg);
    aggd = subwave_best<Width>(aggd);
    bool absorbed = false;
    if (live && lane == 0) {
        if (unagg.c == -1 && aggd.c != -1) {
            agg[row] = agg[aggd.c];
            absorbed = true;
        } else if (unagg.c != -1) {
            strongest[row] = unagg.c;
        } else {
            strongest[row] = row;
        }
    }
    const unsigned long long mask = __ballot(absorbed);
    if ((threadIdx.x & 63) == 0 && mask != 0) atomicAdd(assigned, __popcll(mask));
}

// assigned += entries that leave -1
__global__ __launch_bounds__(block) void match_edge_kernel(int n, const int32_t* __restrict__ strongest, int32_t* agg,
                                                           int32_t* __restrict__ assigned)
{
    const int64_t i64 = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x;
    int count = 0;
    if (i64 < n) {
        const int i = static_cast<int>(i64);
        if (agg[i] == -1) {
            const int32_t neighbor = strongest[i];
            if (neighbor >= 0 && neighbor < n && strongest[neighbor] == i && i <= neighbor) {
                count = 1;
                if (neighbor != i) {
                    // only this thread writes agg[neighbor]: a second writer j would need strongest[neighbor] == j
                    if (agg[neighbor] == -1) count = 2;
                    agg[neighbor] = i;
                }
                agg[i] = i;
            }
        }
    }
    if (assigned != nullptr) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off, 64);
        if ((threadIdx.x & 63) == 0 && count != 0) atomicAdd(assigned, count);
    }
}

__global__ __launch_bounds__(block) void count_unagg_kernel(int64_t n, const int32_t* __restrict__ agg,
                                                            int32_t* __restrict__ counter)
{
    int count = 0;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * block) {
        count += agg[i] == -1;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off, 64);
    if ((threadIdx.x & 63) == 0 && count != 0) atomicAdd(counter, count);
}

// The choice of an unaggregated row among its candidates.  Snapshot (deterministic): the aggregated neighbours, and
// out[row] = the value itself -- agg[choice], row without a candidate, agg[row] for an aggregated row.  Otherwise the
// unaggregated neighbours with a smaller index are candidates too, and out[row] = the choice as a link: the neighbour,
// or row itself for a row without a candidate and for an aggregated row.
template <int Width, bool Snapshot>
__global__ __launch_bounds__(block) void assign_choose_kernel(
    int n, const int32_t* __restrict__ row_ptrs, const int32_t* __restrict__ col_idxs, const double* __restrict__ vals,
    const double* __restrict__ diag, const int32_t* __restrict__ agg, int32_t* __restrict__ out)
{
    const int64_t gid = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x;
    const int lane = threadIdx.x % Width;
    const int64_t row64 = gid / Width;
    const int row = row64 < n ? static_cast<int>(row64) : 0;
    const int32_t own = row64 < n ? agg[row] : 0;
    const bool live = row64 < n && own == -1;
    best aggd{0.0, -1};
    if (live) {
        const double dr = fabs(diag[row]);
        const int32_t end = row_ptrs[row + 1];
        for (int32_t idx = row_ptrs[row] + lane; idx < end; idx += Width) {
            const int32_t col = col_idxs[idx];
            if (col == row) continue;
            if (agg[col] != -1 || (!Snapshot && col < row)) {
                aggd.take(edge_weight(vals[idx], dr, diag[col]), col);
            }
        }
    }
    aggd = subwave_best<Width>(aggd);
    if (row64 < n && lane == 0) {
        if (Snapshot) {
            out[row] = !live ? own : (aggd.c != -1 ? agg[aggd.c] : row);
        } else {
            out[row] = live && aggd.c != -1 ? aggd.c : row;
        }
    }
}

__global__ __launch_bounds__(block) void pointer_jump_kernel(int64_t n, const int32_t* __restrict__ next,
                                                             int32_t* __restrict__ out)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * block) {
        out[i] = next[next[i]];
    }
}

// root[i]: where the chain of row i ends -- an aggregated row (its value) or a row without a candidate (itself)
__global__ __launch_bounds__(block) void assign_resolve_kernel(int64_t n, const int32_t* __restrict__ root,
                                                               const int32_t* __restrict__ agg, int32_t* __restrict__ out)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * block) {
        const int32_t r = root[i];
        const int32_t a = agg[r];
        out[i] = a != -1 ? a : r;
    }
}

__global__ __launch_bounds__(block) void renumber_flag_kernel(int64_t n, const int32_t* __restrict__ agg,
                                                              int32_t* __restrict__ map)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * block) {
        const int32_t a = agg[i];
        if (a >= 0 && a <= n) map[a] = 1;  // every writer of an entry stores the same value
    }
}

__global__ __launch_bounds__(block) void renumber_gather_kernel(int64_t n, const int32_t* __restrict__ map,
                                                                int32_t* __restrict__ agg)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * block) {
        const int32_t a = agg[i];
        if (a >= 0 && a <= n) agg[i] = map[a];
    }
}

__global__ __launch_bounds__(block) void map_row_kernel(int n, const int32_t* __restrict__ row_ptrs,
                                                        const int32_t* __restrict__ agg, int32_t* __restrict__ row_idxs)
{
    // a quarter wave per row
    const int64_t gid = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x;
    const int64_t row = gid / 16;
    if (row >= n) return;
    const int32_t coarse = agg[row];
    const int32_t end = row_ptrs[row + 1];
    for (int32_t idx = row_ptrs[row] + static_cast<int>(gid % 16); idx < end; idx += 16) row_idxs[idx] = coarse;
}

__global__ __launch_bounds__(block) void map_col_kernel(int64_t nnz, const int32_t* __restrict__ col_idxs,
                                                        const int32_t* __restrict__ agg, int32_t* __restrict__ out)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i < nnz;
         i += static_cast<int64_t>(gridDim.x) * block) {
        out[i] = agg[col_idxs[i]];
    }
}

// keys[i] = rows[i] << shift | cols[i], payload[i] = i
__global__ __launch_bounds__(block) void pack_keys_kernel(int64_t num, const int32_t* __restrict__ rows,
                                                          const int32_t* __restrict__ cols, int shift,
                                                          uint64_t* __restrict__ keys, uint32_t* __restrict__ payload)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i < num;
         i += static_cast<int64_t>(gridDim.x) * block) {
        keys[i] = (static_cast<uint64_t>(static_cast<uint32_t>(rows[i])) << shift) | static_cast<uint32_t>(cols[i]);
        if (payload != nullptr) payload[i] = static_cast<uint32_t>(i);
    }
}

// map_row and map_col in one: keys[idx] = agg[row] << shift | agg[col], payload[idx] = idx
__global__ __launch_bounds__(block) void coarse_keys_kernel(int n, const int32_t* __restrict__ row_ptrs,
                                                            const int32_t* __restrict__ col_idxs,
                                                            const int32_t* __restrict__ agg, int shift,
                                                            uint64_t* __restrict__ keys, uint32_t* __restrict__ payload)
{
    const int64_t gid = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x;
    const int64_t row = gid / 16;
    if (row >= n) return;
    const uint64_t high = static_cast<uint64_t>(static_cast<uint32_t>(agg[row])) << shift;
    const int32_t end = row_ptrs[row + 1];
    for (int32_t idx = row_ptrs[row] + static_cast<int>(gid % 16); idx < end; idx += 16) {
        keys[idx] = high | static_cast<uint32_t>(agg[col_idxs[idx]]);
        payload[idx] = static_cast<uint32_t>(idx);
    }
}

__global__ __launch_bounds__(block) void unpack_keys_kernel(int64_t num, const uint64_t* __restrict__ keys, int shift,
                                                            int32_t* __restrict__ rows, int32_t* __restrict__ cols)
{
    const uint64_t mask = (uint64_t{1} << shift) - 1;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i < num;
         i += static_cast<int64_t>(gridDim.x) * block) {
        rows[i] = static_cast<int32_t>(keys[i] >> shift);
        cols[i] = static_cast<int32_t>(keys[i] & mask);
    }
}

__global__ __launch_bounds__(block) void gather_f64_kernel(int64_t num, const uint32_t* __restrict__ from,
                                                           const double* __restrict__ in, double* __restrict__ out)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i < num;
         i += static_cast<int64_t>(gridDim.x) * block) {
        out[i] = in[from[i]];
    }
}

// heads[i] = 1 where a run of equal keys starts, heads[num] = 0: its exclusive sum numbers the runs and ends in
// their count
__global__ __launch_bounds__(block) void key_heads_kernel(int64_t num, const uint64_t* __restrict__ keys,
                                                          int32_t* __restrict__ heads)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i <= num;
         i += static_cast<int64_t>(gridDim.x) * block) {
        heads[i] = i < num && (i == 0 || keys[i] != keys[i - 1]);
    }
}

__global__ __launch_bounds__(block) void pair_heads_kernel(int64_t num, const int32_t* __restrict__ rows,
                                                           const int32_t* __restrict__ cols, int32_t* __restrict__ heads)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i <= num;
         i += static_cast<int64_t>(gridDim.x) * block) {
        heads[i] = i < num && (i == 0 || rows[i] != rows[i - 1] || cols[i] != cols[i - 1]);
    }
}

// One thread per run of equal (row, col): temp = vals[first]; temp += vals[next] ... left to right
// (pgm_kernels.cpp:322-344).  Keyed: the run is a run of equal keys and its values sit at payload[]; otherwise a run
// of equal (rows, cols) with its values in place.
template <bool Keyed>
__global__ __launch_bounds__(block) void coarse_sum_kernel(
    int64_t num, const uint64_t* __restrict__ keys, int shift, const uint32_t* __restrict__ payload,
    const int32_t* __restrict__ rows, const int32_t* __restrict__ cols, const double* __restrict__ vals,
    const int32_t* __restrict__ run_of, int32_t* __restrict__ c_rows, int32_t* __restrict__ c_cols,
    double* __restrict__ c_vals)
{
    const uint64_t mask = (uint64_t{1} << shift) - 1;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i < num;
         i += static_cast<int64_t>(gridDim.x) * block) {
        if (run_of[i + 1] == run_of[i]) continue;  // not the head of a run
        double temp;
        int32_t r, c;
        if (Keyed) {
            const uint64_t key = keys[i];
            temp = vals[payload[i]];
            for (int64_t j = i + 1; j < num && keys[j] == key; ++j) temp += vals[payload[j]];
            r = static_cast<int32_t>(key >> shift);
            c = static_cast<int32_t>(key & mask);
        } else {
            r = rows[i];
            c = cols[i];
            temp = vals[i];
            for (int64_t j = i + 1; j < num && rows[j] == r && cols[j] == c; ++j) temp += vals[j];
        }
        const int32_t e = run_of[i];
        c_rows[e] = r;
        c_cols[e] = c;
        c_vals[e] = temp;
    }
}

bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    if (a == nullptr || b == nullptr || a_bytes == 0 || b_bytes == 0) return false;
    const char* pa = static_cast<const char*>(a);
    const char* pb = static_cast<const char*>(b);
    return pa < pb + b_bytes && pb < pa + a_bytes;
}

int bit_width(int64_t v)
{
    int b = 0;
    while (v > 0) {
        ++b;
        v >>= 1;
    }
    return b;
}

// bits that hold every index below `count`, at least one
int index_bits(int64_t count) { return count > 1 ? bit_width(count - 1) : 1; }

// the sub-wave of a row by the mean row length, as the sub-wave SpMV picks it
int subwave_width(int64_t n, int64_t nnz)
{
    const int64_t mean = n > 0 ? nnz / n : 0;
    return mean <= 4 ? 4 : (mean <= 8 ? 8 : (mean <= 16 ? 16 : 64));
}

unsigned row_grid(int64_t n, int width) { return static_cast<unsigned>(ceildiv(n * width, block)); }

int fill_i32(hipStream_t stream, int64_t n, int32_t value, int32_t* out)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(fill_i32_kernel, dim3(grid_for(n, block)), dim3(block), 0, stream, n, value, out);
    return check_launch();
}

int find_strongest_neighbor_launch(hipStream_t stream, int64_t n, int64_t nnz, const int32_t* rp, const int32_t* ci,
                                   const double* v, const double* diag, int32_t* agg, int32_t* strongest,
                                   int32_t* assigned)
{
    const int rows = static_cast<int>(n);
    const int width = subwave_width(n, nnz);
#define GKOMI_PGM_FIND(W)                                                                                             \
    hipLaunchKernelGGL(find_strongest_neighbor_kernel<W>, dim3(row_grid(n, W)), dim3(block), 0, stream, rows, rp, ci, \
                       v, diag, agg, strongest, assigned)
    if (width == 4) {
        GKOMI_PGM_FIND(4);
    } else if (width == 8) {
        GKOMI_PGM_FIND(8);
    } else if (width == 16) {
        GKOMI_PGM_FIND(16);
    } else {
        GKOMI_PGM_FIND(64);
    }
#undef GKOMI_PGM_FIND
    return check_launch();
}

template <bool Snapshot>
int assign_choose_launch(hipStream_t stream, int64_t n, int64_t nnz, const int32_t* rp, const int32_t* ci,
                         const double* v, const double* diag, const int32_t* agg, int32_t* out)
{
    const int rows = static_cast<int>(n);
    const int width = subwave_width(n, nnz);
#define GKOMI_PGM_CHOOSE(W)                                                                                           \
    hipLaunchKernelGGL((assign_choose_kernel<W, Snapshot>), dim3(row_grid(n, W)), dim3(block), 0, stream, rows, rp, \
                       ci, v, diag, agg, out)
    if (width == 4) {
        GKOMI_PGM_CHOOSE(4);
    } else if (width == 8) {
        GKOMI_PGM_CHOOSE(8);
    } else if (width == 16) {
        GKOMI_PGM_CHOOSE(16);
    } else {
        GKOMI_PGM_CHOOSE(64);
    }
#undef GKOMI_PGM_CHOOSE
    return check_launch();
}

// rounds of pointer jumping that resolve any strictly decreasing chain among n rows: 2^rounds >= n
int jump_rounds(int64_t n) { return n > 1 ? bit_width(n - 1) : 0; }

// scratch: three arrays of n int32 (default mode), one (deterministic with intermediate == nullptr)
int assign_to_exist_agg_launch(hipStream_t stream, int64_t n, int64_t nnz, const int32_t* rp, const int32_t* ci,
                               const double* v, const double* diag, int32_t* agg, int32_t* intermediate,
                               bool deterministic, int32_t* scratch)
{
    const size_t bytes = sizeof(int32_t) * static_cast<size_t>(n);
    if (deterministic) {
        int32_t* out = intermediate != nullptr ? intermediate : scratch;
        GKOMI_TRY(assign_choose_launch<true>(stream, n, nnz, rp, ci, v, diag, agg, out));
        return static_cast<int>(hipMemcpyAsync(agg, out, bytes, hipMemcpyDeviceToDevice, stream));
    }
    int32_t* next = scratch;
    int32_t* other = scratch + n;
    int32_t* resolved = scratch + 2 * n;
    GKOMI_TRY(assign_choose_launch<false>(stream, n, nnz, rp, ci, v, diag, agg, next));
    const int rounds = jump_rounds(n);
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(pointer_jump_kernel, dim3(grid_for(n, block)), dim3(block), 0, stream, n, next, other);
        int32_t* t = next;
        next = other;
        other = t;
    }
    hipLaunchKernelGGL(assign_resolve_kernel, dim3(grid_for(n, block)), dim3(block), 0, stream, n, next, agg, resolved);
    GKOMI_TRY(check_launch());
    return static_cast<int>(hipMemcpyAsync(agg, resolved, bytes, hipMemcpyDeviceToDevice, stream));
}

size_t renumber_bytes(int64_t n) { return align256(sizeof(int32_t) * static_cast<size_t>(n + 1)) + scan_workspace_bytes(n + 1); }

// map = n + 1 int32, then the scan's scratch; *num_agg_dev = &map[n] once the stream has run
int renumber_launch(hipStream_t stream, int64_t n, int32_t* agg, void* ws, const int32_t** num_agg_dev)
{
    int32_t* map = static_cast<int32_t*>(ws);
    void* scan_ws = static_cast<char*>(ws) + align256(sizeof(int32_t) * static_cast<size_t>(n + 1));
    GKOMI_TRY(static_cast<int>(hipMemsetAsync(map, 0, sizeof(int32_t) * static_cast<size_t>(n + 1), stream)));
    hipLaunchKernelGGL(renumber_flag_kernel, dim3(grid_for(n, block)), dim3(block), 0, stream, n, agg, map);
    GKOMI_TRY(exclusive_sum_i32(stream, map, map, n + 1, scan_ws, scan_workspace_bytes(n + 1)));
    hipLaunchKernelGGL(renumber_gather_kernel, dim3(grid_for(n, block)), dim3(block), 0, stream, n, map, agg);
    *num_agg_dev = map + n;
    return check_launch();
}

int read_i32(hipStream_t stream, const int32_t* dev, int32_t* host)
{
    GKOMI_TRY(static_cast<int>(hipMemcpyAsync(host, dev, sizeof(int32_t), hipMemcpyDeviceToHost, stream)));
    return static_cast<int>(hipStreamSynchronize(stream));
}

// the pieces of a workspace, in order, each on a 256-byte boundary.  A null base only measures: every piece is null and
// `used` is the size
struct carver {
    char* base;
    size_t used = 0;
    explicit carver(void* base_) : base(static_cast<char*>(base_)) {}
    template <class T>
    T* take(size_t count)
    {
        T* p = base != nullptr ? reinterpret_cast<T*>(base + used) : nullptr;
        used += align256(sizeof(T) * count);
        return p;
    }
};

// stable sort of (rows, cols[, position]) by (row, col) over all 64 key bits: keys, keys_out [, payload, payload_out]
size_t pair_sort_bytes(int64_t num, bool pairs)
{
    const size_t m = static_cast<size_t>(num > 0 ? num : 1);
    return 2 * align256(8 * m) + (pairs ? 2 * align256(4 * m) : 0) + radix_sort_workspace_bytes(num, 8, pairs);
}

struct generate_ws {
    double* absv;
    int32_t* trp;
    int32_t* tci;
    double* tv;
    int32_t* wrp;
    int32_t* wci;
    double* wv;
    double* diag;
    int32_t* strongest;
    int32_t* scratch;  // 3 n
    int32_t* counters;
    double* half;
    uint64_t* keys;
    uint64_t* keys_out;
    uint32_t* payload;
    uint32_t* payload_out;
    int32_t* run_of;
    int32_t* c_rows;
    int32_t* c_cols;
    double* c_vals;
    void* sub;
    size_t sub_bytes;
    size_t total;
};

generate_ws carve_generate(void* base, int64_t n, int64_t nnz)
{
    generate_ws w;
    carver c(base);
    const size_t rows = static_cast<size_t>(n), nz = static_cast<size_t>(nnz > 0 ? nnz : 1);
    const size_t most = rows > nz ? rows : nz;
    w.absv = c.take<double>(nz);
    w.trp = c.take<int32_t>(rows + 1);
    w.tci = c.take<int32_t>(nz);
    w.tv = c.take<double>(nz);
    w.wrp = c.take<int32_t>(rows + 1);
    w.wci = c.take<int32_t>(2 * nz);  // the union of two patterns of nnz entries
    w.wv = c.take<double>(2 * nz);
    w.diag = c.take<double>(rows);
    w.strongest = c.take<int32_t>(rows);
    w.scratch = c.take<int32_t>(3 * rows);
    w.counters = c.take<int32_t>(64);
    w.half = c.take<double>(1);
    w.keys = c.take<uint64_t>(most);
    w.keys_out = c.take<uint64_t>(most);
    w.payload = c.take<uint32_t>(most);
    w.payload_out = c.take<uint32_t>(most);
    w.run_of = c.take<int32_t>(nz + 1);
    w.c_rows = c.take<int32_t>(nz);
    w.c_cols = c.take<int32_t>(nz);
    w.c_vals = c.take<double>(nz);
    size_t sub = gkomi_csr_transpose_workspace_bytes(n);
    auto grow = [&sub](size_t b) {
        if (b > sub) sub = b;
    };
    grow(gkomi_csr_spgeam_workspace_bytes(n));
    grow(gkomi_prefix_sum_workspace_bytes(n + 2));
    grow(renumber_bytes(n));
    grow(radix_sort_workspace_bytes(static_cast<int64_t>(most), 8, true));
    grow(scan_workspace_bytes(nnz + 1));
    w.sub_bytes = align256(sub);
    w.sub = c.take<char>(w.sub_bytes);
    w.total = c.used;
    return w;
}

}  // namespace
}  // namespace gkomi

using namespace gkomi;

namespace {

bool too_large(int64_t n, int64_t nnz) { return n >= INT32_MAX || nnz >= INT32_MAX; }

bool bad_weight_csr(int64_t n, int64_t nnz, const int32_t* rp, const int32_t* ci, const double* v, const double* diag)
{
    if (rp == nullptr || diag == nullptr) return true;
    return nnz > 0 && (ci == nullptr || v == nullptr);
}

// an output (or scratch) range that overlaps one of the arrays of a weight matrix or its diagonal
bool weight_csr_overlaps(int64_t n, int64_t nnz, const int32_t* rp, const int32_t* ci, const double* v, const double* diag,
                         const void* out, size_t out_bytes)
{
    return overlaps(rp, 4 * static_cast<size_t>(n + 1), out, out_bytes) || overlaps(ci, 4 * static_cast<size_t>(nnz), out, out_bytes) ||
           overlaps(v, 8 * static_cast<size_t>(nnz), out, out_bytes) || overlaps(diag, 8 * static_cast<size_t>(n), out, out_bytes);
}

}  // namespace

extern "C" int gkomi_csr_compute_absolute_f64_i32(gkomi_stream_t s, int64_t nnz, const double* vals, double* abs_vals)
{
    if (nnz < 0) return GKOMI_EINVAL;
    if (nnz == 0) return GKOMI_SUCCESS;
    if (vals == nullptr || abs_vals == nullptr) return GKOMI_EINVAL;
    const size_t bytes = sizeof(double) * static_cast<size_t>(nnz);
    if (overlaps(vals, bytes, abs_vals, bytes)) return GKOMI_EINVAL;
    hipLaunchKernelGGL(absolute_kernel, dim3(grid_for(nnz, block)), dim3(block), 0, to_stream(s), nnz, vals, abs_vals);
    return check_launch();
}

extern "C" int gkomi_pgm_match_edge_i32(gkomi_stream_t s, int64_t n, const int32_t* strongest_neighbor, int32_t* agg)
{
    if (n < 0) return GKOMI_EINVAL;
    if (n == 0) return GKOMI_SUCCESS;
    if (strongest_neighbor == nullptr || agg == nullptr) return GKOMI_EINVAL;
    if (n >= INT32_MAX) return GKOMI_ENOTSUPPORTED;
    const size_t bytes = sizeof(int32_t) * static_cast<size_t>(n);
    if (overlaps(strongest_neighbor, bytes, agg, bytes)) return GKOMI_EINVAL;
    hipLaunchKernelGGL(match_edge_kernel, dim3(static_cast<unsigned>(ceildiv(n, block))), dim3(block), 0, to_stream(s),
                       static_cast<int>(n), strongest_neighbor, agg, static_cast<int32_t*>(nullptr));
    return check_launch();
}

extern "C" int gkomi_pgm_count_unagg_i32(gkomi_stream_t s, int64_t n, const int32_t* agg, int64_t* host_num_unagg,
                                         void* workspace, size_t workspace_bytes)
{
    if (n < 0 || host_num_unagg == nullptr) return GKOMI_EINVAL;
    if (n == 0) {
        *host_num_unagg = 0;
        return GKOMI_SUCCESS;
    }
    if (agg == nullptr) return GKOMI_EINVAL;
    if (workspace == nullptr || workspace_bytes < sizeof(int32_t)) return GKOMI_EINVAL;
    if (overlaps(agg, sizeof(int32_t) * static_cast<size_t>(n), workspace, workspace_bytes)) return GKOMI_EINVAL;
    hipStream_t stream = to_stream(s);
    int32_t* counter = static_cast<int32_t*>(workspace);
    GKOMI_TRY(static_cast<int>(hipMemsetAsync(counter, 0, sizeof(int32_t), stream)));
    hipLaunchKernelGGL(count_unagg_kernel, dim3(grid_for(n, block)), dim3(block), 0, stream, n, agg, counter);
    GKOMI_TRY(check_launch());
    int32_t host = 0;
    GKOMI_TRY(read_i32(stream, counter, &host));
    *host_num_unagg = host;
    return GKOMI_SUCCESS;
}

extern "C" size_t gkomi_pgm_renumber_workspace_bytes(int64_t n) { return n > 0 ? renumber_bytes(n) : 0; }

extern "C" int gkomi_pgm_renumber_i32(gkomi_stream_t s, int64_t n, int32_t* agg, int64_t* host_num_agg,
                                      void* workspace, size_t workspace_bytes)
{
    if (n < 0 || host_num_agg == nullptr) return GKOMI_EINVAL;
    if (n == 0) {
        *host_num_agg = 0;
        return GKOMI_SUCCESS;
    }
    if (agg == nullptr) return GKOMI_EINVAL;
    if (n >= INT32_MAX) return GKOMI_ENOTSUPPORTED;
    if (workspace == nullptr || workspace_bytes < renumber_bytes(n)) return GKOMI_EINVAL;
    if (overlaps(agg, sizeof(int32_t) * static_cast<size_t>(n), workspace, workspace_bytes)) return GKOMI_EINVAL;
    hipStream_t stream = to_stream(s);
    const int32_t* num_agg_dev = nullptr;
    GKOMI_TRY(renumber_launch(stream, n, agg, workspace, &num_agg_dev));
    int32_t host = 0;
    GKOMI_TRY(read_i32(stream, num_agg_dev, &host));
    *host_num_agg = host;
    return GKOMI_SUCCESS;
}

extern "C" size_t gkomi_pgm_sort_workspace_bytes(int64_t num)
{
    // keys twice, positions twice, a copy of the values, the sort's own scratch
    if (num <= 0) return 0;
    return pair_sort_bytes(num, true) + align256(sizeof(double) * static_cast<size_t>(num));
}

extern "C" int gkomi_pgm_sort_agg_i32(gkomi_stream_t s, int64_t num, int32_t* row_idxs, int32_t* col_idxs,
                                      void* workspace, size_t workspace_bytes)
{
    if (num < 0) return GKOMI_EINVAL;
    if (num == 0) return GKOMI_SUCCESS;
    if (row_idxs == nullptr || col_idxs == nullptr) return GKOMI_EINVAL;
    if (num >= INT32_MAX) return GKOMI_ENOTSUPPORTED;
    const size_t bytes = sizeof(int32_t) * static_cast<size_t>(num);
    if (overlaps(row_idxs, bytes, col_idxs, bytes)) return GKOMI_EINVAL;
    if (workspace == nullptr || workspace_bytes < gkomi_pgm_sort_workspace_bytes(num)) return GKOMI_EINVAL;
    if (overlaps(row_idxs, bytes, workspace, workspace_bytes) || overlaps(col_idxs, bytes, workspace, workspace_bytes))
        return GKOMI_EINVAL;
    hipStream_t stream = to_stream(s);
    carver c(workspace);
    uint64_t* keys = c.take<uint64_t>(num);
    uint64_t* keys_out = c.take<uint64_t>(num);
    void* sort_ws = c.take<char>(radix_sort_workspace_bytes(num, 8, false));
    const int grid = grid_for(num, block);
    hipLaunchKernelGGL(pack_keys_kernel, dim3(grid), dim3(block), 0, stream, num, row_idxs, col_idxs, 32, keys,
                       static_cast<uint32_t*>(nullptr));
    GKOMI_TRY(radix_sort_u64(stream, num, keys, keys_out, nullptr, nullptr, 64, sort_ws,
                             radix_sort_workspace_bytes(num, 8, false)));
    hipLaunchKernelGGL(unpack_keys_kernel, dim3(grid), dim3(block), 0, stream, num, keys_out, 32, row_idxs, col_idxs);
    return check_launch();
}

extern "C" int gkomi_pgm_map_row_i32(gkomi_stream_t s, int64_t num_fine_row, const int32_t* fine_row_ptrs,
                                     const int32_t* agg, int32_t* row_idxs)
{
    if (num_fine_row < 0) return GKOMI_EINVAL;
    if (num_fine_row == 0) return GKOMI_SUCCESS;
    if (fine_row_ptrs == nullptr || agg == nullptr) return GKOMI_EINVAL;
    if (num_fine_row >= INT32_MAX) return GKOMI_ENOTSUPPORTED;
    if (row_idxs == nullptr) return GKOMI_EINVAL;
    // the length of row_idxs is fine_row_ptrs[num_fine_row], which the host does not know: only an output that starts
    // inside an input can be told
    {
        const char* out = reinterpret_cast<const char*>(row_idxs);
        const char* a0 = reinterpret_cast<const char*>(agg);
        const char* r0 = reinterpret_cast<const char*>(fine_row_ptrs);
        if ((out >= a0 && out < a0 + 4 * num_fine_row) || (out >= r0 && out < r0 + 4 * (num_fine_row + 1))) return GKOMI_EINVAL;
    }
    hipLaunchKernelGGL(map_row_kernel, dim3(row_grid(num_fine_row, 16)), dim3(block), 0, to_stream(s),
                       static_cast<int>(num_fine_row), fine_row_ptrs, agg, row_idxs);
    return check_launch();
}

extern "C" int gkomi_pgm_map_col_i32(gkomi_stream_t s, int64_t nnz, const int32_t* fine_col_idxs, const int32_t* agg,
                                     int32_t* col_idxs)
{
    if (nnz < 0) return GKOMI_EINVAL;
    if (nnz == 0) return GKOMI_SUCCESS;
    if (fine_col_idxs == nullptr || agg == nullptr || col_idxs == nullptr) return GKOMI_EINVAL;
    const size_t bytes = sizeof(int32_t) * static_cast<size_t>(nnz);
    // agg has at least one entry; its length (the number of fine rows) is not an argument
    if (overlaps(fine_col_idxs, bytes, col_idxs, bytes) || overlaps(agg, sizeof(int32_t), col_idxs, bytes)) return GKOMI_EINVAL;
    hipLaunchKernelGGL(map_col_kernel, dim3(grid_for(nnz, block)), dim3(block), 0, to_stream(s), nnz, fine_col_idxs, agg,
                       col_idxs);
    return check_launch();
}

extern "C" size_t gkomi_pgm_coarse_coo_workspace_bytes(int64_t nnz)
{
    if (nnz <= 0) return 0;
    return align256(sizeof(int32_t) * static_cast<size_t>(nnz + 1)) + scan_workspace_bytes(nnz + 1);
}

namespace {

// run_of = the exclusive sum of the run heads of (rows, cols): run_of[nnz] = the number of runs
int number_pair_runs(hipStream_t stream, int64_t nnz, const int32_t* rows, const int32_t* cols, void* workspace,
                     int32_t** run_of)
{
    carver c(workspace);
    *run_of = c.take<int32_t>(nnz + 1);
    void* scan_ws = c.take<char>(scan_workspace_bytes(nnz + 1));
    hipLaunchKernelGGL(pair_heads_kernel, dim3(grid_for(nnz + 1, block)), dim3(block), 0, stream, nnz, rows, cols, *run_of);
    return exclusive_sum_i32(stream, *run_of, *run_of, nnz + 1, scan_ws, scan_workspace_bytes(nnz + 1));
}

}  // namespace

extern "C" int gkomi_pgm_count_unrepeated_nnz_i32(gkomi_stream_t s, int64_t nnz, const int32_t* row_idxs,
                                                  const int32_t* col_idxs, int64_t* host_coarse_nnz, void* workspace,
                                                  size_t workspace_bytes)
{
    if (nnz < 0 || host_coarse_nnz == nullptr) return GKOMI_EINVAL;
    if (nnz == 0) {
        *host_coarse_nnz = 0;
        return GKOMI_SUCCESS;
    }
    if (row_idxs == nullptr || col_idxs == nullptr) return GKOMI_EINVAL;
    if (nnz >= INT32_MAX) return GKOMI_ENOTSUPPORTED;
    if (workspace == nullptr || workspace_bytes < gkomi_pgm_coarse_coo_workspace_bytes(nnz)) return GKOMI_EINVAL;
    const size_t bytes = sizeof(int32_t) * static_cast<size_t>(nnz);
    if (overlaps(row_idxs, bytes, workspace, workspace_bytes) || overlaps(col_idxs, bytes, workspace, workspace_bytes))
        return GKOMI_EINVAL;
    hipStream_t stream = to_stream(s);
    int32_t* run_of = nullptr;
    GKOMI_TRY(number_pair_runs(stream, nnz, row_idxs, col_idxs, workspace, &run_of));
    int32_t host = 0;
    GKOMI_TRY(read_i32(stream, run_of + nnz, &host));
    *host_coarse_nnz = host;
    return GKOMI_SUCCESS;
}

extern "C" int gkomi_pgm_find_strongest_neighbor_f64_i32(gkomi_stream_t s, int64_t n, int64_t nnz,
                                                         const int32_t* w_row_ptrs, const int32_t* w_col_idxs,
                                                         const double* w_vals, const double* diag, int32_t* agg,
                                                         int32_t* strongest_neighbor, void* workspace,
                                                         size_t workspace_bytes)
{
    if (n < 0 || nnz < 0) return GKOMI_EINVAL;
    if (n == 0) return GKOMI_SUCCESS;
    if (bad_weight_csr(n, nnz, w_row_ptrs, w_col_idxs, w_vals, diag) || agg == nullptr || strongest_neighbor == nullptr)
        return GKOMI_EINVAL;
    if (too_large(n, nnz)) return GKOMI_ENOTSUPPORTED;
    const size_t bytes = sizeof(int32_t) * static_cast<size_t>(n);
    if (overlaps(agg, bytes, strongest_neighbor, bytes)) return GKOMI_EINVAL;
    if (workspace == nullptr || workspace_bytes < sizeof(int32_t)) return GKOMI_EINVAL;
    if (overlaps(agg, bytes, workspace, workspace_bytes) || overlaps(strongest_neighbor, bytes, workspace, workspace_bytes))
        return GKOMI_EINVAL;
    if (weight_csr_overlaps(n, nnz, w_row_ptrs, w_col_idxs, w_vals, diag, agg, bytes) ||
        weight_csr_overlaps(n, nnz, w_row_ptrs, w_col_idxs, w_vals, diag, strongest_neighbor, bytes) ||
        weight_csr_overlaps(n, nnz, w_row_ptrs, w_col_idxs, w_vals, diag, workspace, workspace_bytes))
        return GKOMI_EINVAL;
    return find_strongest_neighbor_launch(to_stream(s), n, nnz, w_row_ptrs, w_col_idxs, w_vals, diag, agg,
                                          strongest_neighbor, static_cast<int32_t*>(workspace));
}

extern "C" size_t gkomi_pgm_assign_workspace_bytes(int64_t n)
{
    return n > 0 ? align256(3 * sizeof(int32_t) * static_cast<size_t>(n)) : 0;
}

extern "C" int gkomi_pgm_assign_to_exist_agg_f64_i32(gkomi_stream_t s, int64_t n, int64_t nnz,
                                                     const int32_t* w_row_ptrs, const int32_t* w_col_idxs,
                                                     const double* w_vals, const double* diag, int32_t* agg,
                                                     int32_t* intermediate_agg, void* workspace, size_t workspace_bytes)
{
    if (n < 0 || nnz < 0) return GKOMI_EINVAL;
    if (n == 0) return GKOMI_SUCCESS;
    if (bad_weight_csr(n, nnz, w_row_ptrs, w_col_idxs, w_vals, diag) || agg == nullptr) return GKOMI_EINVAL;
    if (too_large(n, nnz)) return GKOMI_ENOTSUPPORTED;
    const size_t bytes = sizeof(int32_t) * static_cast<size_t>(n);
    if (overlaps(agg, bytes, intermediate_agg, bytes)) return GKOMI_EINVAL;
    if (workspace == nullptr || workspace_bytes < gkomi_pgm_assign_workspace_bytes(n)) return GKOMI_EINVAL;
    if (overlaps(agg, bytes, workspace, workspace_bytes) || overlaps(intermediate_agg, bytes, workspace, workspace_bytes))
        return GKOMI_EINVAL;
    if (weight_csr_overlaps(n, nnz, w_row_ptrs, w_col_idxs, w_vals, diag, agg, bytes) ||
        weight_csr_overlaps(n, nnz, w_row_ptrs, w_col_idxs, w_vals, diag, intermediate_agg, bytes) ||
        weight_csr_overlaps(n, nnz, w_row_ptrs, w_col_idxs, w_vals, diag, workspace, workspace_bytes))
        return GKOMI_EINVAL;
    return assign_to_exist_agg_launch(to_stream(s), n, nnz, w_row_ptrs, w_col_idxs, w_vals, diag, agg, intermediate_agg,
                                      intermediate_agg != nullptr, static_cast<int32_t*>(workspace));
}

extern "C" int gkomi_pgm_sort_row_major_f64_i32(gkomi_stream_t s, int64_t nnz, int32_t* row_idxs, int32_t* col_idxs,
                                                double* vals, void* workspace, size_t workspace_bytes)
{
    if (nnz < 0) return GKOMI_EINVAL;
    if (nnz == 0) return GKOMI_SUCCESS;
    if (row_idxs == nullptr || col_idxs == nullptr || vals == nullptr) return GKOMI_EINVAL;
    if (nnz >= INT32_MAX) return GKOMI_ENOTSUPPORTED;
    const size_t ib = sizeof(int32_t) * static_cast<size_t>(nnz), vb = sizeof(double) * static_cast<size_t>(nnz);
    if (overlaps(row_idxs, ib, col_idxs, ib) || overlaps(row_idxs, ib, vals, vb) || overlaps(col_idxs, ib, vals, vb))
        return GKOMI_EINVAL;
    if (workspace == nullptr || workspace_bytes < gkomi_pgm_sort_workspace_bytes(nnz)) return GKOMI_EINVAL;
    if (overlaps(row_idxs, ib, workspace, workspace_bytes) || overlaps(col_idxs, ib, workspace, workspace_bytes) ||
        overlaps(vals, vb, workspace, workspace_bytes))
        return GKOMI_EINVAL;
    hipStream_t stream = to_stream(s);
    carver c(workspace);
    uint64_t* keys = c.take<uint64_t>(nnz);
    uint64_t* keys_out = c.take<uint64_t>(nnz);
    uint32_t* payload = c.take<uint32_t>(nnz);
    uint32_t* payload_out = c.take<uint32_t>(nnz);
    double* vals_in = c.take<double>(nnz);
    void* sort_ws = c.take<char>(radix_sort_workspace_bytes(nnz, 8, true));
    const int grid = grid_for(nnz, block);
    hipLaunchKernelGGL(pack_keys_kernel, dim3(grid), dim3(block), 0, stream, nnz, row_idxs, col_idxs, 32, keys, payload);
    GKOMI_TRY(static_cast<int>(hipMemcpyAsync(vals_in, vals, vb, hipMemcpyDeviceToDevice, stream)));
    GKOMI_TRY(radix_sort_u64(stream, nnz, keys, keys_out, payload, payload_out, 64, sort_ws,
                             radix_sort_workspace_bytes(nnz, 8, true)));
    hipLaunchKernelGGL(unpack_keys_kernel, dim3(grid), dim3(block), 0, stream, nnz, keys_out, 32, row_idxs, col_idxs);
    hipLaunchKernelGGL(gather_f64_kernel, dim3(grid), dim3(block), 0, stream, nnz, payload_out, vals_in, vals);
    return check_launch();
}

extern "C" int gkomi_pgm_compute_coarse_coo_f64_i32(gkomi_stream_t s, int64_t fine_nnz, const int32_t* row_idxs,
                                                    const int32_t* col_idxs, const double* vals, int64_t coarse_nnz,
                                                    int32_t* coarse_row_idxs, int32_t* coarse_col_idxs,
                                                    double* coarse_vals, void* workspace, size_t workspace_bytes)
{
    if (fine_nnz < 0 || coarse_nnz < 0 || coarse_nnz > fine_nnz) return GKOMI_EINVAL;
    if (fine_nnz == 0) return GKOMI_SUCCESS;
    if (row_idxs == nullptr || col_idxs == nullptr || vals == nullptr || coarse_nnz == 0 || coarse_row_idxs == nullptr ||
        coarse_col_idxs == nullptr || coarse_vals == nullptr)
        return GKOMI_EINVAL;
    if (fine_nnz >= INT32_MAX) return GKOMI_ENOTSUPPORTED;
    const size_t ib = sizeof(int32_t) * static_cast<size_t>(fine_nnz), vb = sizeof(double) * static_cast<size_t>(fine_nnz);
    const size_t cib = sizeof(int32_t) * static_cast<size_t>(coarse_nnz), cvb = sizeof(double) * static_cast<size_t>(coarse_nnz);
    const void* ins[3] = {row_idxs, col_idxs, vals};
    const size_t in_bytes[3] = {ib, ib, vb};
    const void* outs[3] = {coarse_row_idxs, coarse_col_idxs, coarse_vals};
    const size_t out_bytes[3] = {cib, cib, cvb};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            if (overlaps(ins[i], in_bytes[i], outs[j], out_bytes[j])) return GKOMI_EINVAL;
            if (i < j && overlaps(outs[i], out_bytes[i], outs[j], out_bytes[j])) return GKOMI_EINVAL;
        }
    }
    if (workspace == nullptr || workspace_bytes < gkomi_pgm_coarse_coo_workspace_bytes(fine_nnz)) return GKOMI_EINVAL;
    for (int i = 0; i < 3; ++i) {
        if (overlaps(ins[i], in_bytes[i], workspace, workspace_bytes) ||
            overlaps(outs[i], out_bytes[i], workspace, workspace_bytes))
            return GKOMI_EINVAL;
    }
    hipStream_t stream = to_stream(s);
    int32_t* run_of = nullptr;
    GKOMI_TRY(number_pair_runs(stream, fine_nnz, row_idxs, col_idxs, workspace, &run_of));
    // the caller's count is what sized the outputs (GKO_ASSERT of pgm_kernels.cpp:341): nothing is written unless it
    // is the number of runs
    int32_t runs = 0;
    GKOMI_TRY(read_i32(stream, run_of + fine_nnz, &runs));
    if (runs != coarse_nnz) return GKOMI_EINVAL;
    hipLaunchKernelGGL(coarse_sum_kernel<false>, dim3(grid_for(fine_nnz, block)), dim3(block), 0, stream, fine_nnz,
                       static_cast<const uint64_t*>(nullptr), 0, static_cast<const uint32_t*>(nullptr), row_idxs, col_idxs,
                       vals, run_of, coarse_row_idxs, coarse_col_idxs, coarse_vals);
    return check_launch();
}

extern "C" size_t gkomi_pgm_generate_workspace_bytes(int64_t n, int64_t nnz)
{
    if (n <= 0 || nnz < 0) return 0;
    return carve_generate(nullptr, n, nnz).total;
}

extern "C" int gkomi_pgm_generate_f64_i32(gkomi_stream_t s, int64_t n, int64_t nnz, const int32_t* row_ptrs,
                                          const int32_t* col_idxs, const double* vals, int64_t max_iterations,
                                          double max_unassigned_ratio, int deterministic, int skip_sorting,
                                          int32_t* fine_col_idxs, double* fine_vals, int32_t* agg,
                                          int32_t* restrict_row_ptrs, int32_t* restrict_col_idxs,
                                          int32_t* coarse_row_ptrs, int32_t* coarse_col_idxs, double* coarse_vals,
                                          int64_t* host_num_agg, int64_t* host_coarse_nnz, int64_t* host_info,
                                          void* workspace, size_t workspace_bytes)
{
    if (n < 0 || nnz < 0 || max_iterations < 0 || host_num_agg == nullptr || host_coarse_nnz == nullptr)
        return GKOMI_EINVAL;
    if ((coarse_col_idxs == nullptr) != (coarse_vals == nullptr)) return GKOMI_EINVAL;
    const bool count = coarse_col_idxs == nullptr;
    if (n == 0) {
        if (count) {
            *host_num_agg = 0;
            *host_coarse_nnz = 0;
            if (host_info != nullptr) host_info[0] = host_info[1] = host_info[2] = host_info[3] = 0;
        }
        return GKOMI_SUCCESS;
    }
    if (too_large(n, nnz) || 2 * nnz >= INT32_MAX) return GKOMI_ENOTSUPPORTED;
    const generate_ws w = carve_generate(workspace, n, nnz);
    hipStream_t stream = to_stream(s);
    if (!count) {
        if (workspace == nullptr || workspace_bytes < w.total) return GKOMI_EINVAL;
        // the second call: the entries the first one left in the workspace
        const int64_t cnnz = *host_coarse_nnz;
        if (cnnz < 0 || cnnz > nnz) return GKOMI_EINVAL;
        if (cnnz == 0) return GKOMI_SUCCESS;
        if (overlaps(coarse_col_idxs, 4 * cnnz, workspace, workspace_bytes) ||
            overlaps(coarse_vals, 8 * cnnz, workspace, workspace_bytes) ||
            overlaps(coarse_col_idxs, 4 * cnnz, coarse_vals, 8 * cnnz))
            return GKOMI_EINVAL;
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(coarse_col_idxs, w.c_cols, sizeof(int32_t) * static_cast<size_t>(cnnz),
                                                  hipMemcpyDeviceToDevice, stream)));
        return static_cast<int>(hipMemcpyAsync(coarse_vals, w.c_vals, sizeof(double) * static_cast<size_t>(cnnz),
                                               hipMemcpyDeviceToDevice, stream));
    }
    if (row_ptrs == nullptr || agg == nullptr || restrict_row_ptrs == nullptr || restrict_col_idxs == nullptr ||
        coarse_row_ptrs == nullptr)
        return GKOMI_EINVAL;
    if (nnz > 0 && (col_idxs == nullptr || vals == nullptr)) return GKOMI_EINVAL;
    if (!skip_sorting && nnz > 0 && (fine_col_idxs == nullptr || fine_vals == nullptr)) return GKOMI_EINVAL;
    if (workspace == nullptr || workspace_bytes < w.total) return GKOMI_EINVAL;
    {
        const size_t rb = 4 * static_cast<size_t>(n + 1), ib = 4 * static_cast<size_t>(nnz), vb = 8 * static_cast<size_t>(nnz);
        const void* ins[3] = {row_ptrs, col_idxs, vals};
        const size_t in_bytes[3] = {rb, ib, vb};
        const void* outs[6] = {agg, restrict_row_ptrs, restrict_col_idxs, coarse_row_ptrs, fine_col_idxs, fine_vals};
        const size_t out_bytes[6] = {4 * static_cast<size_t>(n), rb, 4 * static_cast<size_t>(n), rb,
                                     skip_sorting ? 0 : ib, skip_sorting ? 0 : vb};
        for (int j = 0; j < 6; ++j) {
            for (int i = 0; i < 3; ++i) {
                if (overlaps(ins[i], in_bytes[i], outs[j], out_bytes[j])) return GKOMI_EINVAL;
            }
            for (int i = 0; i < j; ++i) {
                if (overlaps(outs[i], out_bytes[i], outs[j], out_bytes[j])) return GKOMI_EINVAL;
            }
            if (overlaps(outs[j], out_bytes[j], workspace, workspace_bytes)) return GKOMI_EINVAL;
        }
        for (int i = 0; i < 3; ++i) {
            if (overlaps(ins[i], in_bytes[i], workspace, workspace_bytes)) return GKOMI_EINVAL;
        }
    }

    // 1. the fine operator: sorted unless skipped (pgm.cpp:163-169)
    const int32_t* ci = col_idxs;
    const double* v = vals;
    if (!skip_sorting && nnz > 0) {
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(fine_col_idxs, col_idxs, 4 * static_cast<size_t>(nnz), hipMemcpyDeviceToDevice, stream)));
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(fine_vals, vals, 8 * static_cast<size_t>(nnz), hipMemcpyDeviceToDevice, stream)));
        GKOMI_TRY(gkomi_csr_sort_by_column_index_f64_i32(s, n, row_ptrs, fine_col_idxs, fine_vals));
        ci = fine_col_idxs;
        v = fine_vals;
    }
    // 2., 3. W = 0.5 |A| + 0.5 |A|^T and its diagonal (pgm.cpp:177-186)
    int64_t wnnz = 0;
    if (nnz > 0) {
        static const double half_host = 0.5;
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(w.half, &half_host, sizeof(double), hipMemcpyHostToDevice, stream)));
        hipLaunchKernelGGL(absolute_kernel, dim3(grid_for(nnz, block)), dim3(block), 0, stream, nnz, v, w.absv);
        GKOMI_TRY(check_launch());
        GKOMI_TRY(gkomi_csr_transpose_f64_i32(s, n, n, nnz, row_ptrs, ci, w.absv, w.trp, w.tci, w.tv, w.sub, w.sub_bytes));
        GKOMI_TRY(gkomi_csr_spgeam_f64_i32(s, n, n, w.half, nnz, row_ptrs, ci, w.absv, w.half, n, n, nnz, w.trp, w.tci,
                                           w.tv, w.wrp, nullptr, nullptr, &wnnz, w.sub, w.sub_bytes));
        if (wnnz > 2 * nnz) return GKOMI_EINVAL;
        GKOMI_TRY(gkomi_csr_spgeam_f64_i32(s, n, n, w.half, nnz, row_ptrs, ci, w.absv, w.half, n, n, nnz, w.trp, w.tci,
                                           w.tv, w.wrp, w.wci, w.wv, &wnnz, w.sub, w.sub_bytes));
        GKOMI_TRY(gkomi_csr_extract_diagonal_f64_i32(s, n, w.wrp, w.wci, w.wv, w.diag));
    } else {
        GKOMI_TRY(static_cast<int>(hipMemsetAsync(w.wrp, 0, 4 * static_cast<size_t>(n + 1), stream)));
        GKOMI_TRY(static_cast<int>(hipMemsetAsync(w.diag, 0, 8 * static_cast<size_t>(n), stream)));
    }
    // 4., 5. the matching rounds; the host's three-way check costs one 4-byte read per round
    GKOMI_TRY(fill_i32(stream, n, -1, agg));
    GKOMI_TRY(fill_i32(stream, n, -1, w.strongest));
    int32_t* assigned = w.counters;
    GKOMI_TRY(static_cast<int>(hipMemsetAsync(assigned, 0, sizeof(int32_t), stream)));
    int64_t num_unagg = n, num_unagg_prev = n, iterations = 0, reason = 3;  // 3: max_iterations ran out
    for (int64_t it = 0; it < max_iterations; ++it) {
        GKOMI_TRY(find_strongest_neighbor_launch(stream, n, wnnz, w.wrp, w.wci, w.wv, w.diag, agg, w.strongest, assigned));
        hipLaunchKernelGGL(match_edge_kernel, dim3(static_cast<unsigned>(ceildiv(n, block))), dim3(block), 0, stream,
                           static_cast<int>(n), w.strongest, agg, assigned);
        GKOMI_TRY(check_launch());
        int32_t done = 0;
        GKOMI_TRY(read_i32(stream, assigned, &done));
        num_unagg = n - done;
        iterations = it + 1;
        if (num_unagg == 0) {
            reason = 0;
            break;
        }
        if (num_unagg == num_unagg_prev) {
            reason = 1;
            break;
        }
        if (static_cast<double>(num_unagg) < max_unassigned_ratio * static_cast<double>(n)) {
            reason = 2;
            break;
        }
        num_unagg_prev = num_unagg;
    }
    // 6. the rows left over
    if (num_unagg != 0) {
        GKOMI_TRY(assign_to_exist_agg_launch(stream, n, wnnz, w.wrp, w.wci, w.wv, w.diag, agg, nullptr, deterministic != 0,
                                             w.scratch));
    }
    // 7. renumber
    const int32_t* num_agg_dev = nullptr;
    GKOMI_TRY(renumber_launch(stream, n, agg, w.sub, &num_agg_dev));
    int32_t num_agg = 0;
    GKOMI_TRY(read_i32(stream, num_agg_dev, &num_agg));
    if (num_agg <= 0 || num_agg > n) return GKOMI_EINVAL;
    // 9. the restriction: (agg[i], i) sorted, then row pointers.  i ascends already and the sort is stable, so the key
    // is agg alone
    const int bits = index_bits(num_agg);
    {
        uint32_t* keys32_out = reinterpret_cast<uint32_t*>(w.keys_out);
        GKOMI_TRY(trs_iota(stream, n, reinterpret_cast<int32_t*>(w.payload)));
        GKOMI_TRY(radix_sort_u32(stream, n, reinterpret_cast<const uint32_t*>(agg), keys32_out, w.payload,
                                 reinterpret_cast<uint32_t*>(restrict_col_idxs), bits, w.sub, w.sub_bytes));
        GKOMI_TRY(gkomi_convert_idxs_to_ptrs_i32(s, reinterpret_cast<const int32_t*>(keys32_out), n, num_agg,
                                                 restrict_row_ptrs, w.sub, w.sub_bytes));
    }
    // 10. the coarse matrix
    int32_t coarse_nnz = 0;
    if (nnz > 0) {
        hipLaunchKernelGGL(coarse_keys_kernel, dim3(row_grid(n, 16)), dim3(block), 0, stream, static_cast<int>(n), row_ptrs,
                           ci, agg, bits, w.keys, w.payload);
        GKOMI_TRY(check_launch());
        GKOMI_TRY(radix_sort_u64(stream, nnz, w.keys, w.keys_out, w.payload, w.payload_out, 2 * bits, w.sub, w.sub_bytes));
        hipLaunchKernelGGL(key_heads_kernel, dim3(grid_for(nnz + 1, block)), dim3(block), 0, stream, nnz, w.keys_out, w.run_of);
        GKOMI_TRY(exclusive_sum_i32(stream, w.run_of, w.run_of, nnz + 1, w.sub, w.sub_bytes));
        hipLaunchKernelGGL(coarse_sum_kernel<true>, dim3(grid_for(nnz, block)), dim3(block), 0, stream, nnz, w.keys_out, bits,
                           w.payload_out, static_cast<const int32_t*>(nullptr), static_cast<const int32_t*>(nullptr), v,
                           w.run_of, w.c_rows, w.c_cols, w.c_vals);
        GKOMI_TRY(check_launch());
        GKOMI_TRY(read_i32(stream, w.run_of + nnz, &coarse_nnz));
    }
    GKOMI_TRY(gkomi_convert_idxs_to_ptrs_i32(s, w.c_rows, coarse_nnz, num_agg, coarse_row_ptrs, w.sub, w.sub_bytes));
    *host_num_agg = num_agg;
    *host_coarse_nnz = coarse_nnz;
    if (host_info != nullptr) {
        host_info[0] = iterations;
        host_info[1] = num_unagg;
        host_info[2] = reason;
        host_info[3] = num_unagg != 0 && !deterministic ? jump_rounds(n) : 0;
    }
    return GKOMI_SUCCESS;
}
