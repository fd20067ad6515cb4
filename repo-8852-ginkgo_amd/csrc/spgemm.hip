// Csr<double, int32> times Csr and plus Csr for gfx950: csr::spgemm, csr::advanced_spgemm and csr::spgeam
// (core/matrix/csr_kernels.hpp; the reference's HIP backend hands all three to a vendor library,
// hip/matrix/csr_kernels.hip.cpp).  Every result is bit for bit what the loops of
// reference/matrix/csr_kernels.cpp:209-357 and reference/components/csr_spgeam.hpp:58-104 produce.
//
// SpGEMM, C = A B or C = alpha A B + beta D, in two calls (count, fill) that share one workspace.
//  1. One pass over the rows of A: u(i) = sum of the lengths of the B rows that row i refers to (+ the length of
//     D's row), in 64 bits, and a bin by u: 0 | <= 32 | <= 512 | <= 2048 | beyond (gkomi_csr_spgemm_bins).  The
//     bin lists and their lengths stay in the workspace for the second call; the host never reads them, every
//     kernel below takes a capped grid and strides over the list of its bin.  A second small kernel notes whether
//     every row of B (and of D) is strictly ascending, i.e. free of repeated columns.
//  2. Count: a group of G = 8 / 64 / 256 lanes owns a row and inserts the columns into a hash set in LDS of the
//     smallest power of two >= 2 u entries (64 / 1024 / 4096 at most: 24 or 48 KB per workgroup of 256 threads,
//     three or more workgroups per CU).  A key is claimed with an LDS compare-and-swap, linear probing; the group
//     counts its successful claims.  Rows beyond 2048 products use a dense marker array of n = B's columns per
//     workgroup (in the workspace) and count the marks between the least and the greatest column they touched.
//     Row lengths are summed in 64 bits; nnz(C) > INT32_MAX is reported, not wrapped.
//  3. Fill: the same walk with a double beside each key and a table of >= 2 * (the now exact row length)
//     entries.  The order of the additions is the reference's because the group loops over the nonzeros of
//     A's row SEQUENTIALLY and only the products of one nonzero (one B row) are spread over its lanes: in a
//     strictly ascending B row all columns differ, so the lanes never meet on a slot, a plain LDS
//     read-add-write is enough, and a wave or workgroup barrier between two nonzeros orders the steps.  D's row
//     is one more such step in front.  Then a bitonic sort of (key, value) in LDS -- empty slots are INT32_MAX
//     and go last -- and the row is written in ascending column order.  No atomics on doubles anywhere.
//     If a row of B or D is not strictly ascending (unsorted, or a repeated column), lanes could meet, so
//     every row runs with ONE lane of its group walking the reference loop literally (the other lanes still
//     clear and sort the table).  That is exact for any input at the cost of speed; sort B first
//     (gkomi_csr_sort_by_column_index_f64_i32) if its columns are merely unordered.  A is never required to be
//     sorted or duplicate-free: its nonzeros are taken one after the other in storage order.
//  Bytes: A once, every B row once per reference to it (12 B per product), C once (12 B per entry).
//
// SpGEAM, C = alpha A + beta B: one lane per row runs the reference's two-pointer merge, once to count and
// once to fill; unsorted input gives what that merge gives.
#include "common.hpp"

#include <climits>

namespace gkomi {
namespace {

constexpr int block = 256;
constexpr int32_t empty_key = INT32_MAX;  // column indices are < n <= INT32_MAX
constexpr int64_t bin_small = 32, bin_medium = 512, bin_large = 2048;
constexpr int num_bins = 4;  // small, medium, large, dense
constexpr int max_list_blocks = 2048;
constexpr int max_dense_blocks = 64;
constexpr size_t dense_budget_bytes = size_t{256} << 20;

// header words at the start of the workspace
constexpr int hdr_count = 0;   // [4] rows in each bin
constexpr int hdr_serial = 8;  // != 0: a row of B or D is not strictly ascending

struct spgemm_ws {
    int32_t* header;
    int64_t* ptrs64;
    void* scan_ws;
    size_t scan_bytes;
    int32_t* work;  // u of the row, clamped (the LDS bins need u <= 2048 only)
    int32_t* lists[num_bins];
    int dense_blocks;
    int32_t* marks;
    double* dense_vals;
    size_t total;
};

int dense_blocks_for(int64_t n)
{
    const int64_t per_block = 12 * (n > 0 ? n : 1);
    int64_t w = static_cast<int64_t>(dense_budget_bytes) / per_block;
    if (w > max_dense_blocks) w = max_dense_blocks;
    if (w < 1) w = 1;
    return static_cast<int>(w);
}

spgemm_ws carve_spgemm(void* base, int64_t m, int64_t n)
{
    const size_t rows = static_cast<size_t>(m > 0 ? m : 1);
    const size_t cols = static_cast<size_t>(n > 0 ? n : 1);
    char* p = static_cast<char*>(base);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        char* r = p + at;
        at += align256(bytes);
        return static_cast<void*>(r);
    };
    spgemm_ws w{};
    w.header = static_cast<int32_t*>(take(256));
    w.ptrs64 = static_cast<int64_t*>(take(8 * (rows + 1)));
    w.scan_bytes = gkomi_prefix_sum_workspace_bytes(static_cast<int64_t>(rows) + 1);
    w.scan_ws = take(w.scan_bytes);
    w.work = static_cast<int32_t*>(take(4 * rows));
    for (int b = 0; b < num_bins; ++b) w.lists[b] = static_cast<int32_t*>(take(4 * rows));
    w.dense_blocks = dense_blocks_for(n);
    w.marks = static_cast<int32_t*>(take(4 * cols * w.dense_blocks));
    w.dense_vals = static_cast<double*>(take(8 * cols * w.dense_blocks));
    w.total = at;
    return w;
}

struct csr_view {
    const int32_t* row_ptrs;
    const int32_t* col_idxs;
    const double* vals;
};

// flag[0] = 1 if some row has col[k] >= col[k + 1]
__global__ __launch_bounds__(block) void strictly_ascending_kernel(int64_t nrows, const int32_t* __restrict__ row_ptrs,
                                                                   const int32_t* __restrict__ col_idxs,
                                                                   int32_t* __restrict__ flag)
{
    for (int64_t row = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; row < nrows;
         row += static_cast<int64_t>(gridDim.x) * block) {
        const int32_t end = row_ptrs[row + 1];
        bool bad = false;
        for (int32_t k = row_ptrs[row]; k + 1 < end; ++k) bad |= col_idxs[k] >= col_idxs[k + 1];
        if (bad) flag[0] = 1;
    }
}

// u(i), the bin of row i and its place in the bin's list; rows without products have length 0
__global__ __launch_bounds__(block) void analyse_rows_kernel(int64_t m, const int32_t* __restrict__ a_row_ptrs,
                                                             const int32_t* __restrict__ a_col_idxs,
                                                             const int32_t* __restrict__ b_row_ptrs,
                                                             const int32_t* __restrict__ d_row_ptrs,
                                                             int32_t* __restrict__ header, int32_t* __restrict__ work,
                                                             int32_t* __restrict__ list0, int32_t* __restrict__ list1,
                                                             int32_t* __restrict__ list2, int32_t* __restrict__ list3,
                                                             int64_t* __restrict__ ptrs64)
{
    for (int64_t row = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; row < m;
         row += static_cast<int64_t>(gridDim.x) * block) {
        int64_t u = d_row_ptrs != nullptr ? d_row_ptrs[row + 1] - d_row_ptrs[row] : 0;
        const int32_t end = a_row_ptrs[row + 1];
        for (int32_t k = a_row_ptrs[row]; k < end; ++k) {
            const int32_t b_row = a_col_idxs[k];
            u += b_row_ptrs[b_row + 1] - b_row_ptrs[b_row];
        }
        work[row] = static_cast<int32_t>(u < INT32_MAX ? u : INT32_MAX);
        if (u == 0) {
            ptrs64[row] = 0;
            continue;
        }
        const int bin = u <= bin_small ? 0 : u <= bin_medium ? 1 : u <= bin_large ? 2 : 3;
        int32_t* list = bin == 0 ? list0 : bin == 1 ? list1 : bin == 2 ? list2 : list3;
        list[atomicAdd(&header[hdr_count + bin], 1)] = static_cast<int32_t>(row);
    }
}

// orders the LDS traffic of the lanes of one group: a wave runs its LDS operations in program order, so lanes of
// one wave only need the compiler to keep that order; a workgroup needs the barrier
template <int G>
__device__ __forceinline__ void group_sync()
{
    if (G > wave_size) {
        __syncthreads();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// slot of col in the set keys[0 .. mask]; claimed = this call put it there
__device__ __forceinline__ int hash_insert(int32_t* keys, int shift, int mask, int32_t col, bool& claimed)
{
    int h = static_cast<int>((static_cast<uint32_t>(col) * 2654435769u) >> shift) & mask;
    claimed = false;
    for (;;) {
        const int32_t old = atomicCAS(&keys[h], empty_key, col);
        if (old == empty_key) {
            claimed = true;
            return h;
        }
        if (old == col) return h;
        h = (h + 1) & mask;
    }
}

// smallest power of two >= 2 * items (>= 2), as its logarithm
__device__ __forceinline__ int table_log2(int items)
{
    const int want = 2 * (items > 0 ? items : 1);
    return 32 - __clz(want - 1);
}

// One group of G lanes per row of a bin whose rows need at most CAP / 2 table entries.
template <int G, int CAP, bool Numeric>
__global__ __launch_bounds__(block) void spgemm_lds_kernel(const int32_t* __restrict__ list,
                                                           const int32_t* __restrict__ header, int bin,
                                                           const int32_t* __restrict__ work, csr_view a, csr_view b,
                                                           csr_view d, const double* __restrict__ alpha_p,
                                                           const double* __restrict__ beta_p,
                                                           int64_t* __restrict__ ptrs64,
                                                           const int32_t* __restrict__ c_row_ptrs,
                                                           int32_t* __restrict__ c_col_idxs,
                                                           double* __restrict__ c_vals)
{
    constexpr int groups = block / G;
    __shared__ int32_t keys_all[groups * CAP];
    __shared__ double vals_all[Numeric ? groups * CAP : 1];
    __shared__ int32_t claims[groups];
    const int gid = threadIdx.x / G, lane = threadIdx.x % G;
    int32_t* keys = keys_all + gid * CAP;
    double* vals = vals_all + (Numeric ? gid * CAP : 0);
    const int64_t bin_rows = header[hdr_count + bin];
    const bool serial = Numeric && header[hdr_serial] != 0;
    const bool advanced = alpha_p != nullptr;
    const double alpha = advanced ? alpha_p[0] : 1.0;
    const double beta = advanced ? beta_p[0] : 0.0;
    // the lanes that walk, and their stride over a row of B or D
    const bool walks = !serial || lane == 0;
    const int first = serial ? 0 : lane, step = serial ? 1 : G;
    // the trip count is the same for all threads of the workgroup (group_sync may be a workgroup barrier)
    for (int64_t base = blockIdx.x * static_cast<int64_t>(groups); base < bin_rows;
         base += static_cast<int64_t>(gridDim.x) * groups) {
        const int64_t item = base + gid;
        if (G <= wave_size && item >= bin_rows) continue;  // a whole group leaves; no workgroup barrier below
        const int64_t row = list[item];
        const int64_t c_begin = Numeric ? c_row_ptrs[row] : 0;
        const int c_len = Numeric ? static_cast<int>(c_row_ptrs[row + 1] - c_begin) : 0;
        const int lg = table_log2(Numeric ? c_len : work[row]);
        const int cap = 1 << lg, mask = cap - 1, shift = 32 - lg;
        for (int s = lane; s < cap; s += G) {
            keys[s] = empty_key;
            if (Numeric) vals[s] = 0.0;
        }
        if (lane == 0) claims[gid] = 0;
        group_sync<G>();
        int mine = 0;
        bool claimed;
        if (advanced) {
            const int32_t d_end = d.row_ptrs[row + 1];
            if (walks) {
                for (int32_t z = d.row_ptrs[row] + first; z < d_end; z += step) {
                    const int slot = hash_insert(keys, shift, mask, d.col_idxs[z], claimed);
                    mine += claimed;
                    if (Numeric) vals[slot] = vals[slot] + beta * d.vals[z];
                }
            }
            if (Numeric) group_sync<G>();
        }
        const int32_t a_end = a.row_ptrs[row + 1];
        for (int32_t k = a.row_ptrs[row]; k < a_end; ++k) {
            const int32_t b_row = a.col_idxs[k];
            const double a_val = Numeric ? (advanced ? alpha * a.vals[k] : a.vals[k]) : 0.0;
            const int32_t b_end = b.row_ptrs[b_row + 1];
            if (walks) {
                for (int32_t z = b.row_ptrs[b_row] + first; z < b_end; z += step) {
                    const int slot = hash_insert(keys, shift, mask, b.col_idxs[z], claimed);
                    mine += claimed;
                    if (Numeric) vals[slot] = vals[slot] + a_val * b.vals[z];
                }
            }
            // the next nonzero of A may add to the slots this one wrote
            if (Numeric) group_sync<G>();
        }
        if (!Numeric) {
            if (mine != 0) atomicAdd(&claims[gid], mine);
            group_sync<G>();
            if (lane == 0) ptrs64[row] = claims[gid];
            group_sync<G>();  // claims[gid] is reset for the next row only after it was read
            continue;
        }
        // bitonic sort of the table by key; the c_len keys come first, ascending
        for (int size = 2; size <= cap; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = lane; t < (cap >> 1); t += G) {
                    const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
                    const int j = i | stride;
                    const int32_t ki = keys[i], kj = keys[j];
                    if ((ki > kj) == ((i & size) == 0)) {
                        keys[i] = kj;
                        keys[j] = ki;
                        const double vi = vals[i], vj = vals[j];
                        vals[i] = vj;
                        vals[j] = vi;
                    }
                }
                group_sync<G>();
            }
        }
        for (int s = lane; s < c_len; s += G) {
            c_col_idxs[c_begin + s] = keys[s];
            c_vals[c_begin + s] = vals[s];
        }
        group_sync<G>();  // the table is cleared for the next row only after it was read
    }
}

// One workgroup per row with more products than the largest LDS table takes: marks[n] (and values[n]) of this
// workgroup in the workspace, all zero between rows.
template <bool Numeric>
__global__ __launch_bounds__(block) void spgemm_dense_kernel(const int32_t* __restrict__ list,
                                                             const int32_t* __restrict__ header, int bin, int64_t n,
                                                             int32_t* marks_all, double* vals_all, csr_view a, csr_view b,
                                                             csr_view d, const double* __restrict__ alpha_p,
                                                             const double* __restrict__ beta_p,
                                                             int64_t* __restrict__ ptrs64,
                                                             const int32_t* __restrict__ c_row_ptrs,
                                                             int32_t* __restrict__ c_col_idxs,
                                                             double* __restrict__ c_vals)
{
    constexpr int waves = block / wave_size;
    __shared__ int32_t range[2];
    __shared__ int32_t wave_total[waves];
    int32_t* marks = marks_all + blockIdx.x * n;
    double* vals = vals_all + blockIdx.x * n;
    const int tid = threadIdx.x, lane = tid % wave_size, wave = tid / wave_size;
    const int64_t bin_rows = header[hdr_count + bin];
    const bool serial = Numeric && header[hdr_serial] != 0;
    const bool advanced = alpha_p != nullptr;
    const double alpha = advanced ? alpha_p[0] : 1.0;
    const double beta = advanced ? beta_p[0] : 0.0;
    const bool walks = !serial || tid == 0;
    const int first = serial ? 0 : tid, step = serial ? 1 : block;
    for (int64_t item = blockIdx.x; item < bin_rows; item += gridDim.x) {
        const int64_t row = list[item];
        if (tid == 0) {
            range[0] = INT32_MAX;
            range[1] = -1;
        }
        __syncthreads();
        int32_t lo = INT32_MAX, hi = -1;
        if (advanced) {
            const int32_t d_end = d.row_ptrs[row + 1];
            if (walks) {
                for (int32_t z = d.row_ptrs[row] + first; z < d_end; z += step) {
                    const int32_t col = d.col_idxs[z];
                    lo = min(lo, col);
                    hi = max(hi, col);
                    marks[col] = 1;
                    if (Numeric) vals[col] = vals[col] + beta * d.vals[z];
                }
            }
            if (Numeric) __syncthreads();
        }
        const int32_t a_end = a.row_ptrs[row + 1];
        for (int32_t k = a.row_ptrs[row]; k < a_end; ++k) {
            const int32_t b_row = a.col_idxs[k];
            const double a_val = Numeric ? (advanced ? alpha * a.vals[k] : a.vals[k]) : 0.0;
            const int32_t b_end = b.row_ptrs[b_row + 1];
            if (walks) {
                for (int32_t z = b.row_ptrs[b_row] + first; z < b_end; z += step) {
                    const int32_t col = b.col_idxs[z];
                    lo = min(lo, col);
                    hi = max(hi, col);
                    marks[col] = 1;
                    if (Numeric) vals[col] = vals[col] + a_val * b.vals[z];
                }
            }
            // the workgroup's stores to vals are visible to its other waves after the barrier
            if (Numeric) __syncthreads();
        }
        if (hi >= 0) {
            atomicMin(&range[0], lo);
            atomicMax(&range[1], hi);
        }
        __syncthreads();
        const int32_t from = range[0], to = range[1];
        // the marked columns of [from, to] in ascending order, 256 at a time
        int64_t out = Numeric ? c_row_ptrs[row] : 0;
        for (int64_t at = from; at <= to; at += block) {
            const int64_t col = at + tid;
            const bool set = col <= to && marks[col] != 0;
            const uint64_t votes = __ballot(set);
            if (lane == 0) wave_total[wave] = __popcll(votes);
            __syncthreads();
            int before = __popcll(votes & ((uint64_t{1} << lane) - 1));
            int total = 0;
#pragma unroll
            for (int w = 0; w < waves; ++w) {
                if (w < wave) before += wave_total[w];
                total += wave_total[w];
            }
            if (set) {
                marks[col] = 0;
                if (Numeric) {
                    c_col_idxs[out + before] = static_cast<int32_t>(col);
                    c_vals[out + before] = vals[col];
                    vals[col] = 0.0;
                }
            }
            out += total;
            __syncthreads();
        }
        if (!Numeric && tid == 0) ptrs64[row] = out;
        __syncthreads();  // range is reset for the next row only after all have read it
    }
}

__global__ __launch_bounds__(block) void narrow_ptrs_kernel(int64_t n, const int64_t* __restrict__ in,
                                                            int32_t* __restrict__ out)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * block) {
        out[i] = static_cast<int32_t>(in[i]);
    }
}

// exclusive 64-bit sum of the m row lengths in ptrs64, the total to the host (blocking), the narrowed copy to
// c_row_ptrs[m + 1]
int finish_count(hipStream_t stream, int64_t m, int64_t* ptrs64, void* scan_ws, size_t scan_bytes,
                 int32_t* c_row_ptrs, int64_t* host_c_nnz)
{
    GKOMI_TRY(static_cast<int>(hipMemsetAsync(ptrs64 + m, 0, sizeof(int64_t), stream)));
    GKOMI_TRY(gkomi_prefix_sum_i64(stream, ptrs64, m + 1, scan_ws, scan_bytes));
    hipLaunchKernelGGL(narrow_ptrs_kernel, dim3(grid_for(m + 1, block)), dim3(block), 0, stream, m + 1, ptrs64,
                       c_row_ptrs);
    GKOMI_TRY(check_launch());
    int64_t total = 0;
    GKOMI_TRY(static_cast<int>(hipMemcpyAsync(&total, ptrs64 + m, sizeof(int64_t), hipMemcpyDeviceToHost, stream)));
    GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
    *host_c_nnz = total;
    return total > INT32_MAX ? GKOMI_ENOTSUPPORTED : GKOMI_SUCCESS;
}

template <bool Numeric>
int launch_bins(hipStream_t stream, const spgemm_ws& w, int64_t m, int64_t n, csr_view a, csr_view b, csr_view d,
                const double* alpha, const double* beta, const int32_t* c_row_ptrs, int32_t* c_col_idxs,
                double* c_vals)
{
    hipLaunchKernelGGL((spgemm_lds_kernel<8, 64, Numeric>), dim3(grid_for(m, block / 8, max_list_blocks)), dim3(block),
                       0, stream, w.lists[0], w.header, 0, w.work, a, b, d, alpha, beta, w.ptrs64, c_row_ptrs,
                       c_col_idxs, c_vals);
    GKOMI_TRY(check_launch());
    hipLaunchKernelGGL((spgemm_lds_kernel<64, 1024, Numeric>), dim3(grid_for(m, block / 64, max_list_blocks)),
                       dim3(block), 0, stream, w.lists[1], w.header, 1, w.work, a, b, d, alpha, beta, w.ptrs64,
                       c_row_ptrs, c_col_idxs, c_vals);
    GKOMI_TRY(check_launch());
    hipLaunchKernelGGL((spgemm_lds_kernel<256, 4096, Numeric>), dim3(grid_for(m, 1, max_list_blocks)), dim3(block), 0,
                       stream, w.lists[2], w.header, 2, w.work, a, b, d, alpha, beta, w.ptrs64, c_row_ptrs,
                       c_col_idxs, c_vals);
    GKOMI_TRY(check_launch());
    hipLaunchKernelGGL(spgemm_dense_kernel<Numeric>, dim3(grid_for(m, 1, w.dense_blocks)), dim3(block), 0, stream,
                       w.lists[3], w.header, 3, n, w.marks, w.dense_vals, a, b, d, alpha, beta, w.ptrs64, c_row_ptrs,
                       c_col_idxs, c_vals);
    return check_launch();
}

// the reference's merge of two rows (reference/components/csr_spgeam.hpp:73-102)
template <bool Numeric>
__global__ __launch_bounds__(block) void spgeam_kernel(int64_t m, csr_view a, csr_view b,
                                                       const double* __restrict__ alpha_p,
                                                       const double* __restrict__ beta_p,
                                                       int64_t* __restrict__ ptrs64,
                                                       const int32_t* __restrict__ c_row_ptrs,
                                                       int32_t* __restrict__ c_col_idxs, double* __restrict__ c_vals)
{
    const double alpha = Numeric ? alpha_p[0] : 0.0, beta = Numeric ? beta_p[0] : 0.0;
    for (int64_t row = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; row < m;
         row += static_cast<int64_t>(gridDim.x) * block) {
        int32_t a_begin = a.row_ptrs[row], b_begin = b.row_ptrs[row];
        const int32_t a_end = a.row_ptrs[row + 1], b_end = b.row_ptrs[row + 1];
        const int64_t total_size = static_cast<int64_t>(a_end - a_begin) + (b_end - b_begin);
        bool skip = false;
        int64_t nz = Numeric ? c_row_ptrs[row] : 0;
        for (int64_t i = 0; i < total_size; ++i) {
            if (skip) {
                skip = false;
                continue;
            }
            const int32_t a_col = a_begin < a_end ? a.col_idxs[a_begin] : INT32_MAX;
            const int32_t b_col = b_begin < b_end ? b.col_idxs[b_begin] : INT32_MAX;
            if (Numeric) {
                const double a_val = a_begin < a_end ? a.vals[a_begin] : 0.0;
                const double b_val = b_begin < b_end ? b.vals[b_begin] : 0.0;
                const int32_t col = min(a_col, b_col);
                c_vals[nz] = alpha * (a_col == col ? a_val : 0.0) + beta * (b_col == col ? b_val : 0.0);
                c_col_idxs[nz] = col;
            }
            ++nz;
            a_begin += a_col <= b_col;
            b_begin += b_col <= a_col;
            skip = a_col == b_col;
        }
        if (!Numeric) ptrs64[row] = nz;
    }
}

struct spgeam_ws {
    int64_t* ptrs64;
    void* scan_ws;
    size_t scan_bytes;
    size_t total;
};

spgeam_ws carve_spgeam(void* base, int64_t m)
{
    const size_t rows = static_cast<size_t>(m > 0 ? m : 1);
    spgeam_ws w{};
    w.ptrs64 = static_cast<int64_t*>(base);
    w.scan_bytes = gkomi_prefix_sum_workspace_bytes(static_cast<int64_t>(rows) + 1);
    w.scan_ws = static_cast<char*>(base) + align256(8 * (rows + 1));
    w.total = align256(8 * (rows + 1)) + align256(w.scan_bytes);
    return w;
}

bool bad_csr(int64_t nrows, int64_t nnz, const int32_t* row_ptrs, const int32_t* col_idxs, const double* vals)
{
    if (nrows > 0 && row_ptrs == nullptr) return true;
    return nnz > 0 && (col_idxs == nullptr || vals == nullptr);
}

}  // namespace
}  // namespace gkomi

using namespace gkomi;

extern "C" int gkomi_csr_spgemm_bins(int64_t out[3])
{
    if (out == nullptr) return GKOMI_EINVAL;
    out[0] = bin_small;
    out[1] = bin_medium;
    out[2] = bin_large;
    return GKOMI_SUCCESS;
}

extern "C" size_t gkomi_csr_spgemm_workspace_bytes(int64_t a_nrows, int64_t b_ncols)
{
    if (a_nrows < 0 || b_ncols < 0) return 0;
    return carve_spgemm(nullptr, a_nrows, b_ncols).total;
}

extern "C" int gkomi_csr_spgemm_f64_i32(gkomi_stream_t s, int64_t a_nrows, int64_t a_ncols, int64_t a_nnz,
                                        const int32_t* a_row_ptrs, const int32_t* a_col_idxs, const double* a_vals,
                                        int64_t b_nrows, int64_t b_ncols, int64_t b_nnz, const int32_t* b_row_ptrs,
                                        const int32_t* b_col_idxs, const double* b_vals, const double* alpha,
                                        const double* beta, int64_t d_nrows, int64_t d_ncols, int64_t d_nnz,
                                        const int32_t* d_row_ptrs, const int32_t* d_col_idxs, const double* d_vals,
                                        int32_t* c_row_ptrs, int32_t* c_col_idxs, double* c_vals,
                                        int64_t* host_c_nnz, void* workspace, size_t workspace_bytes)
{
    const int64_t m = a_nrows, n = b_ncols;
    if (a_nrows < 0 || a_ncols < 0 || a_nnz < 0 || b_nrows < 0 || b_ncols < 0 || b_nnz < 0) return GKOMI_EINVAL;
    if (host_c_nnz == nullptr || c_row_ptrs == nullptr) return GKOMI_EINVAL;
    const bool advanced = alpha != nullptr;
    if ((beta != nullptr) != advanced || (d_row_ptrs != nullptr) != advanced) return GKOMI_EINVAL;
    if (a_ncols != b_nrows) return GKOMI_EINVAL;  // GKO_ASSERT_CONFORMANT
    if (advanced && (d_nnz < 0 || d_nrows != m || d_ncols != n)) return GKOMI_EINVAL;  // GKO_ASSERT_EQUAL_DIMENSIONS
    if (bad_csr(m, a_nnz, a_row_ptrs, a_col_idxs, a_vals) || bad_csr(b_nrows, b_nnz, b_row_ptrs, b_col_idxs, b_vals)) return GKOMI_EINVAL;
    if (advanced && bad_csr(m, d_nnz, d_row_ptrs, d_col_idxs, d_vals)) return GKOMI_EINVAL;
    if ((c_col_idxs == nullptr) != (c_vals == nullptr)) return GKOMI_EINVAL;
    if (m > INT32_MAX || n > INT32_MAX || b_nrows > INT32_MAX || a_nnz > INT32_MAX || b_nnz > INT32_MAX ||
        (advanced && d_nnz > INT32_MAX)) {
        return GKOMI_ENOTSUPPORTED;
    }
    const bool count = c_col_idxs == nullptr;
    hipStream_t stream = to_stream(s);
    if (m == 0) {
        if (!count) return GKOMI_SUCCESS;
        *host_c_nnz = 0;
        GKOMI_TRY(static_cast<int>(hipMemsetAsync(c_row_ptrs, 0, sizeof(int32_t), stream)));
        return static_cast<int>(hipStreamSynchronize(stream));
    }
    const spgemm_ws w = carve_spgemm(workspace, m, n);
    if (workspace == nullptr || workspace_bytes < w.total) return GKOMI_EWORKSPACE;
    const csr_view a{a_row_ptrs, a_col_idxs, a_vals}, b{b_row_ptrs, b_col_idxs, b_vals};
    const csr_view d{d_row_ptrs, d_col_idxs, d_vals};
    if (count) {
        GKOMI_TRY(static_cast<int>(hipMemsetAsync(w.header, 0, 256, stream)));
        // the dense rows find their marks and values zero and leave them so
        GKOMI_TRY(static_cast<int>(hipMemsetAsync(w.marks, 0, sizeof(int32_t) * static_cast<size_t>(n) * w.dense_blocks, stream)));
        GKOMI_TRY(static_cast<int>(hipMemsetAsync(w.dense_vals, 0, sizeof(double) * static_cast<size_t>(n) * w.dense_blocks, stream)));
        if (b_nrows > 0 && b_nnz > 0) {
            hipLaunchKernelGGL(strictly_ascending_kernel, dim3(grid_for(b_nrows, block)), dim3(block), 0, stream, b_nrows,
                               b_row_ptrs, b_col_idxs, w.header + hdr_serial);
            GKOMI_TRY(check_launch());
        }
        if (advanced && d_nnz > 0) {
            hipLaunchKernelGGL(strictly_ascending_kernel, dim3(grid_for(m, block)), dim3(block), 0, stream, m, d_row_ptrs,
                               d_col_idxs, w.header + hdr_serial);
            GKOMI_TRY(check_launch());
        }
        hipLaunchKernelGGL(analyse_rows_kernel, dim3(grid_for(m, block)), dim3(block), 0, stream, m, a_row_ptrs,
                           a_col_idxs, b_row_ptrs, d_row_ptrs, w.header, w.work, w.lists[0], w.lists[1], w.lists[2],
                           w.lists[3], w.ptrs64);
        GKOMI_TRY(check_launch());
        GKOMI_TRY(launch_bins<false>(stream, w, m, n, a, b, d, alpha, beta, nullptr, nullptr, nullptr));
        return finish_count(stream, m, w.ptrs64, w.scan_ws, w.scan_bytes, c_row_ptrs, host_c_nnz);
    }
    if (*host_c_nnz < 0 || *host_c_nnz > INT32_MAX) return GKOMI_EINVAL;
    if (*host_c_nnz == 0) return GKOMI_SUCCESS;
    return launch_bins<true>(stream, w, m, n, a, b, d, alpha, beta, c_row_ptrs, c_col_idxs, c_vals);
}

extern "C" size_t gkomi_csr_spgeam_workspace_bytes(int64_t nrows)
{
    if (nrows < 0) return 0;
    return carve_spgeam(nullptr, nrows).total;
}

extern "C" int gkomi_csr_spgeam_f64_i32(gkomi_stream_t s, int64_t nrows, int64_t ncols, const double* alpha,
                                        int64_t a_nnz, const int32_t* a_row_ptrs, const int32_t* a_col_idxs,
                                        const double* a_vals, const double* beta, int64_t b_nrows, int64_t b_ncols,
                                        int64_t b_nnz, const int32_t* b_row_ptrs, const int32_t* b_col_idxs,
                                        const double* b_vals, int32_t* c_row_ptrs, int32_t* c_col_idxs,
                                        double* c_vals, int64_t* host_c_nnz, void* workspace,
                                        size_t workspace_bytes)
{
    const int64_t m = nrows;
    if (nrows < 0 || ncols < 0 || a_nnz < 0 || b_nnz < 0) return GKOMI_EINVAL;
    if (b_nrows != nrows || b_ncols != ncols) return GKOMI_EINVAL;  // GKO_ASSERT_EQUAL_DIMENSIONS
    if (alpha == nullptr || beta == nullptr || host_c_nnz == nullptr || c_row_ptrs == nullptr) return GKOMI_EINVAL;
    if (bad_csr(m, a_nnz, a_row_ptrs, a_col_idxs, a_vals) || bad_csr(m, b_nnz, b_row_ptrs, b_col_idxs, b_vals)) return GKOMI_EINVAL;
    if ((c_col_idxs == nullptr) != (c_vals == nullptr)) return GKOMI_EINVAL;
    if (m > INT32_MAX || ncols > INT32_MAX || a_nnz > INT32_MAX || b_nnz > INT32_MAX) return GKOMI_ENOTSUPPORTED;
    const bool count = c_col_idxs == nullptr;
    hipStream_t stream = to_stream(s);
    if (m == 0) {
        if (!count) return GKOMI_SUCCESS;
        *host_c_nnz = 0;
        GKOMI_TRY(static_cast<int>(hipMemsetAsync(c_row_ptrs, 0, sizeof(int32_t), stream)));
        return static_cast<int>(hipStreamSynchronize(stream));
    }
    const spgeam_ws w = carve_spgeam(workspace, m);
    if (workspace == nullptr || workspace_bytes < w.total) return GKOMI_EWORKSPACE;
    const csr_view a{a_row_ptrs, a_col_idxs, a_vals}, b{b_row_ptrs, b_col_idxs, b_vals};
    if (count) {
        hipLaunchKernelGGL(spgeam_kernel<false>, dim3(grid_for(m, block)), dim3(block), 0, stream, m, a, b, alpha, beta,
                           w.ptrs64, static_cast<const int32_t*>(nullptr), static_cast<int32_t*>(nullptr),
                           static_cast<double*>(nullptr));
        GKOMI_TRY(check_launch());
        return finish_count(stream, m, w.ptrs64, w.scan_ws, w.scan_bytes, c_row_ptrs, host_c_nnz);
    }
    if (*host_c_nnz < 0 || *host_c_nnz > INT32_MAX) return GKOMI_EINVAL;
    if (*host_c_nnz == 0) return GKOMI_SUCCESS;
    hipLaunchKernelGGL(spgeam_kernel<true>, dim3(grid_for(m, block)), dim3(block), 0, stream, m, a, b, alpha, beta, w.ptrs64,
                       c_row_ptrs, c_col_idxs, c_vals);
    return check_launch();
}
