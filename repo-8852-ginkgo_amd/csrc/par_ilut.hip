// ParILUT: factorization::ParIlut (core/factorization/par_ilut.cpp:190-344), the five kernels of
// reference/factorization/par_ilut_kernels.cpp with the results of the REFERENCE executor, bit for bit:
// threshold_select (:73-90), threshold_filter (:103-182), threshold_filter_approx (:198-253),
// compute_l_u_factors (:264-341), add_candidates (:355-464 over reference/components/csr_spgeam.hpp:58-104).
// <double, int32>.  No vendor library.
//
// The sweep.  The reference executor's compute_l_u_factors is ONE sequential in-place sweep in row order.
// Entry (row, col) reads l(row, k), u(k, col) and u(col, col) for k < min(row, col) only, and every one of
// them has been rewritten earlier in the same sweep: the result is an order-determined incomplete
// factorization on the current pattern, not a relaxation step, and it can be reproduced by any schedule
// that finishes row k before a row i that stores l(i, k).  That is the lower-triangular level structure of
// L', which the analysis of ilu.hip (gkomi_ilu_analyse_i32) computes; it runs here on the "combined"
// pattern M = strictly lower part of L' + U' (row i of M: the lower columns of L' without the unit
// diagonal, then the row of U', which starts with its diagonal), so its row lengths -- and with them its
// bins -- are those of the working row of the sweep.
//
// Bits.  compute_sum (:287-317) starts every sum at +0.0 and adds l(row, k) * u(k, col) over the k that both
// store, in ascending k, one rounding per product and per sum; then a - sum (a = 0.0 where A does not store
// the entry), then, below the diagonal, one IEEE quotient by u(col, col).  A value that is not finite leaves
// the old one in place, and the old one is what later entries read.  The row-wise IKJ form used here walks
// the lower columns k of row i in ascending order, finishes l(i, k) from the running sum of entry (i, k),
// and adds l(i, k) * u(k, j) to the running sum of every stored j > k of row i that row k of U stores:
// every entry receives the same products in the same order.  The library is built with -ffp-contract=off.
// U is read by rows (CSR); the reference reads its CSC copy, which holds the same values at every moment
// of its sweep.  ut_vals is brought up to date from u_vals afterwards.
//
// Scheduling: as in fact_levels.hpp, whose frame runs sweep_row over the levels of M (boundaries:
// gkomi_par_ilut_tuning).
#include "common.hpp"

#include <cmath>
#include <cstring>

#include "fact_levels.hpp"
#include "internal.hpp"
#include "sort_scan.hpp"

namespace gkomi {
namespace {

using namespace fact;

constexpr int block = 256;
// sampleselect_searchtree_height = 8, sampleselect_oversampling = 4 (core/factorization/par_ilut_kernels.hpp:99-100)
constexpr int bucket_count = 256;
constexpr int oversampling = 4;
constexpr int sample_size = bucket_count * oversampling;

constexpr int64_t sweep_magic = 0x70696c7574737770ll;

__device__ __forceinline__ uint64_t abs_bits(double v)
{
    return static_cast<uint64_t>(__double_as_longlong(v)) & 0x7fffffffffffffffull;
}

// ---- threshold_select ---------------------------------------------------------------------------------
__global__ __launch_bounds__(block) void abs_keys_kernel(int64_t nnz, const double* __restrict__ vals,
                                                         uint64_t* __restrict__ keys)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i < nnz;
         i += static_cast<int64_t>(gridDim.x) * block) {
        keys[i] = abs_bits(vals[i]);
    }
}

struct select_ws {
    size_t keys_in, keys_out, sort, sort_bytes, total;
};

select_ws carve_select(int64_t nnz)
{
    const size_t m = static_cast<size_t>(nnz > 0 ? nnz : 1);
    select_ws w{};
    w.keys_in = 0;
    w.keys_out = align256(8 * m);
    w.sort = w.keys_out + align256(8 * m);
    w.sort_bytes = align256(radix_sort_workspace_bytes(static_cast<int64_t>(m), sizeof(uint64_t), false)) + 256;
    w.total = w.sort + w.sort_bytes;
    return w;
}

// ---- threshold_filter: abstract_filter (:103-161), a wave per row -----------------------------------------
template <bool Fill>
__global__ __launch_bounds__(block) void filter_kernel(int32_t n, const int32_t* __restrict__ row_ptrs,
                                                       const int32_t* __restrict__ col_idxs,
                                                       const double* __restrict__ vals, double threshold,
                                                       int32_t* __restrict__ new_row_ptrs,
                                                       int32_t* __restrict__ new_col_idxs,
                                                       double* __restrict__ new_vals,
                                                       int32_t* __restrict__ new_row_idxs)
{
    constexpr int waves = block / wave_size;
    const int lane = threadIdx.x % wave_size;
    for (int row = blockIdx.x * waves + threadIdx.x / wave_size; row < n; row += gridDim.x * waves) {
        const int begin = row_ptrs[row], end = row_ptrs[row + 1];
        int out = Fill ? new_row_ptrs[row] : 0;
        for (int base = begin; base < end; base += wave_size) {
            const int nz = base + lane;
            bool keep = false;
            int col = 0;
            double v = 0.0;
            if (nz < end) {
                col = col_idxs[nz];
                v = vals[nz];
                // a NaN compares false and stays only on the diagonal
                keep = fabs(v) >= threshold || col == row;
            }
            const unsigned long long mask = __ballot(keep);
            if (Fill && keep) {
                const int at = out + __popcll(mask & ((1ull << lane) - 1ull));
                if (new_row_idxs != nullptr) new_row_idxs[at] = row;
                new_col_idxs[at] = col;
                new_vals[at] = v;
            }
            out += __popcll(mask);
        }
        if (!Fill && lane == 0) new_row_ptrs[row] = out;
    }
}

// ---- threshold_filter_approx: the threshold (:206-247) ----------------------------------------------------
// first position of splitters[0, count) whose value is greater than x (std::upper_bound)
__device__ __forceinline__ int upper_bound_f64(const double* s, int count, double x)
{
    int lo = 0;
    while (count > 0) {
        const int half = count / 2;
        if (!(x < s[lo + half])) {
            lo += half + 1;
            count -= half + 1;
        } else {
            count = half;
        }
    }
    return lo;
}

// one workgroup: the sample, sorted (bitonic, on the bits of the magnitudes: the order of non-negative
// doubles), then splitter i = sample[(i + 1) * oversampling]
__global__ __launch_bounds__(sample_size) void sample_splitters_kernel(int32_t nnz, const double* __restrict__ vals,
                                                                      double* __restrict__ splitters,
                                                                      int32_t* __restrict__ histogram)
{
    __shared__ uint64_t sample[sample_size];
    const int i = threadIdx.x;
    const double stride = static_cast<double>(nnz) / sample_size;
    sample[i] = abs_bits(vals[static_cast<int32_t>(i * stride)]);
    if (i < bucket_count) histogram[i] = 0;
    __syncthreads();
    for (int k = 2; k <= sample_size; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int partner = i ^ j;
            if (partner > i) {
                const uint64_t a = sample[i], b = sample[partner];
                const bool ascending = (i & k) == 0;
                if ((a > b) == ascending) {
                    sample[i] = b;
                    sample[partner] = a;
                }
            }
            __syncthreads();
        }
    }
    if (i < bucket_count - 1) splitters[i] = __longlong_as_double(static_cast<long long>(sample[(i + 1) * oversampling]));
}

__global__ __launch_bounds__(block) void histogram_kernel(int32_t nnz, const double* __restrict__ vals,
                                                          const double* __restrict__ splitters,
                                                          int32_t* __restrict__ histogram)
{
    __shared__ double tree[bucket_count];
    __shared__ int32_t local[bucket_count];
    static_assert(block == bucket_count, "one thread per bucket");
    tree[threadIdx.x] = threadIdx.x < bucket_count - 1 ? splitters[threadIdx.x] : 0.0;
    local[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t nz = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; nz < nnz;
         nz += static_cast<int64_t>(gridDim.x) * block) {
        atomicAdd(local + upper_bound_f64(tree, bucket_count - 1, fabs(vals[nz])), 1);
    }
    __syncthreads();
    if (local[threadIdx.x] != 0) atomicAdd(histogram + threadIdx.x, local[threadIdx.x]);
}

// the workspace of the approximate threshold: bucket_count doubles, then bucket_count counts
constexpr size_t approx_splitters = 0, approx_histogram = 8 * bucket_count;
constexpr size_t approx_total = approx_histogram + 4 * bucket_count;
static_assert(approx_histogram % 256 == 0 && approx_total % 256 == 0, "workspace pieces start on 256-byte boundaries");

// ---- add_candidates (:355-464): the merge of row i of A and of LU, one lane per row ---------------------
template <bool Fill>
__global__ __launch_bounds__(block) void add_candidates_kernel(int32_t n, csr_in lu, csr_in a, csr_in l, csr_in u,
                                                               csr_out l_new, csr_out u_new)
{
    for (int row = blockIdx.x * block + threadIdx.x; row < n; row += gridDim.x * block) {
        int a_begin = a.row_ptrs[row], b_begin = lu.row_ptrs[row];
        const int a_end = a.row_ptrs[row + 1], b_end = lu.row_ptrs[row + 1];
        const int64_t total_size = static_cast<int64_t>(a_end - a_begin) + (b_end - b_begin);
        int l_new_nz = 0, u_new_nz = 0, l_old_begin = 0, l_old_end = 0, u_old_begin = 0, u_old_end = 0;
        bool finished_l = true;
        if (Fill) {
            l_new_nz = l_new.row_ptrs[row];
            u_new_nz = u_new.row_ptrs[row];
            l_old_begin = l.row_ptrs[row];
            l_old_end = l.row_ptrs[row + 1] - 1;  // skip diagonal
            u_old_begin = u.row_ptrs[row];
            u_old_end = u.row_ptrs[row + 1];
            finished_l = l_old_begin >= l_old_end;
        }
        bool skip = false;
        for (int64_t i = 0; i < total_size; ++i) {
            if (skip) {
                skip = false;
                continue;
            }
            const int32_t a_col = a_begin < a_end ? a.col_idxs[a_begin] : INT32_MAX;
            const int32_t b_col = b_begin < b_end ? lu.col_idxs[b_begin] : INT32_MAX;
            const int32_t col = min(a_col, b_col);
            if (Fill) {
                const double a_val = a_col == col ? a.vals[a_begin] : 0.0;
                const double lu_val = b_col == col ? lu.vals[b_begin] : 0.0;
                const double r_val = a_val - lu_val;
                // the matching entry of L + U
                int32_t lpu_col;
                double lpu_val;
                if (finished_l) {
                    const bool has = u_old_begin < u_old_end;
                    lpu_col = has ? u.col_idxs[u_old_begin] : INT32_MAX;
                    lpu_val = has ? u.vals[u_old_begin] : 0.0;
                } else {
                    lpu_col = l.col_idxs[l_old_begin];
                    lpu_val = l.vals[l_old_begin];
                }
                // the diagonal of U, the first entry of its row, for an entry below the diagonal
                const double diag = col < row ? u.vals[u.row_ptrs[col]] : 1.0;
                const double out_val = lpu_col == col ? lpu_val : r_val / diag;
                if (row >= col) {
                    l_new.col_idxs[l_new_nz] = col;
                    l_new.vals[l_new_nz] = row == col ? 1.0 : out_val;
                }
                if (row <= col) {
                    u_new.col_idxs[u_new_nz] = col;
                    u_new.vals[u_new_nz] = out_val;
                }
                if (finished_l) {
                    u_old_begin += lpu_col == col;
                } else {
                    l_old_begin += lpu_col == col;
                    finished_l = l_old_begin >= l_old_end;
                }
            }
            l_new_nz += row >= col;
            u_new_nz += row <= col;
            a_begin += a_col <= b_col;
            b_begin += b_col <= a_col;
            skip = a_col == b_col;
        }
        if (!Fill) {
            l_new.row_ptrs[row] = l_new_nz;
            u_new.row_ptrs[row] = u_new_nz;
        }
    }
}

// ---- compute_l_u_factors ---------------------------------------------------------------------------------
struct sweep_header {
    int64_t magic;  // sweep_magic once the analysis has succeeded
    int64_t n, l_nnz, u_nnz;
};

struct sweep_layout {
    size_t m_row_ptrs, m_cols, sums, flags, levels, levels_bytes, total;
};

sweep_layout make_sweep_layout(int64_t n, int64_t l_nnz, int64_t u_nnz)
{
    const size_t rows = static_cast<size_t>(n > 0 ? n : 1);
    const size_t entries = static_cast<size_t>(l_nnz + u_nnz > 0 ? l_nnz + u_nnz : 1);
    sweep_layout l{};
    size_t off = 256;
    l.m_row_ptrs = off; off += align256(sizeof(int32_t) * (rows + 1));
    l.m_cols = off; off += align256(sizeof(int32_t) * entries);
    l.sums = off; off += align256(sizeof(double) * entries);
    l.flags = off; off += 256;
    l.levels_bytes = make_layout(n).total;
    l.levels = off; off += l.levels_bytes;
    l.total = off;
    return l;
}

// The combined pattern: row i = the columns of L' without its last entry (the unit diagonal), then the row of U'.
// flags[0] != 0: a row pointer out of range, a row of L' that does not end in its diagonal, a row of U' that
// does not start with it, a column out of [0, n) or out of order.  Nothing is written for such a row, and no
// access leaves the arrays.
__global__ __launch_bounds__(block) void combine_rows_kernel(int32_t n, int32_t l_nnz, int32_t u_nnz,
                                                             const int32_t* __restrict__ l_row_ptrs,
                                                             const int32_t* __restrict__ l_col_idxs,
                                                             const int32_t* __restrict__ u_row_ptrs,
                                                             const int32_t* __restrict__ u_col_idxs,
                                                             int32_t* __restrict__ m_row_ptrs,
                                                             int32_t* __restrict__ m_cols, int32_t* __restrict__ flags)
{
    const int row = blockIdx.x * block + threadIdx.x;
    if (row >= n) return;
    const int lb = l_row_ptrs[row], le = l_row_ptrs[row + 1], ub = u_row_ptrs[row], ue = u_row_ptrs[row + 1];
    bool bad = lb < 0 || le <= lb || le > l_nnz || ub < 0 || ue <= ub || ue > u_nnz;
    if (row == 0 && (lb != 0 || ub != 0)) bad = true;
    if (row == n - 1 && (le != l_nnz || ue != u_nnz)) bad = true;
    const int64_t mb = static_cast<int64_t>(lb) - row + ub;
    if (mb < 0) bad = true;
    if (!bad) {
        int prev = -1;
        for (int k = lb; k < le; ++k) {
            const int col = l_col_idxs[k];
            if (col <= prev || col > row) bad = true;
            prev = col;
        }
        if (prev != row) bad = true;
        prev = row - 1;
        for (int k = ub; k < ue; ++k) {
            const int col = u_col_idxs[k];
            if (col <= prev || col >= n) bad = true;
            prev = col;
        }
        if (u_col_idxs[ub] != row) bad = true;
    }
    if (bad) {
        atomicOr(flags, 1);
        return;
    }
    m_row_ptrs[row] = static_cast<int32_t>(mb);
    if (row == n - 1) m_row_ptrs[n] = l_nnz - n + u_nnz;
    int at = static_cast<int32_t>(mb);
    for (int k = lb; k < le - 1; ++k) m_cols[at++] = l_col_idxs[k];
    for (int k = ub; k < ue; ++k) m_cols[at++] = u_col_idxs[k];
}

struct sweep_args {
    const int32_t* a_row_ptrs;
    const int32_t* a_col_idxs;
    const double* a_vals;
    const int32_t* l_row_ptrs;
    double* l_vals;
    const int32_t* u_row_ptrs;
    const int32_t* u_col_idxs;
    double* u_vals;
    const int32_t* m_row_ptrs;
    const int32_t* m_cols;
    double* sums;  // the running sums of a row too long for LDS
};

// a(row, col), 0.0 where A does not store it (:289-295)
__device__ __forceinline__ double a_value(const sweep_args& g, int a_begin, int a_end, int col)
{
    const int at = find_col(g.a_col_idxs, a_begin, a_end, col);
    return at >= 0 ? g.a_vals[at] : 0.0;
}

// One row of the sweep by a group of W lanes (t = my lane in the group).  w: the running sums of the combined
// row (len entries), entries [0, dpos) below the diagonal.
template <int W, bool InMemory, bool Coherent, class Meet>
__device__ __forceinline__ void sweep_row(int t, int row, const sweep_args& g, double* w, Meet meet)
{
    const int mb = g.m_row_ptrs[row];
    const int len = g.m_row_ptrs[row + 1] - mb;
    const int lb = g.l_row_ptrs[row];
    const int dpos = g.l_row_ptrs[row + 1] - 1 - lb;
    const int ub = g.u_row_ptrs[row];
    const int a_begin = g.a_row_ptrs[row], a_end = g.a_row_ptrs[row + 1];
    const int32_t* cols = g.m_cols + mb;
    for (int q = t; q < len; q += W) wst<InMemory>(w + q, 0.0);
    meet();
    for (int p = 0; p < dpos; ++p) {
        const int k = cols[p];
        const int uk = g.u_row_ptrs[k];  // u(k, k), the first entry of row k of U
        const double new_val = (a_value(g, a_begin, a_end, k) - wld<InMemory>(w + p)) / finished<Coherent>(g.u_vals + uk);
        // only this group touches the L values of its row
        const double l = std::isfinite(new_val) ? new_val : g.l_vals[lb + p];
        const int kend = g.u_row_ptrs[k + 1];
        for (int q = uk + 1 + t; q < kend; q += W) {
            const int r = find_col(cols, p + 1, len, g.u_col_idxs[q]);
            if (r >= 0) {
                const double prod = l * finished<Coherent>(g.u_vals + q);
                wst<InMemory>(w + r, wld<InMemory>(w + r) + prod);
            }
        }
        meet();
        // nobody reads entry p of the row any more
        if (t == 0) g.l_vals[lb + p] = l;
    }
    for (int q = dpos + t; q < len; q += W) {
        const double new_val = a_value(g, a_begin, a_end, cols[q]) - wld<InMemory>(w + q);
        if (std::isfinite(new_val)) g.u_vals[ub + (q - dpos)] = new_val;
    }
}

// the row policy of the frame (fact_levels.hpp): the combined row bins it; the sums of a row too long for LDS
// live in the workspace
struct sweep_rows {
    sweep_args g;
    static constexpr bool needs_products = false;
    __device__ __forceinline__ int length(int i) const { return g.m_row_ptrs[i + 1] - g.m_row_ptrs[i]; }
    __device__ __forceinline__ double* memory_row(int i) const { return g.sums + g.m_row_ptrs[i]; }
    template <int W, bool InMemory, bool Coherent, class Meet>
    __device__ __forceinline__ void row(int t, int i, double* w, double*, Meet meet) const
    {
        sweep_row<W, InMemory, Coherent>(t, i, g, w, meet);
    }
};

// ut_vals[q] = u(row, col) for the entry q of the CSC copy: col from the column pointers, row = ut_col_idxs[q]
__global__ __launch_bounds__(block) void refresh_transposed_kernel(int32_t n, int32_t u_nnz,
                                                                   const int32_t* __restrict__ u_row_ptrs,
                                                                   const int32_t* __restrict__ u_col_idxs,
                                                                   const double* __restrict__ u_vals,
                                                                   const int32_t* __restrict__ ut_row_ptrs,
                                                                   const int32_t* __restrict__ ut_col_idxs,
                                                                   double* __restrict__ ut_vals)
{
    for (int q = blockIdx.x * block + threadIdx.x; q < u_nnz; q += gridDim.x * block) {
        // the last column whose first entry is at or before q
        int lo = 0, hi = n;
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (ut_row_ptrs[mid] <= q) {
                lo = mid;
            } else {
                hi = mid;
            }
        }
        const int row = ut_col_idxs[q];
        if (row < 0 || row >= n) continue;
        const int at = find_col(u_col_idxs, u_row_ptrs[row], u_row_ptrs[row + 1], lo);
        if (at >= 0) ut_vals[q] = u_vals[at];
    }
}

bool bad_csr(int64_t nrows, int64_t nnz, const int32_t* row_ptrs, const int32_t* col_idxs, const double* vals)
{
    if (nrows > 0 && row_ptrs == nullptr) return true;
    return nnz > 0 && (col_idxs == nullptr || vals == nullptr);
}

}  // namespace
}  // namespace gkomi

using namespace gkomi;

extern "C" size_t gkomi_par_ilut_select_workspace_bytes(int64_t nnz)
{
    if (nnz < 0 || nnz > INT32_MAX) return 0;
    return carve_select(nnz).total;
}

extern "C" int gkomi_par_ilut_threshold_select_f64(gkomi_stream_t s, int64_t nnz, const double* vals, int64_t rank,
                                                   void* workspace, size_t workspace_bytes, double* host_threshold)
{
    if (nnz < 0 || host_threshold == nullptr) return GKOMI_EINVAL;
    if (rank < 0 || rank >= nnz || vals == nullptr) return GKOMI_EINVAL;
    if (nnz > INT32_MAX) return GKOMI_ENOTSUPPORTED;
    const select_ws w = carve_select(nnz);
    if (workspace == nullptr || workspace_bytes < w.total) return GKOMI_EWORKSPACE;
    hipStream_t stream = to_stream(s);
    char* ws = static_cast<char*>(workspace);
    uint64_t* keys_in = reinterpret_cast<uint64_t*>(ws + w.keys_in);
    uint64_t* keys_out = reinterpret_cast<uint64_t*>(ws + w.keys_out);
    hipLaunchKernelGGL(abs_keys_kernel, dim3(grid_for(nnz, block)), dim3(block), 0, stream, nnz, vals, keys_in);
    GKOMI_TRY(check_launch());
    // the sign bit is cleared: 63 key bits
    GKOMI_TRY(radix_sort_u64(stream, nnz, keys_in, keys_out, nullptr, nullptr, 63, ws + w.sort, w.sort_bytes));
    uint64_t bits = 0;
    GKOMI_TRY(static_cast<int>(hipMemcpyAsync(&bits, keys_out + rank, sizeof(bits), hipMemcpyDeviceToHost, stream)));
    GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
    std::memcpy(host_threshold, &bits, sizeof(bits));
    return GKOMI_SUCCESS;
}

extern "C" size_t gkomi_par_ilut_approx_workspace_bytes(void) { return approx_total; }

extern "C" int gkomi_par_ilut_threshold_approx_f64(gkomi_stream_t s, int64_t nnz, const double* vals, int64_t rank,
                                                   void* workspace, size_t workspace_bytes, double* host_threshold)
{
    if (nnz < 0 || rank < 0 || host_threshold == nullptr) return GKOMI_EINVAL;
    if (nnz > 0 && (vals == nullptr || rank >= nnz)) return GKOMI_EINVAL;
    if (nnz > INT32_MAX) return GKOMI_ENOTSUPPORTED;
    if (nnz == 0) {  // nothing to sample
        *host_threshold = 0.0;
        return GKOMI_SUCCESS;
    }
    if (workspace == nullptr || workspace_bytes < approx_total) return GKOMI_EWORKSPACE;
    hipStream_t stream = to_stream(s);
    char* ws = static_cast<char*>(workspace);
    double* splitters = reinterpret_cast<double*>(ws + approx_splitters);
    int32_t* histogram = reinterpret_cast<int32_t*>(ws + approx_histogram);
    const int32_t nnz32 = static_cast<int32_t>(nnz);
    hipLaunchKernelGGL(sample_splitters_kernel, dim3(1), dim3(sample_size), 0, stream, nnz32, vals, splitters, histogram);
    GKOMI_TRY(check_launch());
    hipLaunchKernelGGL(histogram_kernel, dim3(grid_for(nnz, block)), dim3(block), 0, stream, nnz32, vals, splitters,
                       histogram);
    GKOMI_TRY(check_launch());
    double host_splitters[bucket_count];
    int32_t host_histogram[bucket_count];
    GKOMI_TRY(static_cast<int>(hipMemcpyAsync(host_splitters, splitters, sizeof(double) * (bucket_count - 1),
                                              hipMemcpyDeviceToHost, stream)));
    GKOMI_TRY(static_cast<int>(hipMemcpyAsync(host_histogram, histogram, sizeof(host_histogram), hipMemcpyDeviceToHost, stream)));
    GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
    // prefix sums, then the bucket with prefix[bucket] <= rank < prefix[bucket + 1] (:240-247)
    int64_t prefix = 0;
    int bucket = bucket_count;
    for (int b = 0; b < bucket_count; ++b) {
        prefix += host_histogram[b];
        if (prefix > rank) {
            bucket = b;
            break;
        }
    }
    *host_threshold = bucket > 0 ? host_splitters[bucket - 1] : 0.0;
    return GKOMI_SUCCESS;
}

extern "C" size_t gkomi_par_ilut_filter_workspace_bytes(int64_t n)
{
    if (n < 0 || n > INT32_MAX - 1024) return 0;
    return row_scan_bytes(n);
}

extern "C" int gkomi_par_ilut_threshold_filter_f64_i32(gkomi_stream_t s, int64_t n, const int32_t* row_ptrs,
                                                       const int32_t* col_idxs, const double* vals, double threshold,
                                                       int32_t* new_row_ptrs, int32_t* new_col_idxs, double* new_vals,
                                                       int32_t* new_row_idxs, int64_t* host_new_nnz, void* workspace,
                                                       size_t workspace_bytes)
{
    if (n < 0 || host_new_nnz == nullptr || new_row_ptrs == nullptr) return GKOMI_EINVAL;
    if (n > 0 && row_ptrs == nullptr) return GKOMI_EINVAL;
    if ((new_col_idxs == nullptr) != (new_vals == nullptr)) return GKOMI_EINVAL;
    if (n > INT32_MAX - 1024) return GKOMI_ENOTSUPPORTED;
    const bool count = new_col_idxs == nullptr;
    if (count && new_row_idxs != nullptr) return GKOMI_EINVAL;
    hipStream_t stream = to_stream(s);
    if (n == 0) {
        if (!count) return GKOMI_SUCCESS;
        *host_new_nnz = 0;
        GKOMI_TRY(static_cast<int>(hipMemsetAsync(new_row_ptrs, 0, sizeof(int32_t), stream)));
        return static_cast<int>(hipStreamSynchronize(stream));
    }
    const int32_t n32 = static_cast<int32_t>(n);
    const dim3 grid(grid_for(n, block / wave_size));
    if (count) {
        if (workspace == nullptr || workspace_bytes < row_scan_bytes(n)) return GKOMI_EWORKSPACE;
        hipLaunchKernelGGL(filter_kernel<false>, grid, dim3(block), 0, stream, n32, row_ptrs, col_idxs, vals, threshold,
                           new_row_ptrs, static_cast<int32_t*>(nullptr), static_cast<double*>(nullptr),
                           static_cast<int32_t*>(nullptr));
        GKOMI_TRY(check_launch());
        return finish_row_ptrs(stream, n, new_row_ptrs, workspace, workspace_bytes, host_new_nnz);
    }
    if (*host_new_nnz < 0 || *host_new_nnz > INT32_MAX) return GKOMI_EINVAL;
    if (*host_new_nnz == 0) return GKOMI_SUCCESS;
    hipLaunchKernelGGL(filter_kernel<true>, grid, dim3(block), 0, stream, n32, row_ptrs, col_idxs, vals, threshold,
                       new_row_ptrs, new_col_idxs, new_vals, new_row_idxs);
    return check_launch();
}

extern "C" size_t gkomi_par_ilut_add_candidates_workspace_bytes(int64_t n)
{
    if (n < 0 || n > INT32_MAX - 1024) return 0;
    return row_scan_bytes(n);
}

extern "C" int gkomi_par_ilut_add_candidates_f64_i32(
    gkomi_stream_t s, int64_t n, const int32_t* lu_row_ptrs, const int32_t* lu_col_idxs, const double* lu_vals,
    const int32_t* a_row_ptrs, const int32_t* a_col_idxs, const double* a_vals, const int32_t* l_row_ptrs,
    const int32_t* l_col_idxs, const double* l_vals, const int32_t* u_row_ptrs, const int32_t* u_col_idxs,
    const double* u_vals, int32_t* l_new_row_ptrs, int32_t* l_new_col_idxs, double* l_new_vals,
    int32_t* u_new_row_ptrs, int32_t* u_new_col_idxs, double* u_new_vals, int64_t* host_l_new_nnz,
    int64_t* host_u_new_nnz, void* workspace, size_t workspace_bytes)
{
    if (n < 0 || host_l_new_nnz == nullptr || host_u_new_nnz == nullptr) return GKOMI_EINVAL;
    if (l_new_row_ptrs == nullptr || u_new_row_ptrs == nullptr) return GKOMI_EINVAL;
    if (n > 0 && (lu_row_ptrs == nullptr || a_row_ptrs == nullptr || l_row_ptrs == nullptr || u_row_ptrs == nullptr)) return GKOMI_EINVAL;
    const bool count = l_new_col_idxs == nullptr;
    if ((l_new_vals == nullptr) != count || (u_new_col_idxs == nullptr) != count || (u_new_vals == nullptr) != count) return GKOMI_EINVAL;
    if (n > INT32_MAX - 1024) return GKOMI_ENOTSUPPORTED;
    hipStream_t stream = to_stream(s);
    if (n == 0) {
        if (!count) return GKOMI_SUCCESS;
        *host_l_new_nnz = *host_u_new_nnz = 0;
        GKOMI_TRY(static_cast<int>(hipMemsetAsync(l_new_row_ptrs, 0, sizeof(int32_t), stream)));
        GKOMI_TRY(static_cast<int>(hipMemsetAsync(u_new_row_ptrs, 0, sizeof(int32_t), stream)));
        return static_cast<int>(hipStreamSynchronize(stream));
    }
    const int32_t n32 = static_cast<int32_t>(n);
    const csr_in lu{lu_row_ptrs, lu_col_idxs, lu_vals}, a{a_row_ptrs, a_col_idxs, a_vals};
    const csr_in l{l_row_ptrs, l_col_idxs, l_vals}, u{u_row_ptrs, u_col_idxs, u_vals};
    const csr_out l_new{l_new_row_ptrs, l_new_col_idxs, l_new_vals}, u_new{u_new_row_ptrs, u_new_col_idxs, u_new_vals};
    if (count) {
        if (workspace == nullptr || workspace_bytes < row_scan_bytes(n)) return GKOMI_EWORKSPACE;
        hipLaunchKernelGGL(add_candidates_kernel<false>, dim3(grid_for(n, block)), dim3(block), 0, stream, n32, lu, a, l,
                           u, l_new, u_new);
        GKOMI_TRY(check_launch());
        GKOMI_TRY(finish_row_ptrs(stream, n, l_new_row_ptrs, workspace, workspace_bytes, host_l_new_nnz));
        return finish_row_ptrs(stream, n, u_new_row_ptrs, workspace, workspace_bytes, host_u_new_nnz);
    }
    if (*host_l_new_nnz < 0 || *host_l_new_nnz > INT32_MAX || *host_u_new_nnz < 0 || *host_u_new_nnz > INT32_MAX) return GKOMI_EINVAL;
    if (l_col_idxs == nullptr || l_vals == nullptr || u_col_idxs == nullptr || u_vals == nullptr) return GKOMI_EINVAL;
    hipLaunchKernelGGL(add_candidates_kernel<true>, dim3(grid_for(n, block)), dim3(block), 0, stream, n32, lu, a, l, u,
                       l_new, u_new);
    return check_launch();
}

extern "C" void gkomi_par_ilut_tuning(int64_t* host_out) { fill_tuning(host_out); }

extern "C" size_t gkomi_par_ilut_sweep_workspace_bytes(int64_t n, int64_t l_nnz, int64_t u_nnz)
{
    if (n < 0 || n > INT32_MAX - 1024 || l_nnz < 0 || u_nnz < 0 || l_nnz + u_nnz > INT32_MAX) return 0;
    return make_sweep_layout(n, l_nnz, u_nnz).total;
}

extern "C" int gkomi_par_ilut_analyse_i32(gkomi_stream_t s, int64_t n, int64_t l_nnz, const int32_t* l_row_ptrs,
                                          const int32_t* l_col_idxs, int64_t u_nnz, const int32_t* u_row_ptrs,
                                          const int32_t* u_col_idxs, void* workspace, size_t workspace_bytes,
                                          int64_t* host_out)
{
    if (n < 0 || l_nnz < 0 || u_nnz < 0 || host_out == nullptr) return GKOMI_EINVAL;
    // every row of L' and of U' stores its diagonal
    if (l_nnz < n || u_nnz < n) return GKOMI_EINVAL;
    if (n > 0 && (l_row_ptrs == nullptr || l_col_idxs == nullptr || u_row_ptrs == nullptr || u_col_idxs == nullptr)) return GKOMI_EINVAL;
    if (n > INT32_MAX - 1024 || l_nnz + u_nnz > INT32_MAX) return GKOMI_ENOTSUPPORTED;
    if (n == 0 && (l_nnz != 0 || u_nnz != 0)) return GKOMI_EINVAL;
    const sweep_layout l = make_sweep_layout(n, l_nnz, u_nnz);
    if (workspace == nullptr || workspace_bytes < l.total) return GKOMI_EWORKSPACE;
    hipStream_t stream = to_stream(s);
    char* ws = static_cast<char*>(workspace);
    for (int i = 0; i < 6; ++i) host_out[i] = 0;
    // the workspace is not valid until the end of a successful analysis
    GKOMI_TRY(static_cast<int>(hipMemsetAsync(ws, 0, 256, stream)));
    int32_t* m_row_ptrs = reinterpret_cast<int32_t*>(ws + l.m_row_ptrs);
    int32_t* m_cols = reinterpret_cast<int32_t*>(ws + l.m_cols);
    if (n > 0) {
        int32_t* flags = reinterpret_cast<int32_t*>(ws + l.flags);
        GKOMI_TRY(static_cast<int>(hipMemsetAsync(flags, 0, 256, stream)));
        hipLaunchKernelGGL(combine_rows_kernel, dim3(static_cast<unsigned>(ceildiv(n, block))), dim3(block), 0, stream,
                           static_cast<int32_t>(n), static_cast<int32_t>(l_nnz), static_cast<int32_t>(u_nnz), l_row_ptrs,
                           l_col_idxs, u_row_ptrs, u_col_idxs, m_row_ptrs, m_cols, flags);
        GKOMI_TRY(check_launch());
        int32_t bad = 0;
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(&bad, flags, sizeof(bad), hipMemcpyDeviceToHost, stream)));
        GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
        if (bad != 0) return GKOMI_EINVAL;
    }
    GKOMI_TRY(gkomi_ilu_analyse_i32(s, n, m_row_ptrs, m_cols, ws + l.levels, l.levels_bytes, host_out));
    sweep_header h{sweep_magic, n, l_nnz, u_nnz};
    GKOMI_TRY(static_cast<int>(hipMemcpyAsync(ws, &h, sizeof(h), hipMemcpyHostToDevice, stream)));
    return static_cast<int>(hipStreamSynchronize(stream));
}

extern "C" int gkomi_par_ilut_compute_l_u_factors_f64_i32(
    gkomi_stream_t s, int64_t n, const int32_t* a_row_ptrs, const int32_t* a_col_idxs, const double* a_vals,
    int64_t l_nnz, const int32_t* l_row_ptrs, const int32_t* l_col_idxs, double* l_vals, int64_t u_nnz,
    const int32_t* u_row_ptrs, const int32_t* u_col_idxs, double* u_vals, const int32_t* ut_row_ptrs,
    const int32_t* ut_col_idxs, double* ut_vals, const void* analysis_workspace, size_t workspace_bytes)
{
    if (n < 0 || l_nnz < n || u_nnz < n) return GKOMI_EINVAL;
    if (n > 0 && (a_row_ptrs == nullptr || l_row_ptrs == nullptr || l_col_idxs == nullptr || l_vals == nullptr ||
                  u_row_ptrs == nullptr || u_col_idxs == nullptr || u_vals == nullptr)) {
        return GKOMI_EINVAL;
    }
    // the CSC copy of U: all of it or none
    const bool refresh = ut_vals != nullptr;
    if ((ut_row_ptrs != nullptr) != refresh || (ut_col_idxs != nullptr) != refresh) return GKOMI_EINVAL;
    if (n > INT32_MAX - 1024 || l_nnz + u_nnz > INT32_MAX) return GKOMI_ENOTSUPPORTED;
    const sweep_layout l = make_sweep_layout(n, l_nnz, u_nnz);
    if (analysis_workspace == nullptr || workspace_bytes < l.total) return GKOMI_EWORKSPACE;
    hipStream_t stream = to_stream(s);
    const char* ws = static_cast<const char*>(analysis_workspace);
    sweep_header sh{};
    schedule sched;
    GKOMI_TRY(load_schedule(stream, ws + l.levels, n, &sched, ws, &sh, sizeof(sh)));
    // no analysis, a failed one, or one of other factors
    if (sh.magic != sweep_magic || sh.n != n || sh.l_nnz != l_nnz || sh.u_nnz != u_nnz) return GKOMI_EINVAL;
    if (n == 0) return GKOMI_SUCCESS;
    // the sums of the rows too long for LDS live in the workspace, which the caller hands over as const: the
    // analysis owns the pattern, the numeric call its scratch
    char* scratch = const_cast<char*>(ws);
    const sweep_args g{a_row_ptrs, a_col_idxs, a_vals, l_row_ptrs, l_vals, u_row_ptrs, u_col_idxs, u_vals,
                       reinterpret_cast<const int32_t*>(ws + l.m_row_ptrs), reinterpret_cast<const int32_t*>(ws + l.m_cols),
                       reinterpret_cast<double*>(scratch + l.sums)};
    GKOMI_TRY(launch_schedule<sweep_rows>(stream, sched, g));
    if (refresh) {
        hipLaunchKernelGGL(refresh_transposed_kernel, dim3(grid_for(u_nnz, block)), dim3(block), 0, stream,
                           static_cast<int32_t>(n), static_cast<int32_t>(u_nnz), u_row_ptrs, u_col_idxs, u_vals, ut_row_ptrs,
                           ut_col_idxs, ut_vals);
        GKOMI_TRY(check_launch());
    }
    return GKOMI_SUCCESS;
}
