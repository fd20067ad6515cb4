// ParICT: factorization::ParIct (core/factorization/par_ict.cpp:174-292), the two kernels of
// reference/factorization/par_ict_kernels.cpp with the results of the REFERENCE executor, bit for bit:
// compute_factor (:65-121) and add_candidates (:127-199 over reference/components/csr_spgeam.hpp:58-104).
// <double, int32>.  Selection and filter are those of par_ilut.hip.  No vendor library.
//
// The sweep.  The reference executor's compute_factor is ONE sequential in-place sweep in row order.  Entry
// (row, col) reads l(row, k) and l(col, k) for k < col and the diagonal l(col, col), the last entry of row
// col, and every one of them has been rewritten earlier in the same sweep (or kept, where the new value was
// not finite): the result is determined by the pattern, and any schedule that finishes row col before a row
// that stores l(row, col) reproduces it.  That is the lower-triangular level structure of L', which the
// analysis of ilu.hip (gkomi_ilu_analyse_i32) computes; it runs on the pattern of L' itself, whose rows are
// sorted and end in their diagonal, so its row lengths -- and with them its bins -- are those of the working
// row of the sweep.
//
// Bits.  Every sum starts at +0.0 and receives the products l(row, k) * l(col, k) of the k < col that both
// rows store, in ascending k, one rounding per product and per sum (:91-108); then a - sum (a = 0.0 where A
// does not store the entry, A's row searched by lower_bound), then one IEEE square root on the diagonal or
// one IEEE quotient by l(col, col).  A result that is not finite leaves the old value in place, and the old
// value is what later entries read.  As in ic_row (ilu.hip) the lanes of a group form the products of one
// sum side by side over the lower entries of row col and every lane adds them one after the other; an entry
// of row col that this row does not store contributes +0.0, which leaves every bit alone because a sum that
// starts at +0.0 is never -0.0.  The library is built with -ffp-contract=off.
//
// Scheduling: as in fact_levels.hpp, whose frame runs ict_row over the levels of L' (boundaries:
// gkomi_par_ict_tuning).
#include "common.hpp"

#include <cmath>

#include "fact_levels.hpp"
#include "internal.hpp"
#include "sort_scan.hpp"

namespace gkomi {
namespace {

using namespace fact;

constexpr int block = 256;

constexpr int64_t ict_magic = 0x7069637473777070ll;

// ---- add_candidates (:127-199): the merge of row i of A and of L L^T, one lane per row ------------------
template <bool Fill>
__global__ __launch_bounds__(block) void ict_add_candidates_kernel(int32_t n, csr_in llh, csr_in a, csr_in l,
                                                                   csr_out l_new)
{
    for (int row = blockIdx.x * block + threadIdx.x; row < n; row += gridDim.x * block) {
        int a_begin = a.row_ptrs[row], b_begin = llh.row_ptrs[row];
        const int a_end = a.row_ptrs[row + 1], b_end = llh.row_ptrs[row + 1];
        const int64_t total_size = static_cast<int64_t>(a_end - a_begin) + (b_end - b_begin);
        int l_new_nz = 0, l_old_begin = 0, l_old_end = 0;
        if (Fill) {
            l_new_nz = l_new.row_ptrs[row];
            l_old_begin = l.row_ptrs[row];
            l_old_end = l.row_ptrs[row + 1];
        }
        bool skip = false;
        for (int64_t i = 0; i < total_size; ++i) {
            if (skip) {
                skip = false;
                continue;
            }
            const int32_t a_col = a_begin < a_end ? a.col_idxs[a_begin] : INT32_MAX;
            const int32_t b_col = b_begin < b_end ? llh.col_idxs[b_begin] : INT32_MAX;
            const int32_t col = min(a_col, b_col);
            // both rows ascend: nothing at or below the diagonal follows an entry above it
            if (col > row) break;
            if (Fill) {
                const double a_val = a_col == col ? a.vals[a_begin] : 0.0;
                const double llh_val = b_col == col ? llh.vals[b_begin] : 0.0;
                const double r_val = a_val - llh_val;
                // the matching entry of L
                const bool has = l_old_begin < l_old_end;
                const int32_t l_col = has ? l.col_idxs[l_old_begin] : INT32_MAX;
                const double l_val = has ? l.vals[l_old_begin] : 0.0;
                // the diagonal of L, the last entry of row col
                const int dq = l.row_ptrs[col + 1] - 1;
                const double diag = dq >= 0 ? l.vals[dq] : 0.0;
                l_new.col_idxs[l_new_nz] = col;
                l_new.vals[l_new_nz] = l_col == col ? l_val : r_val / diag;
                l_old_begin += l_col == col;
            }
            ++l_new_nz;
            a_begin += a_col <= b_col;
            b_begin += b_col <= a_col;
            skip = a_col == b_col;
        }
        if (!Fill) l_new.row_ptrs[row] = l_new_nz;
    }
}

// ---- compute_factor ---------------------------------------------------------------------------------------
struct ict_header {
    int64_t magic;  // ict_magic once the analysis has succeeded
    int64_t n, l_nnz;
};

struct ict_layout {
    size_t flags, levels, levels_bytes, total;
};

ict_layout make_ict_layout(int64_t n)
{
    ict_layout l{};
    size_t off = 256;
    l.flags = off; off += 256;
    l.levels_bytes = make_layout(n).total;
    l.levels = off; off += l.levels_bytes;
    l.total = off;
    return l;
}

// flags[0] != 0: a row pointer out of range, a row that is not strictly ascending, leaves [0, row] or does
// not end in its diagonal.  No access leaves the arrays.
__global__ __launch_bounds__(block) void ict_check_rows_kernel(int32_t n, int32_t l_nnz,
                                                               const int32_t* __restrict__ l_row_ptrs,
                                                               const int32_t* __restrict__ l_col_idxs,
                                                               int32_t* __restrict__ flags)
{
    const int row = blockIdx.x * block + threadIdx.x;
    if (row >= n) return;
    const int lb = l_row_ptrs[row], le = l_row_ptrs[row + 1];
    bool bad = lb < 0 || le <= lb || le > l_nnz;
    if (row == 0 && lb != 0) bad = true;
    if (row == n - 1 && le != l_nnz) bad = true;
    if (!bad) {
        int prev = -1;
        for (int k = lb; k < le; ++k) {
            const int col = l_col_idxs[k];
            if (col <= prev || col > row) bad = true;
            prev = col;
        }
        if (prev != row) bad = true;
    }
    if (bad) atomicOr(flags, 1);
}

struct ict_args {
    const int32_t* a_row_ptrs;
    const int32_t* a_col_idxs;
    const double* a_vals;
    const int32_t* l_row_ptrs;
    const int32_t* l_col_idxs;
    double* l_vals;
};

// compute_factor of one row by a group of W lanes (t = my lane in the group).  w: the working row, the current
// values of l(row, :) (len entries, the last one the diagonal); products: W doubles of the group.
template <int W, bool InMemory, bool Coherent, class Meet>
__device__ __forceinline__ void ict_row(int t, int row, const ict_args& g, double* w, double* products, Meet meet)
{
    const int begin = g.l_row_ptrs[row];
    const int dpos = g.l_row_ptrs[row + 1] - 1 - begin;
    const int32_t* cols = g.l_col_idxs + begin;
    const int a_begin = g.a_row_ptrs[row], a_end = g.a_row_ptrs[row + 1];
    if (!InMemory) {
        for (int q = t; q <= dpos; q += W) w[q] = g.l_vals[begin + q];
        meet();
    }
    for (int p = 0; p <= dpos; ++p) {
        const int j = cols[p];
        const bool is_diag = p == dpos;
        // a(row, j), 0.0 where A does not store it (:83-89)
        const int at = find_col(g.a_col_idxs, a_begin, a_end, j);
        const double a = at >= 0 ? g.a_vals[at] : 0.0;
        // the entries of row j before its diagonal; for the diagonal they are this row's own, in the working row
        const int jb = g.l_row_ptrs[j];
        const int jd = is_diag ? begin + dpos : g.l_row_ptrs[j + 1] - 1;
        double sum = 0.0;
        for (int base = jb; base < jd; base += W) {
            const int q = base + t;
            double prod = 0.0;
            if (q < jd) {
                if (is_diag) {
                    const double v = wld<InMemory>(w + (q - begin));
                    prod = v * v;
                } else {
                    const int r = find_col(cols, 0, p, g.l_col_idxs[q]);
                    if (r >= 0) prod = wld<InMemory>(w + r) * finished<Coherent>(g.l_vals + q);
                }
            }
            products[t] = prod;
            meet();
            const int m = jd - base < W ? jd - base : W;
            for (int s = 0; s < m; ++s) sum += products[s];
            meet();
        }
        const double diff = a - sum;
        const double new_val = is_diag ? sqrt(diff) : diff / finished<Coherent>(g.l_vals + jd);
        // a value that is not finite leaves the old one, which is what the entries after it read (:116-118)
        if (t == 0 && std::isfinite(new_val)) wst<InMemory>(w + p, new_val);
        meet();
    }
    if (!InMemory) {
        for (int q = t; q <= dpos; q += W) g.l_vals[begin + q] = w[q];
    }
}

// the row policy of the frame (fact_levels.hpp): the row of L' bins it; a row too long for LDS is swept in place
struct ict_rows {
    ict_args g;
    static constexpr bool needs_products = true;
    __device__ __forceinline__ int length(int i) const { return g.l_row_ptrs[i + 1] - g.l_row_ptrs[i]; }
    __device__ __forceinline__ double* memory_row(int i) const { return g.l_vals + g.l_row_ptrs[i]; }
    template <int W, bool InMemory, bool Coherent, class Meet>
    __device__ __forceinline__ void row(int t, int i, double* w, double* products, Meet meet) const
    {
        ict_row<W, InMemory, Coherent>(t, i, g, w, products, meet);
    }
};

}  // namespace
}  // namespace gkomi

using namespace gkomi;

extern "C" size_t gkomi_par_ict_add_candidates_workspace_bytes(int64_t n)
{
    if (n < 0 || n > INT32_MAX - 1024) return 0;
    return row_scan_bytes(n);
}

extern "C" int gkomi_par_ict_add_candidates_f64_i32(gkomi_stream_t s, int64_t n, const int32_t* llh_row_ptrs,
                                                    const int32_t* llh_col_idxs, const double* llh_vals,
                                                    const int32_t* a_row_ptrs, const int32_t* a_col_idxs,
                                                    const double* a_vals, const int32_t* l_row_ptrs,
                                                    const int32_t* l_col_idxs, const double* l_vals,
                                                    int32_t* l_new_row_ptrs, int32_t* l_new_col_idxs, double* l_new_vals,
                                                    int64_t* host_l_new_nnz, void* workspace, size_t workspace_bytes)
{
    if (n < 0 || host_l_new_nnz == nullptr || l_new_row_ptrs == nullptr) return GKOMI_EINVAL;
    if (n > 0 && (llh_row_ptrs == nullptr || a_row_ptrs == nullptr || l_row_ptrs == nullptr)) return GKOMI_EINVAL;
    const bool count = l_new_col_idxs == nullptr;
    if ((l_new_vals == nullptr) != count) return GKOMI_EINVAL;
    if (n > INT32_MAX - 1024) return GKOMI_ENOTSUPPORTED;
    hipStream_t stream = to_stream(s);
    if (n == 0) {
        if (!count) return GKOMI_SUCCESS;
        *host_l_new_nnz = 0;
        GKOMI_TRY(static_cast<int>(hipMemsetAsync(l_new_row_ptrs, 0, sizeof(int32_t), stream)));
        return static_cast<int>(hipStreamSynchronize(stream));
    }
    const int32_t n32 = static_cast<int32_t>(n);
    const csr_in llh{llh_row_ptrs, llh_col_idxs, llh_vals}, a{a_row_ptrs, a_col_idxs, a_vals};
    const csr_in l{l_row_ptrs, l_col_idxs, l_vals};
    const csr_out l_new{l_new_row_ptrs, l_new_col_idxs, l_new_vals};
    if (count) {
        if (workspace == nullptr || workspace_bytes < row_scan_bytes(n)) return GKOMI_EWORKSPACE;
        hipLaunchKernelGGL(ict_add_candidates_kernel<false>, dim3(grid_for(n, block)), dim3(block), 0, stream, n32, llh, a,
                           l, l_new);
        GKOMI_TRY(check_launch());
        return finish_row_ptrs(stream, n, l_new_row_ptrs, workspace, workspace_bytes, host_l_new_nnz);
    }
    if (*host_l_new_nnz < 0 || *host_l_new_nnz > INT32_MAX) return GKOMI_EINVAL;
    if (l_col_idxs == nullptr || l_vals == nullptr) return GKOMI_EINVAL;
    hipLaunchKernelGGL(ict_add_candidates_kernel<true>, dim3(grid_for(n, block)), dim3(block), 0, stream, n32, llh, a, l,
                       l_new);
    return check_launch();
}

extern "C" void gkomi_par_ict_tuning(int64_t* host_out) { fill_tuning(host_out); }

extern "C" size_t gkomi_par_ict_sweep_workspace_bytes(int64_t n, int64_t l_nnz)
{
    if (n < 0 || n > INT32_MAX - 1024 || l_nnz < 0 || l_nnz > INT32_MAX) return 0;
    return make_ict_layout(n).total;
}

extern "C" int gkomi_par_ict_analyse_i32(gkomi_stream_t s, int64_t n, int64_t l_nnz, const int32_t* l_row_ptrs,
                                         const int32_t* l_col_idxs, void* workspace, size_t workspace_bytes,
                                         int64_t* host_out)
{
    if (n < 0 || l_nnz < 0 || host_out == nullptr) return GKOMI_EINVAL;
    // every row of L' stores its diagonal
    if (l_nnz < n) return GKOMI_EINVAL;
    if (n > 0 && (l_row_ptrs == nullptr || l_col_idxs == nullptr)) return GKOMI_EINVAL;
    if (n > INT32_MAX - 1024 || l_nnz > INT32_MAX) return GKOMI_ENOTSUPPORTED;
    if (n == 0 && l_nnz != 0) return GKOMI_EINVAL;
    const ict_layout l = make_ict_layout(n);
    if (workspace == nullptr || workspace_bytes < l.total) return GKOMI_EWORKSPACE;
    hipStream_t stream = to_stream(s);
    char* ws = static_cast<char*>(workspace);
    for (int i = 0; i < 6; ++i) host_out[i] = 0;
    // the workspace is not valid until the end of a successful analysis
    GKOMI_TRY(static_cast<int>(hipMemsetAsync(ws, 0, 256, stream)));
    if (n > 0) {
        int32_t* flags = reinterpret_cast<int32_t*>(ws + l.flags);
        GKOMI_TRY(static_cast<int>(hipMemsetAsync(flags, 0, 256, stream)));
        hipLaunchKernelGGL(ict_check_rows_kernel, dim3(static_cast<unsigned>(ceildiv(n, block))), dim3(block), 0, stream,
                           static_cast<int32_t>(n), static_cast<int32_t>(l_nnz), l_row_ptrs, l_col_idxs, flags);
        GKOMI_TRY(check_launch());
        int32_t bad = 0;
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(&bad, flags, sizeof(bad), hipMemcpyDeviceToHost, stream)));
        GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
        if (bad != 0) return GKOMI_EINVAL;
    }
    GKOMI_TRY(gkomi_ilu_analyse_i32(s, n, l_row_ptrs, l_col_idxs, ws + l.levels, l.levels_bytes, host_out));
    ict_header h{ict_magic, n, l_nnz};
    GKOMI_TRY(static_cast<int>(hipMemcpyAsync(ws, &h, sizeof(h), hipMemcpyHostToDevice, stream)));
    return static_cast<int>(hipStreamSynchronize(stream));
}

extern "C" int gkomi_par_ict_compute_factor_f64_i32(gkomi_stream_t s, int64_t n, const int32_t* a_row_ptrs,
                                                    const int32_t* a_col_idxs, const double* a_vals, int64_t l_nnz,
                                                    const int32_t* l_row_ptrs, const int32_t* l_col_idxs, double* l_vals,
                                                    const void* analysis_workspace, size_t workspace_bytes)
{
    if (n < 0 || l_nnz < n) return GKOMI_EINVAL;
    if (n > 0 && (a_row_ptrs == nullptr || l_row_ptrs == nullptr || l_col_idxs == nullptr || l_vals == nullptr)) {
        return GKOMI_EINVAL;
    }
    if (n > INT32_MAX - 1024 || l_nnz > INT32_MAX) return GKOMI_ENOTSUPPORTED;
    const ict_layout l = make_ict_layout(n);
    if (analysis_workspace == nullptr || workspace_bytes < l.total) return GKOMI_EWORKSPACE;
    hipStream_t stream = to_stream(s);
    const char* ws = static_cast<const char*>(analysis_workspace);
    ict_header ih{};
    schedule sched;
    GKOMI_TRY(load_schedule(stream, ws + l.levels, n, &sched, ws, &ih, sizeof(ih)));
    // no analysis, a failed one, or one of another factor
    if (ih.magic != ict_magic || ih.n != n || ih.l_nnz != l_nnz || sched.header.nnz != l_nnz) return GKOMI_EINVAL;
    if (n == 0) return GKOMI_SUCCESS;
    return launch_schedule<ict_rows>(stream, sched, ict_args{a_row_ptrs, a_col_idxs, a_vals, l_row_ptrs, l_col_idxs, l_vals});
}
