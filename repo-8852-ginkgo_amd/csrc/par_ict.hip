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
// Scheduling: as in ilu.hip.  No kernel waits on another workgroup: no flags, no spins, no device-wide
// meetings.  A wide level is one launch per row-length bin it holds rows of, a run of narrow levels one
// launch of one workgroup.  All boundaries (gkomi_par_ict_tuning) are tuning constants; none has been
// measured.
#include "common.hpp"

#include <cmath>
#include <vector>

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

// one row by a whole workgroup: in LDS when it fits, in memory otherwise.  image: bin_lds doubles.
template <bool Coherent>
__device__ __forceinline__ void ict_block_row(int row, const ict_args& g, double* image, double* products)
{
    const int begin = g.l_row_ptrs[row];
    if (g.l_row_ptrs[row + 1] - begin <= bin_lds) {
        ict_row<fact_block, false, Coherent>(threadIdx.x, row, g, image, products, block_meet{});
    } else {
        ict_row<fact_block, true, Coherent>(threadIdx.x, row, g, g.l_vals + begin, products, block_meet{});
    }
}

__device__ __forceinline__ int row_bin(const ict_args& g, int row)
{
    return bin_of(g.l_row_ptrs[row + 1] - g.l_row_ptrs[row]);
}

// (a) one wide level, its rows of bin Bin (at most Cap entries): a group of W lanes per row, grid-stride over
// perm[first, last)
template <int W, int Cap, int Bin>
__global__ __launch_bounds__(fact_block) void ict_level_kernel(ict_args g, const int32_t* __restrict__ perm, int first,
                                                              int last)
{
    constexpr int groups = fact_block / W;
    __shared__ double image[groups * Cap];
    __shared__ double products[fact_block];
    const int grp = threadIdx.x / W, t = threadIdx.x % W;
    for (int pos = first + blockIdx.x * groups + grp; pos < last; pos += gridDim.x * groups) {
        const int row = perm[pos];
        if (row_bin(g, row) != Bin) continue;  // the same answer in every lane of the group
        ict_row<W, false, false>(t, row, g, image + grp * Cap, products + grp * W, wave_meet{});
        wave_meet{}();  // the image is loaded again
    }
}

// (a) the rows longer than bin_wave of one wide level: a workgroup per row
__global__ __launch_bounds__(fact_block) void ict_level_block_kernel(ict_args g, const int32_t* __restrict__ perm,
                                                                    int first, int last)
{
    __shared__ double image[bin_lds];
    __shared__ double products[fact_block];
    for (int pos = first + blockIdx.x; pos < last; pos += gridDim.x) {
        const int row = perm[pos];
        if (row_bin(g, row) != 2) continue;  // the same answer in the whole workgroup
        ict_block_row<false>(row, g, image, products);
        __syncthreads();
    }
}

// (b) ONE workgroup walks the narrow levels [first_level, last_level): a wave per row of at most bin_wave
// entries, then the workgroup per longer row, __syncthreads between levels.  What a level wrote is read by the
// next through agent-scope loads after a release fence.
__global__ __launch_bounds__(fact_block) void ict_run_kernel(ict_args g, const int32_t* __restrict__ perm,
                                                            const int32_t* __restrict__ level_start,
                                                            const int32_t* __restrict__ level_longest, int first_level,
                                                            int last_level)
{
    constexpr int waves = fact_block / wave_size;
    static_assert(waves * bin_wave >= bin_lds, "the images of the waves hold the image of the workgroup");
    __shared__ double image[waves * bin_wave];
    __shared__ double products[fact_block];
    const int wave = threadIdx.x / wave_size, lane = threadIdx.x % wave_size;
    for (int lvl = first_level; lvl < last_level; ++lvl) {
        const int first = level_start[lvl], last = level_start[lvl + 1];
        // the rows of at most bin_wave entries: a wave each
        for (int pos = first + wave; pos < last; pos += waves) {
            const int row = perm[pos];
            if (row_bin(g, row) == 2) continue;
            ict_row<wave_size, false, true>(lane, row, g, image + wave * bin_wave, products + wave * wave_size, wave_meet{});
            wave_meet{}();
        }
        // the longer ones, if the level has any: the workgroup, one after the other (the images are shared)
        if (level_longest[lvl] > bin_wave) {
            __syncthreads();
            for (int pos = first; pos < last; ++pos) {
                const int row = perm[pos];
                if (row_bin(g, row) != 2) continue;
                ict_block_row<true>(row, g, image, products);
                __syncthreads();
            }
        }
        __threadfence();
        __syncthreads();
    }
}

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

extern "C" void gkomi_par_ict_tuning(int64_t* host_out)
{
    if (host_out == nullptr) return;
    host_out[0] = bin_short;
    host_out[1] = bin_wave;
    host_out[2] = bin_lds;
    host_out[3] = narrow_level_rows;
}

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
    analysis_header h{};
    GKOMI_TRY(static_cast<int>(hipMemcpyAsync(&ih, ws, sizeof(ih), hipMemcpyDeviceToHost, stream)));
    GKOMI_TRY(static_cast<int>(hipMemcpyAsync(&h, ws + l.levels, sizeof(h), hipMemcpyDeviceToHost, stream)));
    GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
    // no analysis, a failed one, or one of another factor
    if (ih.magic != ict_magic || ih.n != n || ih.l_nnz != l_nnz) return GKOMI_EINVAL;
    if (h.magic != ws_magic || h.n != n || h.nnz != l_nnz || h.nsegments < 0 || h.nsegments > n) return GKOMI_EINVAL;
    if (n == 0) return GKOMI_SUCCESS;
    const analysis_layout al = make_layout(n);
    const char* lws = ws + l.levels;
    std::vector<segment> segs(static_cast<size_t>(h.nsegments));
    GKOMI_TRY(static_cast<int>(hipMemcpyAsync(segs.data(), lws + al.segments, sizeof(segment) * segs.size(),
                                              hipMemcpyDeviceToHost, stream)));
    GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
    const int32_t* perm = reinterpret_cast<const int32_t*>(lws + al.perm);
    const int32_t* level_start = reinterpret_cast<const int32_t*>(lws + al.level_start);
    const int32_t* level_longest = reinterpret_cast<const int32_t*>(lws + al.level_longest);
    const ict_args g{a_row_ptrs, a_col_idxs, a_vals, l_row_ptrs, l_col_idxs, l_vals};
    for (const segment& sg : segs) {
        if (sg.kind == 1) {
            hipLaunchKernelGGL(ict_run_kernel, dim3(1), dim3(fact_block), 0, stream, g, perm, level_start, level_longest,
                               sg.first, sg.last);
            continue;
        }
        const int64_t rows = sg.last - sg.first;
        // one launch per bin the level holds rows of
        if (sg.bins & 1) {
            hipLaunchKernelGGL((ict_level_kernel<short_width, bin_short, 0>),
                               dim3(grid_for(rows, fact_block / short_width, max_level_grid)), dim3(fact_block), 0, stream, g,
                               perm, sg.first, sg.last);
        }
        if (sg.bins & 2) {
            hipLaunchKernelGGL((ict_level_kernel<wave_size, bin_wave, 1>),
                               dim3(grid_for(rows, fact_block / wave_size, max_level_grid)), dim3(fact_block), 0, stream, g,
                               perm, sg.first, sg.last);
        }
        if (sg.bins & 4) {
            hipLaunchKernelGGL(ict_level_block_kernel, dim3(grid_for(rows, 1, max_level_grid)), dim3(fact_block), 0, stream, g,
                               perm, sg.first, sg.last);
        }
    }
    return check_launch();
}
