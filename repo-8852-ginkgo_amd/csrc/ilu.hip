// Exact ILU(0) and IC(0): factorization::Ilu / factorization::Ic
// (core/factorization/ilu.cpp:67-124 -> reference/factorization/ilu_kernels.cpp:56-97 compute_lu;
//  core/factorization/ic.cpp:67-120 -> reference/factorization/ic_kernels.cpp:53-100 compute).
// The reference's HIP backend hands both to the vendor library (csrilu0 / csric0); this library links none.
//
// Dependencies: row i needs the FINISHED rows k < i for which a_ik is stored -- for ILU their U part and
// pivot, for IC their whole lower part.  That is the lower-triangular level structure trs_levels.hip
// analyses, run on the pattern of the whole of A.  Rows of one level are independent.
//
// Bits.  compute_lu forms entry (i, j) as a_ij minus l_ik u_kj over the stored k < min(i, j) of row i in
// ascending k, one product and one difference each, then divides by u_jj below the diagonal.  The row-wise
// IKJ form used here walks the lower entries k of row i in the same ascending order and, per k, subtracts
// l_ik u_kj from every stored j > k of row i for which row k stores j: every entry sees the same terms in
// the same order.  Different j of one k step are different entries (the lanes of a group take them), and the
// group meets between two k steps.  ic compute is a chain inside the row (entry (i, j) needs every earlier
// l_ik), so only the products of one dot are formed in parallel; the sum starts at +0.0 and the products are
// added one after the other in ascending k.  A column of row j that row i does not store contributes +0.0:
// a sum that starts at +0.0 is never -0.0 (x + y is -0.0 only for x = y = -0.0), so adding +0.0 leaves every
// bit alone.  Quotient and root are the IEEE ones; the library is built with -ffp-contract=off.
//
// The working row lives in LDS (an "image" per group); finished rows are read from memory.
//
// Scheduling: as in fact_levels.hpp, whose frame runs ilu_row and ic_row over the levels analysed here.
#include "common.hpp"

#include <vector>

#include "fact_levels.hpp"
#include "internal.hpp"
#include "sort_scan.hpp"

namespace gkomi {
namespace {

// the bins, the analysed workspace, the meetings and the frame are shared with the sweeps (fact_levels.hpp)
using namespace fact;

// diag[row] = position of the diagonal; flags[0] |= 1: a row without diagonal, |= 2: a row that is not
// strictly ascending or leaves [0, n); flags[1] = longest row
__global__ __launch_bounds__(256) void fact_check_rows_kernel(int32_t n, const int32_t* __restrict__ row_ptrs,
                                                             const int32_t* __restrict__ col_idxs,
                                                             int32_t* __restrict__ diag, int32_t* __restrict__ flags)
{
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const int begin = row_ptrs[row], end = row_ptrs[row + 1];
    int d = -1, bad = 0, prev = -1;
    for (int k = begin; k < end; ++k) {
        const int col = col_idxs[k];
        if (col <= prev || col >= n) bad = 2;
        if (col == row) d = k;
        prev = col;
    }
    if (end < begin) bad = 2;
    diag[row] = d;
    if (d < 0) bad |= 1;
    if (bad) atomicOr(flags, bad);
    atomicMax(flags + 1, end - begin);
}

// level_longest[l] = longest row of level l, level_bins[3 l + b] = its rows of bin b (both zeroed by the caller)
__global__ __launch_bounds__(256) void fact_level_longest_kernel(int32_t n, const int32_t* __restrict__ row_ptrs,
                                                                const int32_t* __restrict__ perm,
                                                                const int32_t* __restrict__ level_sorted,
                                                                int32_t* __restrict__ level_longest,
                                                                int32_t* __restrict__ level_bins)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int row = perm[p];
    const int len = row_ptrs[row + 1] - row_ptrs[row];
    atomicMax(level_longest + level_sorted[p], len);
    atomicAdd(level_bins + 3 * level_sorted[p] + bin_of(len), 1);
}

// compute_lu of one row by a group of W lanes (t = my lane in the group).  w: the working row (len entries).
template <int W, bool InMemory, bool Coherent, class Meet>
__device__ __forceinline__ void ilu_row(int t, int row, const int32_t* __restrict__ row_ptrs,
                                        const int32_t* __restrict__ col_idxs, const int32_t* __restrict__ diag,
                                        double* vals, double* w, Meet meet)
{
    const int begin = row_ptrs[row];
    const int len = row_ptrs[row + 1] - begin;
    const int dpos = diag[row] - begin;
    const int32_t* cols = col_idxs + begin;
    if (!InMemory) {
        for (int q = t; q < len; q += W) w[q] = vals[begin + q];
        meet();
    }
    for (int p = 0; p < dpos; ++p) {
        const int k = cols[p];
        const int dk = diag[k];
        const double l = wld<InMemory>(w + p) / finished<Coherent>(vals + dk);
        const int kend = row_ptrs[k + 1];
        for (int q = dk + 1 + t; q < kend; q += W) {
            const int r = find_col(cols, p + 1, len, col_idxs[q]);
            if (r >= 0) {
                const double prod = l * finished<Coherent>(vals + q);
                wst<InMemory>(w + r, wld<InMemory>(w + r) - prod);
            }
        }
        meet();
        // nobody reads entry p of the working row any more
        if (t == 0) vals[begin + p] = l;
    }
    if (!InMemory) {
        for (int q = dpos + t; q < len; q += W) vals[begin + q] = w[q];
    }
}

// ic compute of one row.  w: the lower part of the working row with its diagonal; products: W doubles of the group.
template <int W, bool InMemory, bool Coherent, class Meet>
__device__ __forceinline__ void ic_row(int t, int row, const int32_t* __restrict__ row_ptrs,
                                       const int32_t* __restrict__ col_idxs, const int32_t* __restrict__ diag,
                                       double* vals, double* w, double* products, Meet meet)
{
    const int begin = row_ptrs[row];
    const int dpos = diag[row] - begin;
    const int32_t* cols = col_idxs + begin;
    if (!InMemory) {
        for (int q = t; q <= dpos; q += W) w[q] = vals[begin + q];
        meet();
    }
    for (int p = 0; p <= dpos; ++p) {
        const int j = cols[p];
        const bool is_diag = p == dpos;
        const double a = wld<InMemory>(w + p);
        // the lower entries of row j; for the diagonal they are this row's own, in the working row
        const int jb = row_ptrs[j];
        const int jd = is_diag ? begin + dpos : diag[j];
        double sum = 0.0;
        for (int base = jb; base < jd; base += W) {
            const int q = base + t;
            double prod = 0.0;
            if (q < jd) {
                if (is_diag) {
                    const double v = wld<InMemory>(w + (q - begin));
                    prod = v * v;
                } else {
                    const int r = find_col(cols, 0, p, col_idxs[q]);
                    if (r >= 0) prod = wld<InMemory>(w + r) * finished<Coherent>(vals + q);
                }
            }
            products[t] = prod;
            meet();
            const int m = jd - base < W ? jd - base : W;
            for (int s = 0; s < m; ++s) sum += products[s];
            meet();
        }
        const double diff = a - sum;
        const double l = is_diag ? sqrt(diff) : diff / finished<Coherent>(vals + jd);
        meet();
        if (t == 0) wst<InMemory>(w + p, l);
        meet();
    }
    if (!InMemory) {
        for (int q = t; q <= dpos; q += W) vals[begin + q] = w[q];
    }
}

// ---- the row policies of the frame (fact_levels.hpp) -----------------------------------------------------
// A's own rows bin them; a row too long for LDS is factorized in place
template <bool Ic>
struct csr_rows {
    const int32_t* row_ptrs;
    const int32_t* col_idxs;
    const int32_t* diag;
    double* vals;
    static constexpr bool needs_products = Ic;
    __device__ __forceinline__ int length(int i) const { return row_ptrs[i + 1] - row_ptrs[i]; }
    __device__ __forceinline__ double* memory_row(int i) const { return vals + row_ptrs[i]; }
    template <int W, bool InMemory, bool Coherent, class Meet>
    __device__ __forceinline__ void row(int t, int i, double* w, double* products, Meet meet) const
    {
        if constexpr (Ic) {
            ic_row<W, InMemory, Coherent>(t, i, row_ptrs, col_idxs, diag, vals, w, products, meet);
        } else {
            ilu_row<W, InMemory, Coherent>(t, i, row_ptrs, col_idxs, diag, vals, w, meet);
        }
    }
};
using ilu_rows = csr_rows<false>;
using ic_rows = csr_rows<true>;

template <class Rows>
int compute(hipStream_t stream, int64_t n, const int32_t* row_ptrs, const int32_t* col_idxs, double* vals,
            const void* workspace, size_t workspace_bytes)
{
    if (n < 0) return GKOMI_EINVAL;
    if (n > INT32_MAX - 1024) return GKOMI_ENOTSUPPORTED;
    const analysis_layout l = make_layout(n);
    if (workspace == nullptr || workspace_bytes < l.total) return GKOMI_EWORKSPACE;
    const char* ws = static_cast<const char*>(workspace);
    schedule sched;
    GKOMI_TRY(load_schedule(stream, ws, n, &sched));
    if (n == 0) return GKOMI_SUCCESS;
    return launch_schedule<Rows>(stream, sched, row_ptrs, col_idxs, reinterpret_cast<const int32_t*>(ws + l.diag), vals);
}

}  // namespace

// the numeric phase of lu_factorization::factorize (lu.hip) is compute_lu on a pattern closed under fill
int ilu_compute_lu(hipStream_t stream, int64_t n, const int32_t* row_ptrs, const int32_t* col_idxs, double* vals,
                   const void* analysis_workspace, size_t workspace_bytes)
{
    return compute<ilu_rows>(stream, n, row_ptrs, col_idxs, vals, analysis_workspace, workspace_bytes);
}

}  // namespace gkomi

using namespace gkomi;

extern "C" size_t gkomi_ilu_analysis_workspace_bytes(int64_t n)
{
    if (n < 0 || n > INT32_MAX - 1024) return 0;
    return make_layout(n).total;
}

extern "C" int gkomi_ilu_analyse_i32(gkomi_stream_t s, int64_t n, const int32_t* row_ptrs, const int32_t* col_idxs,
                                     void* workspace, size_t workspace_bytes, int64_t* host_out)
{
    if (n < 0 || host_out == nullptr) return GKOMI_EINVAL;
    if (n > INT32_MAX - 1024) return GKOMI_ENOTSUPPORTED;
    const analysis_layout l = make_layout(n);
    if (workspace == nullptr || workspace_bytes < l.total) return GKOMI_EWORKSPACE;
    hipStream_t stream = to_stream(s);
    char* ws = static_cast<char*>(workspace);
    for (int i = 0; i < 6; ++i) host_out[i] = 0;
    // the workspace is not valid until the end of a successful analysis
    GKOMI_TRY(static_cast<int>(hipMemsetAsync(ws, 0, 256, stream)));
    analysis_header h{};
    h.magic = ws_magic;
    h.n = n;
    if (n > 0) {
        int32_t* diag = reinterpret_cast<int32_t*>(ws + l.diag);
        int32_t* level = reinterpret_cast<int32_t*>(ws + l.level);
        int32_t* level_sorted = reinterpret_cast<int32_t*>(ws + l.level_sorted);
        int32_t* rows = reinterpret_cast<int32_t*>(ws + l.rows);
        int32_t* perm = reinterpret_cast<int32_t*>(ws + l.perm);
        int32_t* cnt = reinterpret_cast<int32_t*>(ws + l.cnt);
        int32_t* level_start = reinterpret_cast<int32_t*>(ws + l.level_start);
        int32_t* level_longest = reinterpret_cast<int32_t*>(ws + l.level_longest);
        int32_t* level_bins = reinterpret_cast<int32_t*>(ws + l.level_bins);
        int32_t* flags = reinterpret_cast<int32_t*>(ws + l.flags);
        const int32_t n32 = static_cast<int32_t>(n);
        const dim3 grid(static_cast<unsigned>(ceildiv(n, 256)));
        GKOMI_TRY(static_cast<int>(hipMemsetAsync(flags, 0, 256, stream)));
        hipLaunchKernelGGL(fact_check_rows_kernel, grid, dim3(256), 0, stream, n32, row_ptrs, col_idxs, diag, flags);
        int32_t hf[2] = {0, 0};
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(hf, flags, sizeof(hf), hipMemcpyDeviceToHost, stream)));
        int32_t nnz = 0;
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(&nnz, row_ptrs + n, sizeof(nnz), hipMemcpyDeviceToHost, stream)));
        GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
        if (hf[0] != 0) return GKOMI_EINVAL;  // a row without its diagonal, or not strictly ascending
        h.nnz = nnz;
        h.longest_row = hf[1];
        GKOMI_TRY(trs_relax_lower_levels(stream, n, row_ptrs, col_idxs, level, cnt, flags));
        GKOMI_TRY(trs_iota(stream, n, rows));
        // stable: the rows of a level keep their order
        GKOMI_TRY(radix_sort_u32(stream, n, reinterpret_cast<const uint32_t*>(level),
                                 reinterpret_cast<uint32_t*>(level_sorted), reinterpret_cast<const uint32_t*>(rows),
                                 reinterpret_cast<uint32_t*>(perm), 32, ws + l.tmp, l.tmp_bytes));
        int32_t top = 0;
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(&top, level_sorted + (n - 1), sizeof(top), hipMemcpyDeviceToHost, stream)));
        GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
        const int64_t nlevels = static_cast<int64_t>(top) + 1;
        if (nlevels < 1 || nlevels > n) return GKOMI_EINVAL;
        h.nlevels = nlevels;
        GKOMI_TRY(trs_level_starts(stream, n, nlevels, level_sorted, level_start));
        GKOMI_TRY(static_cast<int>(hipMemsetAsync(level_longest, 0, sizeof(int32_t) * nlevels, stream)));
        GKOMI_TRY(static_cast<int>(hipMemsetAsync(level_bins, 0, sizeof(int32_t) * 3 * nlevels, stream)));
        hipLaunchKernelGGL(fact_level_longest_kernel, grid, dim3(256), 0, stream, n32, row_ptrs, perm, level_sorted,
                           level_longest, level_bins);
        std::vector<int32_t> start(static_cast<size_t>(nlevels) + 1), longest(static_cast<size_t>(nlevels)),
            bins(3 * static_cast<size_t>(nlevels));
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(bins.data(), level_bins, sizeof(int32_t) * bins.size(),
                                                  hipMemcpyDeviceToHost, stream)));
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(start.data(), level_start, sizeof(int32_t) * start.size(),
                                                  hipMemcpyDeviceToHost, stream)));
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(longest.data(), level_longest, sizeof(int32_t) * longest.size(),
                                                  hipMemcpyDeviceToHost, stream)));
        GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
        // the launches of the numeric phase
        for (int64_t lvl = 0; lvl < nlevels; ++lvl) {
            if (start[lvl + 1] - start[lvl] > h.widest_level) h.widest_level = start[lvl + 1] - start[lvl];
        }
        std::vector<segment> segs;
        for (int64_t lvl = 0; lvl < nlevels;) {
            const int32_t width = start[lvl + 1] - start[lvl];
            if (width > narrow_level_rows) {
                int32_t mask = 0;
                for (int b = 0; b < 3; ++b) {
                    if (bins[3 * lvl + b] > 0) {
                        mask |= 1 << b;
                        ++h.launches;
                    }
                }
                segs.push_back({0, start[lvl], start[lvl + 1], longest[lvl], mask, 0});
                ++lvl;
                continue;
            }
            int64_t end = lvl;
            int32_t run_longest = 0;
            for (; end < nlevels && start[end + 1] - start[end] <= narrow_level_rows; ++end) {
                if (longest[end] > run_longest) run_longest = longest[end];
            }
            segs.push_back({1, static_cast<int32_t>(lvl), static_cast<int32_t>(end), run_longest, 0, 0});
            ++h.narrow_runs;
            ++h.launches;
            lvl = end;
        }
        h.nsegments = static_cast<int64_t>(segs.size());
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(ws + l.segments, segs.data(), sizeof(segment) * segs.size(),
                                                  hipMemcpyHostToDevice, stream)));
        GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));  // segs leaves scope
        GKOMI_TRY(check_launch());
    }
    GKOMI_TRY(static_cast<int>(hipMemcpyAsync(ws, &h, sizeof(h), hipMemcpyHostToDevice, stream)));
    GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
    host_out[0] = h.nlevels;
    host_out[1] = h.longest_row;
    host_out[2] = h.widest_level;
    host_out[3] = h.launches;
    host_out[4] = h.narrow_runs;
    host_out[5] = h.nnz;
    return GKOMI_SUCCESS;
}

extern "C" void gkomi_ilu_tuning(int64_t* host_out) { fill_tuning(host_out); }

extern "C" int gkomi_ilu_compute_lu_f64_i32(gkomi_stream_t s, int64_t n, const int32_t* row_ptrs,
                                            const int32_t* col_idxs, double* vals, const void* analysis_workspace,
                                            size_t workspace_bytes)
{
    return ilu_compute_lu(to_stream(s), n, row_ptrs, col_idxs, vals, analysis_workspace, workspace_bytes);
}

extern "C" int gkomi_ic_compute_f64_i32(gkomi_stream_t s, int64_t n, const int32_t* row_ptrs, const int32_t* col_idxs,
                                        double* vals, const void* analysis_workspace, size_t workspace_bytes)
{
    return compute<ic_rows>(to_stream(s), n, row_ptrs, col_idxs, vals, analysis_workspace, workspace_bytes);
}
