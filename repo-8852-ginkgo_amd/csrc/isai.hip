// ISAI: preconditioner::Isai (core/preconditioner/isai.cpp:121-265), the five kernels of
// core/preconditioner/isai_kernels.hpp with the results of reference/preconditioner/isai_kernels.cpp, bit for
// bit; <double, int32>.  The apply of the generated inverse is a CSR SpMV (gkomi_isai_apply_cb below).
//
// generate_tri_inverse / generate_general_inverse (:80-188, :192-236, :268-331).  A group of 32 lanes, two
// groups per wave, takes one row of the inverse.  A row of at most row_size_limit = 32 entries is solved in
// place: the dense system M[S(i), S(i)] is gathered into LDS (zero-filled; lane t merges the sorted row
// col(t) of M against the row's pattern, the reference's forall_matching :60-76), solved, and written with
// the reference's guard (a value that is not finite becomes 1 on the diagonal, 0 elsewhere).  A longer row
// only counts its right-hand-side entries and matches; an exclusive scan (sort_scan.hip) over n + 1 counts
// gives excess_rhs_ptrs / excess_nz_ptrs.
//
// Bits.  The system of a group lives in LDS (32 x 33 doubles), so the two rows that share a wave never
// exchange registers and may run loops of different length; a group meets through wave_meet only (LDS
// operations of a wave complete in program order).  No workgroup barrier, no atomics, no flags.
//   tri      the reference's column-oriented substitution :210-231: bot = rhs[col] / diag, lane `row`
//            computes rhs[row] -= bot * T(col, row); columns descending (lower) or ascending (upper).
//   general  the reference's Gauss-Jordan on the transposed system :290-326 as it is written: first maximum
//            of |.| as pivot, rows and rhs swapped, column col divided by -d, its diagonal set to 0, then
//            ts[i][j] += ts[i][col] * ts[col][j] for ALL i in ascending order and all j -- lane j owns
//            column j, the multipliers ts[i][col] are copied aside first because the sequential loop reads
//            each before its row changes, and row col itself is rewritten at i == col (x + 0 * x, which
//            turns an infinity into a NaN that the rows after it read) -- then the divisions by d; for spd
//            the scaling by 1 / sqrt(rhs[size - 1]).
// Every product is rounded before it is added (-ffp-contract=off, no fma call); / and sqrt are IEEE.
//
// generate_excess_system (:338-394), scale_excess_solution (:401-422), scatter_excess_solution (:429-447): a
// group per long row of [e_start, e_end); the entries of a row of the excess system start at a running sum of
// the matches of the entries before it, taken 32 at a time.
#include "common.hpp"

#include <cmath>

#include "internal.hpp"
#include "sort_scan.hpp"

namespace gkomi {
namespace {

constexpr int row_size_limit = 32;  // core/preconditioner/isai_kernels.hpp: kernels::isai::row_size_limit
constexpr int group = 32;           // lanes per row
constexpr int isai_block = 128;     // 4 groups: 4 x (32 x 33 + 64) doubles = 35 KB of the CU's 160 KB of LDS
constexpr int groups_per_block = isai_block / group;
constexpr int sys_stride = row_size_limit + 1;

struct wave_meet {
    __device__ __forceinline__ void operator()() const
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
};

struct csr_pattern {
    const int32_t* __restrict__ row_ptrs;
    const int32_t* __restrict__ col_idxs;
};

// forall_matching (:60-76) of row `col` of M against the pattern row [i_cols, i_cols + i_size)
template <class Callback>
__device__ __forceinline__ void forall_matching(const int32_t* __restrict__ m_cols, int m_size,
                                                const int32_t* __restrict__ i_cols, int i_size, Callback cb)
{
    int fst = 0, snd = 0;
    while (fst < m_size && snd < i_size) {
        const int32_t fst_val = m_cols[fst];
        const int32_t snd_val = i_cols[snd];
        if (fst_val == snd_val) cb(fst_val, fst, snd);
        fst += fst_val <= snd_val;
        snd += fst_val >= snd_val;
    }
}

// row `col` of M, empty for an index that no row of M has
__device__ __forceinline__ void m_row(int32_t n, const int32_t* __restrict__ m_row_ptrs, int32_t col, int* begin, int* size)
{
    if (col < 0 || col >= n) {
        *begin = 0;
        *size = 0;
        return;
    }
    *begin = m_row_ptrs[col];
    *size = m_row_ptrs[col + 1] - *begin;
}

// Tri: 0 general, 1 lower, 2 upper.  Spd only with Tri == 0.
template <int Tri, bool Spd>
__global__ __launch_bounds__(isai_block) void isai_generate_kernel(int32_t n, const int32_t* __restrict__ m_row_ptrs,
                                                                   const int32_t* __restrict__ m_cols,
                                                                   const double* __restrict__ m_vals,
                                                                   const int32_t* __restrict__ i_row_ptrs,
                                                                   const int32_t* __restrict__ i_cols_all,
                                                                   double* __restrict__ i_vals, int32_t* __restrict__ rhs_counts,
                                                                   int32_t* __restrict__ nz_counts)
{
    __shared__ double sys_all[groups_per_block][row_size_limit * sys_stride];
    __shared__ double rhs_all[groups_per_block][row_size_limit];
    __shared__ double aside_all[groups_per_block][row_size_limit];
    __shared__ int32_t ints_all[groups_per_block][group];
    const int g = threadIdx.x / group, t = threadIdx.x % group;
    double* sys = sys_all[g];
    double* rhs = rhs_all[g];
    double* aside = aside_all[g];
    int32_t* ints = ints_all[g];
    const wave_meet meet;
    const int64_t total_groups = static_cast<int64_t>(gridDim.x) * groups_per_block;
    for (int64_t row64 = static_cast<int64_t>(blockIdx.x) * groups_per_block + g; row64 < n; row64 += total_groups) {
        const int32_t row = static_cast<int32_t>(row64);
        const int i_begin = i_row_ptrs[row];
        const int i_size = i_row_ptrs[row + 1] - i_begin;
        const int32_t* i_cols = i_cols_all + i_begin;
        if (i_size > row_size_limit) {
            // count the matches of the row's entries (:174-183)
            int matches = 0;
            for (int i = t; i < i_size; i += group) {
                int m_begin, m_size;
                m_row(n, m_row_ptrs, i_cols[i], &m_begin, &m_size);
                forall_matching(m_cols + m_begin, m_size, i_cols, i_size, [&](int32_t, int, int) { ++matches; });
            }
            ints[t] = matches;
            meet();
            if (t == 0) {
                int sum = 0;
                for (int k = 0; k < group; ++k) sum += ints[k];
                rhs_counts[row] = i_size;
                nz_counts[row] = sum;
            }
            meet();
            continue;
        }
        if (t == 0) {
            rhs_counts[row] = 0;
            nz_counts[row] = 0;
        }
        if (i_size <= 0) continue;
        const int size = i_size;
        // the dense system, zero-filled (:129-154)
        for (int r = 0; r < size; ++r) sys[r * sys_stride + t] = 0.0;
        ints[0] = 0;  // rhs_one_idx
        meet();
        if (t < size) {
            const int32_t col = i_cols[t];
            int m_begin, m_size;
            m_row(n, m_row_ptrs, col, &m_begin, &m_size);
            int below = 0;
            forall_matching(m_cols + m_begin, m_size, i_cols, size, [&](int32_t m_col, int m_idx, int i_idx) {
                if (m_col < row && col == row) ++below;
                if (Tri != 0) {
                    sys[t * sys_stride + i_idx] = m_vals[m_begin + m_idx];
                } else {
                    sys[i_idx * sys_stride + t] = m_vals[m_begin + m_idx];
                }
            });
            if (col == row) ints[0] = below;
        }
        meet();
        if (Tri != 0) {
            // trs_solve (:198-232)
            if (t < size) rhs[t] = t == (Tri == 1 ? size - 1 : 0) ? 1.0 : 0.0;
            meet();
            for (int k = 0; k < size; ++k) {
                const int col = Tri == 1 ? size - 1 - k : k;
                const double diag = sys[col * sys_stride + col];
                const double bot = rhs[col] / diag;
                meet();  // every lane has read rhs[col]
                if (t == col) rhs[col] = bot;
                const bool mine = Tri == 1 ? t < col : (t > col && t < size);
                if (mine) rhs[t] = rhs[t] - bot * sys[col * sys_stride + t];
                meet();
            }
        } else {
            // general_solve (:275-327)
            if (t < size) rhs[t] = t == ints[0] ? 1.0 : 0.0;
            meet();
            for (int col = 0; col < size; ++col) {
                // choose_pivot (:243-253) on column col from row col on: the first maximum
                int piv = col;
                for (int i = col + 1; i < size; ++i) {
                    if (fabs(sys[piv * sys_stride + col]) < fabs(sys[i * sys_stride + col])) piv = i;
                }
                meet();
                if (piv != col) {
                    if (t < size) {
                        const double a = sys[col * sys_stride + t], b = sys[piv * sys_stride + t];
                        sys[col * sys_stride + t] = b;
                        sys[piv * sys_stride + t] = a;
                    }
                    if (t == 0) {
                        const double a = rhs[col], b = rhs[piv];
                        rhs[col] = b;
                        rhs[piv] = a;
                    }
                    meet();
                }
                const double d = sys[col * sys_stride + col];
                meet();  // every lane has read d
                if (t < size) {
                    // column col divided by -d, its diagonal entry then set to 0; the multipliers set aside
                    const double q = t == col ? 0.0 : sys[t * sys_stride + col] / -d;
                    sys[t * sys_stride + col] = q;
                    aside[t] = q;
                }
                meet();
                const double rhs_key_val = rhs[col];
                meet();  // every lane has read rhs[col]
                if (t < size) {
                    // column t of the update, rows ascending; row col is rewritten when i reaches it
                    const double p_old = sys[col * sys_stride + t];
                    const double p_new = p_old + aside[col] * p_old;
                    for (int i = 0; i < size; ++i) {
                        if (i == col) {
                            sys[col * sys_stride + t] = p_new;
                        } else {
                            const double scal = aside[i];
                            const double p = i < col ? p_old : p_new;
                            sys[i * sys_stride + t] = sys[i * sys_stride + t] + scal * p;
                        }
                    }
                    rhs[t] = rhs[t] + rhs_key_val * aside[t];
                }
                meet();
                if (t < size) {
                    sys[col * sys_stride + t] = t == col ? 1.0 / d : sys[col * sys_stride + t] / d;
                }
                if (t == col) rhs[col] = rhs[col] / d;
                meet();
            }
            if (Spd) {
                const double scal = 1.0 / sqrt(rhs[size - 1]);
                meet();  // every lane has read rhs[size - 1]
                if (t < size) rhs[t] = rhs[t] * scal;
                meet();
            }
        }
        // the row, with the guard (:160-171)
        if (t < size) {
            const double new_val = rhs[t];
            i_vals[i_begin + t] = std::isfinite(new_val) ? new_val : (i_cols[t] == row ? 1.0 : 0.0);
        }
        meet();  // sys and rhs are used again
    }
}

__global__ __launch_bounds__(isai_block) void isai_excess_system_kernel(
    int32_t n, const int32_t* __restrict__ m_row_ptrs, const int32_t* __restrict__ m_cols, const double* __restrict__ m_vals,
    const int32_t* __restrict__ i_row_ptrs, const int32_t* __restrict__ i_cols_all, const int32_t* __restrict__ excess_rhs_ptrs,
    const int32_t* __restrict__ excess_nz_ptrs, int32_t* __restrict__ e_row_ptrs, int32_t* __restrict__ e_cols,
    double* __restrict__ e_vals, double* __restrict__ e_rhs, int32_t e_start, int32_t e_end)
{
    __shared__ int32_t ints_all[groups_per_block][group];
    const int g = threadIdx.x / group, t = threadIdx.x % group;
    int32_t* ints = ints_all[g];
    const wave_meet meet;
    const int64_t total_groups = static_cast<int64_t>(gridDim.x) * groups_per_block;
    const int32_t rhs_offset = excess_rhs_ptrs[e_start], nz_offset = excess_nz_ptrs[e_start];
    for (int64_t row64 = e_start + static_cast<int64_t>(blockIdx.x) * groups_per_block + g; row64 < e_end; row64 += total_groups) {
        const int32_t row = static_cast<int32_t>(row64);
        const int i_begin = i_row_ptrs[row];
        const int i_size = i_row_ptrs[row + 1] - i_begin;
        if (i_size <= row_size_limit) continue;
        const int32_t* i_cols = i_cols_all + i_begin;
        const int32_t e_begin = excess_rhs_ptrs[row] - rhs_offset;
        int32_t e_nz = excess_nz_ptrs[row] - nz_offset;
        for (int base = 0; base < i_size; base += group) {
            const int i = base + t;
            int32_t col = 0;
            int m_begin = 0, m_size = 0, matches = 0;
            if (i < i_size) {
                col = i_cols[i];
                m_row(n, m_row_ptrs, col, &m_begin, &m_size);
                forall_matching(m_cols + m_begin, m_size, i_cols, i_size, [&](int32_t, int, int) { ++matches; });
            }
            ints[t] = matches;
            meet();
            int32_t before = 0, all = 0;
            for (int k = 0; k < group; ++k) {
                const int32_t c = ints[k];
                before += k < t ? c : 0;
                all += c;
            }
            meet();  // ints is used again
            if (i < i_size) {
                const int32_t e_row = e_begin + i;
                int32_t at = e_nz + before;
                e_row_ptrs[e_row] = at;
                e_rhs[e_row] = row == col ? 1.0 : 0.0;
                forall_matching(m_cols + m_begin, m_size, i_cols, i_size, [&](int32_t, int m_idx, int i_idx) {
                    e_cols[at] = i_idx + e_begin;
                    e_vals[at] = m_vals[m_begin + m_idx];
                    ++at;
                });
            }
            e_nz += all;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        e_row_ptrs[excess_rhs_ptrs[e_end] - rhs_offset] = excess_nz_ptrs[e_end] - nz_offset;
    }
}

__global__ __launch_bounds__(isai_block) void isai_scale_excess_kernel(const int32_t* __restrict__ excess_block_ptrs,
                                                                       double* __restrict__ excess_values, int32_t e_start,
                                                                       int32_t e_end)
{
    const int g = threadIdx.x / group, t = threadIdx.x % group;
    const int64_t total_groups = static_cast<int64_t>(gridDim.x) * groups_per_block;
    const int32_t offset = excess_block_ptrs[e_start];
    for (int64_t row = e_start + static_cast<int64_t>(blockIdx.x) * groups_per_block + g; row < e_end; row += total_groups) {
        const int32_t block_start = excess_block_ptrs[row] - offset;
        const int32_t block_end = excess_block_ptrs[row + 1] - offset;
        if (block_end == block_start) continue;
        // read by every lane of the group before the lane that owns the entry scales it: one wave, program order
        const double last = excess_values[block_end - 1];
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        const double scal = 1.0 / sqrt(last);
        for (int32_t i = block_start + t; i < block_end; i += group) excess_values[i] = excess_values[i] * scal;
    }
}

__global__ __launch_bounds__(isai_block) void isai_scatter_excess_kernel(const int32_t* __restrict__ excess_block_ptrs,
                                                                         const double* __restrict__ excess_values,
                                                                         const int32_t* __restrict__ i_row_ptrs,
                                                                         double* __restrict__ i_vals, int32_t e_start,
                                                                         int32_t e_end)
{
    const int g = threadIdx.x / group, t = threadIdx.x % group;
    const int64_t total_groups = static_cast<int64_t>(gridDim.x) * groups_per_block;
    const int32_t offset = excess_block_ptrs[e_start];
    for (int64_t row = e_start + static_cast<int64_t>(blockIdx.x) * groups_per_block + g; row < e_end; row += total_groups) {
        const int32_t begin = excess_block_ptrs[row] - offset;
        const int32_t count = excess_block_ptrs[row + 1] - offset - begin;
        const int32_t out = i_row_ptrs[row];
        for (int32_t i = t; i < count; i += group) i_vals[out + i] = excess_values[begin + i];
    }
}

int isai_grid(int64_t rows) { return grid_for(rows, groups_per_block); }

bool bad_size(int64_t n) { return n < 0; }
bool too_large(int64_t n) { return n > INT32_MAX - 1024; }

template <int Tri, bool Spd>
int isai_generate(gkomi_stream_t s, int64_t n, const int32_t* m_row_ptrs, const int32_t* m_col_idxs, const double* m_vals,
                  const int32_t* i_row_ptrs, const int32_t* i_col_idxs, double* i_vals, int32_t* excess_rhs_ptrs,
                  int32_t* excess_nz_ptrs, void* workspace, size_t workspace_bytes)
{
    hipStream_t stream = to_stream(s);
    // the counts of the n rows and a last 0, scanned in place: entry n is the total
    GKOMI_TRY(static_cast<int>(hipMemsetAsync(excess_rhs_ptrs + n, 0, sizeof(int32_t), stream)));
    GKOMI_TRY(static_cast<int>(hipMemsetAsync(excess_nz_ptrs + n, 0, sizeof(int32_t), stream)));
    if (n > 0) {
        hipLaunchKernelGGL((isai_generate_kernel<Tri, Spd>), dim3(isai_grid(n)), dim3(isai_block), 0, stream,
                           static_cast<int32_t>(n), m_row_ptrs, m_col_idxs, m_vals, i_row_ptrs, i_col_idxs, i_vals,
                           excess_rhs_ptrs, excess_nz_ptrs);
        GKOMI_TRY(check_launch());
    }
    GKOMI_TRY(exclusive_sum_i32(stream, excess_rhs_ptrs, excess_rhs_ptrs, n + 1, workspace, workspace_bytes));
    return exclusive_sum_i32(stream, excess_nz_ptrs, excess_nz_ptrs, n + 1, workspace, workspace_bytes);
}

// what both generate entries check before any HIP call
int check_generate(int64_t n, const int32_t* m_row_ptrs, const int32_t* m_col_idxs, const double* m_vals,
                   const int32_t* i_row_ptrs, const int32_t* i_col_idxs, double* i_vals, int32_t* excess_rhs_ptrs,
                   int32_t* excess_nz_ptrs, int flag, void* workspace, size_t workspace_bytes)
{
    if (bad_size(n) || (flag != 0 && flag != 1)) return GKOMI_EINVAL;
    if (excess_rhs_ptrs == nullptr || excess_nz_ptrs == nullptr) return GKOMI_EINVAL;
    if (n > 0 && (m_row_ptrs == nullptr || m_col_idxs == nullptr || m_vals == nullptr || i_row_ptrs == nullptr ||
                  i_col_idxs == nullptr || i_vals == nullptr)) {
        return GKOMI_EINVAL;
    }
    if (too_large(n)) return GKOMI_ENOTSUPPORTED;
    if (workspace == nullptr || workspace_bytes < scan_workspace_bytes(n + 1)) return GKOMI_EWORKSPACE;
    return GKOMI_SUCCESS;
}

int check_range(int64_t n, int64_t e_start, int64_t e_end)
{
    if (bad_size(n) || e_start < 0 || e_end < e_start || e_end > n) return GKOMI_EINVAL;
    return too_large(n) ? GKOMI_ENOTSUPPORTED : GKOMI_SUCCESS;
}

int spmv_of(gkomi_stream_t s, const gkomi_csr_ctx& m, int64_t nrhs, const double* in, double* out)
{
    return gkomi_csr_spmv_srow_f64_i32(s, m.nrows, m.ncols, nrhs, m.nnz, m.row_ptrs, m.col_idxs, m.vals, in, nrhs, out, nrhs,
                                       nullptr, nullptr, static_cast<int>(m.strategy), m.max_row_nnz_hint, m.srow,
                                       m.srow != nullptr ? m.srow_tile : 0);
}

}  // namespace
}  // namespace gkomi

using namespace gkomi;

extern "C" size_t gkomi_isai_generate_workspace_bytes(int64_t n)
{
    if (bad_size(n) || too_large(n)) return 0;
    return scan_workspace_bytes(n + 1);
}

extern "C" int gkomi_isai_generate_tri_inverse_f64_i32(gkomi_stream_t s, int64_t n, const int32_t* m_row_ptrs,
                                                       const int32_t* m_col_idxs, const double* m_vals,
                                                       const int32_t* i_row_ptrs, const int32_t* i_col_idxs, double* i_vals,
                                                       int32_t* excess_rhs_ptrs, int32_t* excess_nz_ptrs, int lower,
                                                       void* workspace, size_t workspace_bytes)
{
    GKOMI_TRY(check_generate(n, m_row_ptrs, m_col_idxs, m_vals, i_row_ptrs, i_col_idxs, i_vals, excess_rhs_ptrs,
                             excess_nz_ptrs, lower, workspace, workspace_bytes));
    return lower ? isai_generate<1, false>(s, n, m_row_ptrs, m_col_idxs, m_vals, i_row_ptrs, i_col_idxs, i_vals,
                                           excess_rhs_ptrs, excess_nz_ptrs, workspace, workspace_bytes)
                 : isai_generate<2, false>(s, n, m_row_ptrs, m_col_idxs, m_vals, i_row_ptrs, i_col_idxs, i_vals,
                                           excess_rhs_ptrs, excess_nz_ptrs, workspace, workspace_bytes);
}

extern "C" int gkomi_isai_generate_general_inverse_f64_i32(gkomi_stream_t s, int64_t n, const int32_t* m_row_ptrs,
                                                           const int32_t* m_col_idxs, const double* m_vals,
                                                           const int32_t* i_row_ptrs, const int32_t* i_col_idxs,
                                                           double* i_vals, int32_t* excess_rhs_ptrs, int32_t* excess_nz_ptrs,
                                                           int spd, void* workspace, size_t workspace_bytes)
{
    GKOMI_TRY(check_generate(n, m_row_ptrs, m_col_idxs, m_vals, i_row_ptrs, i_col_idxs, i_vals, excess_rhs_ptrs,
                             excess_nz_ptrs, spd, workspace, workspace_bytes));
    return spd ? isai_generate<0, true>(s, n, m_row_ptrs, m_col_idxs, m_vals, i_row_ptrs, i_col_idxs, i_vals, excess_rhs_ptrs,
                                        excess_nz_ptrs, workspace, workspace_bytes)
               : isai_generate<0, false>(s, n, m_row_ptrs, m_col_idxs, m_vals, i_row_ptrs, i_col_idxs, i_vals,
                                         excess_rhs_ptrs, excess_nz_ptrs, workspace, workspace_bytes);
}

extern "C" int gkomi_isai_generate_excess_system_f64_i32(gkomi_stream_t s, int64_t n, const int32_t* m_row_ptrs,
                                                         const int32_t* m_col_idxs, const double* m_vals,
                                                         const int32_t* i_row_ptrs, const int32_t* i_col_idxs,
                                                         const int32_t* excess_rhs_ptrs, const int32_t* excess_nz_ptrs,
                                                         int64_t e_dim, int64_t e_nnz, int32_t* e_row_ptrs,
                                                         int32_t* e_col_idxs, double* e_vals, double* e_rhs, int64_t e_start,
                                                         int64_t e_end)
{
    GKOMI_TRY(check_range(n, e_start, e_end));
    if (e_dim < 0 || e_nnz < 0 || e_dim > INT32_MAX - 1024 || e_nnz > INT32_MAX) return GKOMI_EINVAL;
    if (m_row_ptrs == nullptr || i_row_ptrs == nullptr || excess_rhs_ptrs == nullptr || excess_nz_ptrs == nullptr ||
        e_row_ptrs == nullptr) {
        return GKOMI_EINVAL;
    }
    if (e_dim > 0 && (i_col_idxs == nullptr || e_rhs == nullptr)) return GKOMI_EINVAL;
    if (e_nnz > 0 && (m_col_idxs == nullptr || m_vals == nullptr || e_col_idxs == nullptr || e_vals == nullptr)) {
        return GKOMI_EINVAL;
    }
    hipLaunchKernelGGL(isai_excess_system_kernel, dim3(isai_grid(e_end - e_start)), dim3(isai_block), 0, to_stream(s),
                       static_cast<int32_t>(n), m_row_ptrs, m_col_idxs, m_vals, i_row_ptrs, i_col_idxs, excess_rhs_ptrs,
                       excess_nz_ptrs, e_row_ptrs, e_col_idxs, e_vals, e_rhs, static_cast<int32_t>(e_start),
                       static_cast<int32_t>(e_end));
    return check_launch();
}

extern "C" int gkomi_isai_scale_excess_solution_f64_i32(gkomi_stream_t s, int64_t n, const int32_t* excess_block_ptrs,
                                                        double* excess_solution, int64_t e_start, int64_t e_end)
{
    GKOMI_TRY(check_range(n, e_start, e_end));
    if (excess_block_ptrs == nullptr) return GKOMI_EINVAL;
    if (e_end == e_start) return GKOMI_SUCCESS;
    if (excess_solution == nullptr) return GKOMI_EINVAL;
    hipLaunchKernelGGL(isai_scale_excess_kernel, dim3(isai_grid(e_end - e_start)), dim3(isai_block), 0, to_stream(s),
                       excess_block_ptrs, excess_solution, static_cast<int32_t>(e_start), static_cast<int32_t>(e_end));
    return check_launch();
}

extern "C" int gkomi_isai_scatter_excess_solution_f64_i32(gkomi_stream_t s, int64_t n, const int32_t* excess_block_ptrs,
                                                          const double* excess_solution, const int32_t* i_row_ptrs,
                                                          double* i_vals, int64_t e_start, int64_t e_end)
{
    GKOMI_TRY(check_range(n, e_start, e_end));
    if (excess_block_ptrs == nullptr || i_row_ptrs == nullptr) return GKOMI_EINVAL;
    if (e_end == e_start) return GKOMI_SUCCESS;
    if (excess_solution == nullptr || i_vals == nullptr) return GKOMI_EINVAL;
    hipLaunchKernelGGL(isai_scatter_excess_kernel, dim3(isai_grid(e_end - e_start)), dim3(isai_block), 0, to_stream(s),
                       excess_block_ptrs, excess_solution, i_row_ptrs, i_vals, static_cast<int32_t>(e_start),
                       static_cast<int32_t>(e_end));
    return check_launch();
}

// out = second * (first * in), or first * in alone: the apply of Isai (isai.hpp: approximate_inverse_->apply), of SpdIsai
// (L then L^T) and of Ilu / Ic over two Isai solvers (lower inverse, then upper inverse)
extern "C" int gkomi_isai_apply_cb(void* ctx_, gkomi_stream_t s, const double* in, double* out)
{
    const auto* c = static_cast<const gkomi_isai_ctx*>(ctx_);
    if (c == nullptr || c->n < 0 || c->nrhs < 0 || (c->num_matrices != 1 && c->num_matrices != 2)) return GKOMI_EINVAL;
    if (c->first.nrows != c->n || c->first.ncols != c->n) return GKOMI_EINVAL;
    if (c->num_matrices == 1) return spmv_of(s, c->first, c->nrhs, in, out);
    if (c->second.nrows != c->n || c->second.ncols != c->n) return GKOMI_EINVAL;
    if (c->intermediate == nullptr && c->n > 0 && c->nrhs > 0) return GKOMI_EINVAL;
    GKOMI_TRY(spmv_of(s, c->first, c->nrhs, in, c->intermediate));
    return spmv_of(s, c->second, c->nrhs, c->intermediate, out);
}
