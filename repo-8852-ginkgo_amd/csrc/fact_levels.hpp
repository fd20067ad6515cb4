// What the level-scheduled factorizations share (ilu.hip: exact ILU(0) / IC(0); par_ilut.hip, par_ict.hip: the
// ParILUT and ParICT sweeps): the analysed workspace of gkomi_ilu_analyse_i32, the row-length bins and the ways
// a group of lanes meets; and what the two add_candidates merges share.  Internal to the library.
#pragma once
#include "common.hpp"

#include "sort_scan.hpp"

namespace gkomi {
namespace fact {

constexpr int fact_block = 256;
// row-length bins: a row of at most bin_short entries is factorized by 8 lanes, one of at most bin_wave
// by a wave (both with an LDS image per group), one of at most bin_lds by a workgroup with the row in
// LDS, anything longer by a workgroup on the row in memory
constexpr int bin_short = 32;
constexpr int short_width = 8;
constexpr int bin_wave = 512;
constexpr int bin_lds = 1024;
// the boundary between (a) and (b): a level of at most this many rows is narrow (4 rows per wave of the
// one workgroup that walks it)
constexpr int narrow_level_rows = 16;
constexpr int max_level_grid = 4096;

constexpr int64_t ws_magic = 0x696c7530676b6f6dll;

struct analysis_header {
    int64_t magic;  // ws_magic once the analysis has succeeded
    int64_t n, nnz, nlevels, nsegments, longest_row, widest_level, narrow_runs, launches;
};
static_assert(sizeof(analysis_header) <= 256, "the header has 256 bytes");

// one launch of the numeric phase
struct segment {
    int32_t kind;      // 0: one wide level, 1: a run of narrow levels
    int32_t first;     // wide: first position of the level; run: first level
    int32_t last;      // wide: one past its last position;   run: one past the last level
    int32_t longest;   // longest row inside
    int32_t bins;      // wide: bit b set = the level holds a row of bin b (0 short, 1 wave, 2 workgroup)
    int32_t pad_;
};

struct analysis_layout {
    size_t diag, level, level_sorted, rows, perm, cnt, level_start, level_longest, level_bins, segments, flags, tmp, tmp_bytes, total;
};

inline analysis_layout make_layout(int64_t n)
{
    analysis_layout l{};
    const size_t m = static_cast<size_t>(n > 0 ? n : 1);
    const size_t vec = align256(sizeof(int32_t) * (m + 1));
    size_t off = 256;
    l.diag = off; off += vec;
    l.level = off; off += vec;
    l.level_sorted = off; off += vec;
    l.rows = off; off += vec;
    l.perm = off; off += vec;
    l.cnt = off; off += vec;
    l.level_start = off; off += vec;
    l.level_longest = off; off += vec;
    l.level_bins = off; off += align256(sizeof(int32_t) * 3 * (m + 1));
    l.segments = off; off += align256(sizeof(segment) * (m + 1));
    l.flags = off; off += 256;
    l.tmp_bytes = align256(radix_sort_workspace_bytes(static_cast<int64_t>(m), sizeof(uint32_t), true)) + 256;
    l.tmp = off; off += l.tmp_bytes;
    l.total = off;
    return l;
}

__host__ __device__ __forceinline__ int bin_of(int len) { return len <= bin_short ? 0 : (len <= bin_wave ? 1 : 2); }

// ---- the matrices of a merge kernel (add_candidates), and the end of its count call ----------------------
struct csr_in {
    const int32_t* row_ptrs;
    const int32_t* col_idxs;
    const double* vals;
};
struct csr_out {
    int32_t* row_ptrs;
    int32_t* col_idxs;
    double* vals;
};

// counts in ptrs[0, n) -> row pointers in ptrs[0, n], the total to the host
inline int finish_row_ptrs(hipStream_t stream, int64_t n, int32_t* ptrs, void* scan_ws, size_t scan_bytes, int64_t* host_total)
{
    GKOMI_TRY(static_cast<int>(hipMemsetAsync(ptrs + n, 0, sizeof(int32_t), stream)));
    GKOMI_TRY(exclusive_sum_i32(stream, ptrs, ptrs, n + 1, scan_ws, scan_bytes));
    int32_t total = 0;
    GKOMI_TRY(static_cast<int>(hipMemcpyAsync(&total, ptrs + n, sizeof(total), hipMemcpyDeviceToHost, stream)));
    GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
    *host_total = total;
    return GKOMI_SUCCESS;
}

inline size_t row_scan_bytes(int64_t n) { return align256(scan_workspace_bytes((n > 0 ? n : 1) + 1)) + 256; }

#ifdef __HIPCC__
// ---- how a group meets ------------------------------------------------------------------------------
// lanes of one wave: LDS operations of a wave complete in program order; the fences keep the compiler from
// moving an LDS access across the meeting point
struct wave_meet {
    __device__ __forceinline__ void operator()() const
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
};
struct block_meet {
    __device__ __forceinline__ void operator()() const { __syncthreads(); }
};

// a value of a finished row.  Coherent (the narrow-level workgroup: the row was finished by another wave of
// this launch): past the compute unit's vector cache, which may still hold the line from before.
template <bool Coherent>
__device__ __forceinline__ double finished(const double* p)
{
    if (Coherent) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return *p;
}
// the working row: an LDS image, or (InMemory) the row itself, shared by the waves of one workgroup
template <bool InMemory>
__device__ __forceinline__ double wld(const double* p)
{
    if (InMemory) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return *p;
}
template <bool InMemory>
__device__ __forceinline__ void wst(double* p, double v)
{
    if (InMemory) {
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        *p = v;
    }
}
#endif

}  // namespace fact
}  // namespace gkomi
