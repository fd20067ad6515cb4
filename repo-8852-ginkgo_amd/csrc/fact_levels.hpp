// What the level-scheduled factorizations share (ilu.hip: exact ILU(0) / IC(0); par_ilut.hip, par_ict.hip: the
// ParILUT and ParICT sweeps): the analysed workspace of gkomi_ilu_analyse_i32, the row-length bins and the ways
// a group of lanes meets, and the frame that schedules their rows; and what the two add_candidates merges share.
// Internal to the library.
//
// Scheduling.  No kernel here waits on another workgroup: no flags, no spins, no device-wide meetings.
//   (a) a level of more than `narrow_level_rows` rows is one launch per row-length bin it holds rows of (the
//       group width follows the row), each a capped grid that strides over the level's list of rows and takes
//       the rows of its bin;
//   (b) a run of consecutive levels of at most `narrow_level_rows` rows each is ONE launch of ONE
//       workgroup that walks the levels with __syncthreads in between (a chain or thin band would
//       otherwise cost a launch per row).
// All boundaries are tuning constants; none has been measured.
//
// The frame is written once, over a row policy `Rows`: an aggregate of the factorization's pointers, built in the
// kernel from its fields (see kernel_arg), with
//   length(row)                                  the length that bins the row (the one the analysis saw);
//   needs_products                               whether row() wants fact_block doubles of LDS for its products;
//   row<W, InMemory, Coherent>(t, row, w, products, meet)   one row by a group of W lanes, lane t;
//   memory_row(row)                              the working row of a row longer than bin_lds.
#pragma once
#include "common.hpp"

#include <vector>

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

// ---- the frame: the kernels of (a) and (b) over a row policy ------------------------------------------------
// A kernel takes the policy's fields one by one and builds the policy itself.  A field that is a pointer to const
// arrives as a `const T* __restrict__` kernel argument: the pattern, read-only and unaliased for the whole launch.
// Only of such an argument does the compiler know that no store and no meeting of the kernel changes what it
// points to, which keeps the uniform loads of the pattern scalar; a pointer inside a struct argument carries no
// such promise.  Any other field (a pointer to the values, a struct of pointers) arrives as it is.
template <class Field>
struct kernel_arg {
    using type = Field;
};
template <class T>
struct kernel_arg<const T*> {
    using type = const T* __restrict__;
};

// fact_block doubles of LDS for the products of the workgroup's lanes, only where the row routine forms any:
// those of the group whose first lane is `lane`
template <class Rows>
__device__ __forceinline__ double* products_from(int lane)
{
    if constexpr (Rows::needs_products) {
        __shared__ double products[fact_block];
        return products + lane;
    } else {
        return nullptr;
    }
}

// one row by a whole workgroup: in LDS when it fits, in memory otherwise.  image: bin_lds doubles.
template <class Rows, bool Coherent>
__device__ __forceinline__ void block_row(const Rows& rows, int row, double* image, double* products)
{
    if (rows.length(row) <= bin_lds) {
        rows.template row<fact_block, false, Coherent>(threadIdx.x, row, image, products, block_meet{});
    } else {
        rows.template row<fact_block, true, Coherent>(threadIdx.x, row, rows.memory_row(row), products, block_meet{});
    }
}

// (a) one wide level, its rows of bin Bin (at most Cap entries): a group of W lanes per row, grid-stride over
// perm[first, last); rows of the other bins are left to their own launch (rows of a level are independent)
template <class Rows, int W, int Cap, int Bin, class... Fields>
__global__ __launch_bounds__(fact_block) void level_kernel(const int32_t* __restrict__ perm, int first, int last,
                                                          typename kernel_arg<Fields>::type... fields)
{
    const Rows rows{fields...};
    constexpr int groups = fact_block / W;
    __shared__ double image[groups * Cap];
    const int g = threadIdx.x / W, t = threadIdx.x % W;
    double* products = products_from<Rows>(g * W);
    for (int pos = first + blockIdx.x * groups + g; pos < last; pos += gridDim.x * groups) {
        const int row = perm[pos];
        if (bin_of(rows.length(row)) != Bin) continue;  // the same answer in every lane of the group
        rows.template row<W, false, false>(t, row, image + g * Cap, products, wave_meet{});
        wave_meet{}();  // the image is used again
    }
}

// (a) the rows longer than bin_wave of one wide level: a workgroup per row
template <class Rows, class... Fields>
__global__ __launch_bounds__(fact_block) void level_block_kernel(const int32_t* __restrict__ perm, int first, int last,
                                                                typename kernel_arg<Fields>::type... fields)
{
    const Rows rows{fields...};
    __shared__ double image[bin_lds];
    double* products = products_from<Rows>(0);
    for (int pos = first + blockIdx.x; pos < last; pos += gridDim.x) {
        const int row = perm[pos];
        if (bin_of(rows.length(row)) != 2) continue;  // the same answer in the whole workgroup
        block_row<Rows, false>(rows, row, image, products);
        __syncthreads();
    }
}

// (b) ONE workgroup walks the narrow levels [first_level, last_level): a wave per row of at most bin_wave entries,
// then the workgroup per longer row, __syncthreads between levels.  What a level wrote is read by the
// next through agent-scope loads after a release fence.
template <class Rows, class... Fields>
__global__ __launch_bounds__(fact_block) void run_kernel(const int32_t* __restrict__ perm,
                                                        const int32_t* __restrict__ level_start,
                                                        const int32_t* __restrict__ level_longest, int first_level,
                                                        int last_level, typename kernel_arg<Fields>::type... fields)
{
    const Rows rows{fields...};
    constexpr int waves = fact_block / wave_size;
    static_assert(waves * bin_wave >= bin_lds, "the images of the waves hold the image of the workgroup");
    __shared__ double image[waves * bin_wave];
    const int wave = threadIdx.x / wave_size, lane = threadIdx.x % wave_size;
    for (int lvl = first_level; lvl < last_level; ++lvl) {
        const int first = level_start[lvl], last = level_start[lvl + 1];
        // the rows of at most bin_wave entries: a wave each
        for (int pos = first + wave; pos < last; pos += waves) {
            const int row = perm[pos];
            if (bin_of(rows.length(row)) == 2) continue;
            rows.template row<wave_size, false, true>(lane, row, image + wave * bin_wave,
                                                      products_from<Rows>(wave * wave_size), wave_meet{});
            wave_meet{}();
        }
        // the longer ones, if the level has any: the workgroup, one after the other (the images are shared)
        if (level_longest[lvl] > bin_wave) {
            __syncthreads();
            for (int pos = first; pos < last; ++pos) {
                const int row = perm[pos];
                if (bin_of(rows.length(row)) != 2) continue;
                block_row<Rows, true>(rows, row, image, products_from<Rows>(0));
                __syncthreads();
            }
        }
        __threadfence();
        __syncthreads();
    }
}

// ---- the host side of the frame ------------------------------------------------------------------------------
// the launches of an analysed workspace
struct schedule {
    analysis_header header;
    std::vector<segment> segments;
    const int32_t* perm;
    const int32_t* level_start;
    const int32_t* level_longest;
};

// Reads the workspace of gkomi_ilu_analyse_i32 at `ws` (the caller has checked its size).  GKOMI_EINVAL: no
// analysis, a failed one (missing diagonal, unsorted row), or one of another n.  A sweep that keeps a header of
// its own in front of its workspace has it fetched in the same round trip (outer_bytes of `outer` to
// `outer_header`) and checks it itself.
inline int load_schedule(hipStream_t stream, const char* ws, int64_t n, schedule* out, const void* outer = nullptr,
                         void* outer_header = nullptr, size_t outer_bytes = 0)
{
    analysis_header& h = out->header;
    if (outer != nullptr) {
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(outer_header, outer, outer_bytes, hipMemcpyDeviceToHost, stream)));
    }
    GKOMI_TRY(static_cast<int>(hipMemcpyAsync(&h, ws, sizeof(h), hipMemcpyDeviceToHost, stream)));
    GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
    if (h.magic != ws_magic || h.n != n || h.nsegments < 0 || h.nsegments > n) return GKOMI_EINVAL;
    const analysis_layout l = make_layout(n);
    out->segments.resize(static_cast<size_t>(h.nsegments));
    if (h.nsegments > 0) {
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(out->segments.data(), ws + l.segments,
                                                  sizeof(segment) * out->segments.size(), hipMemcpyDeviceToHost, stream)));
        GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
    }
    out->perm = reinterpret_cast<const int32_t*>(ws + l.perm);
    out->level_start = reinterpret_cast<const int32_t*>(ws + l.level_start);
    out->level_longest = reinterpret_cast<const int32_t*>(ws + l.level_longest);
    return GKOMI_SUCCESS;
}

// the launches of `s` for the policy Rows{fields...}
template <class Rows, class... Fields>
int launch_schedule(hipStream_t stream, const schedule& s, Fields... fields)
{
    for (const segment& sg : s.segments) {
        if (sg.kind == 1) {
            hipLaunchKernelGGL((run_kernel<Rows, Fields...>), dim3(1), dim3(fact_block), 0, stream, s.perm, s.level_start,
                               s.level_longest, sg.first, sg.last, fields...);
            continue;
        }
        const int64_t count = sg.last - sg.first;
        // one launch per bin the level holds rows of
        if (sg.bins & 1) {
            hipLaunchKernelGGL((level_kernel<Rows, short_width, bin_short, 0, Fields...>),
                               dim3(grid_for(count, fact_block / short_width, max_level_grid)), dim3(fact_block), 0, stream,
                               s.perm, sg.first, sg.last, fields...);
        }
        if (sg.bins & 2) {
            hipLaunchKernelGGL((level_kernel<Rows, wave_size, bin_wave, 1, Fields...>),
                               dim3(grid_for(count, fact_block / wave_size, max_level_grid)), dim3(fact_block), 0, stream,
                               s.perm, sg.first, sg.last, fields...);
        }
        if (sg.bins & 4) {
            hipLaunchKernelGGL((level_block_kernel<Rows, Fields...>), dim3(grid_for(count, 1, max_level_grid)),
                               dim3(fact_block), 0, stream, s.perm, sg.first, sg.last, fields...);
        }
    }
    return check_launch();
}
#endif

// what gkomi_ilu_tuning, gkomi_par_ilut_tuning and gkomi_par_ict_tuning report
inline void fill_tuning(int64_t* host_out)
{
    if (host_out == nullptr) return;
    host_out[0] = bin_short;
    host_out[1] = bin_wave;
    host_out[2] = bin_lds;
    host_out[3] = narrow_level_rows;
}

}  // namespace fact
}  // namespace gkomi
