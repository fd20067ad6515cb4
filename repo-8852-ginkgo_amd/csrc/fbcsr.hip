// Fbcsr<double, int32> for gfx950: SpMV, conversions, transpose, sort, diagonal.  Replaces
// gko::kernels::hip::fbcsr::* (core/matrix/fbcsr_kernels.hpp; the HIP backend's spmv is a vendor bsrmv call,
// hip/matrix/fbcsr_kernels.hip.cpp:164,222) and csr::convert_to_fbcsr, all bit-identical to the loops of
// reference/matrix/fbcsr_kernels.cpp and reference/matrix/csr_kernels.cpp:464-530.
//
// Layout: row_ptrs[nbrows + 1], col_idxs[nbnz] (block columns), values[nbnz * bs * bs]; a block is column-major,
// entry (ib, jb) of block z at z * bs^2 + ib + jb * bs (acc::block_col_major).
//
// SpMV (bs <= 16): the row-cut LDS design of the float CSR kernel on blocks.  A workgroup of 256 threads owns
// 256 / bs block rows, i.e. at most 256 scalar rows, one thread each, and walks the blocks of these rows in tiles of
// floor(2046 / bs^2) blocks.  Per tile every lane loads up to four aligned 16-byte pairs of the value stream in
// storage order (the first and the last value of a tile may be half of a pair: bs^2 is odd for bs = 3, 7, and the
// array itself may start on an odd 8 bytes), multiplies each value by b[col * bs + jb] -- gathers come in runs of bs
// contiguous values -- and parks the product in LDS.  After the barrier the thread of a scalar row adds its products
// in (z, jb) order to the sum it carries in a register across tiles, so a block row may be of any length and the
// order of the additions is the storage order, sorted columns or not.  No FMA (-ffp-contract=off), no MFMA.
// LDS image: block z of the tile at z * pitch + ib + jb * bs with pitch = bs^2 | 1.  The write is contiguous across
// lanes; the reading lanes differ in (block row, ib), and with the natural pitch bs^2 = 4, 16, 64 the block rows of a
// half-wave would start on multiples of 4 or 16 doubles = the same few banks; an odd pitch spreads them over all 32
// (8-byte) banks whatever the row lengths.  20 KB per workgroup: eight workgroups per CU.
// bs > 16: a block column is >= 136 contiguous bytes, one thread per scalar row reads it straight from memory.
// Bytes: (8 bs^2 + 4) per block + 4 per block row + 8 per row of c + the gathered part of b.
#include "common.hpp"
#include "sort_scan.hpp"

#include <climits>

namespace gkomi {
namespace {

constexpr int block = 256;
constexpr int tile_elems = 2046;   // + 2 halves of the pairs at its ends = 4 pairs for each of 256 lanes
constexpr int lds_doubles = 2560;  // max over bs <= 16 of floor(2046 / bs^2) * (bs^2 | 1): 511 * 5 at bs = 2
constexpr int lds_max_bs = 16;

template <int BS, bool Advanced>
__global__ __launch_bounds__(block) void fbcsr_spmv_kernel(
    int64_t nbrows, int bs_rt, const int32_t* __restrict__ row_ptrs, const int32_t* __restrict__ col_idxs,
    const double* __restrict__ vals, int misalign, const double* __restrict__ b, int64_t b_stride,
    double* __restrict__ c, int64_t c_stride, const double* __restrict__ alpha_p, const double* __restrict__ beta_p)
{
    const int bs = BS ? BS : bs_rt;
    const int bs2 = bs * bs;
    const int pitch = bs2 | 1;
    const int rows_per_wg = block / bs;
    const int tb = tile_elems / bs2;
    __shared__ double prod[lds_doubles];
    const int tid = threadIdx.x;
    b += blockIdx.y;
    c += blockIdx.y;
    double alpha = 1.0, beta = 0.0;
    if (Advanced) {
        alpha = alpha_p[0];
        beta = beta_p[0];
    }
    const int64_t first = blockIdx.x * static_cast<int64_t>(rows_per_wg);
    const int64_t last = min(first + rows_per_wg, nbrows);
    const int64_t z_begin = row_ptrs[first], z_end = row_ptrs[last];
    // the scalar row of this thread
    const int lr = tid / bs, ib = tid - lr * bs;
    const bool owner = first + lr < last;
    int64_t my_lo = 0, my_hi = 0, row = 0;
    double acc = 0.0;
    if (owner) {
        my_lo = row_ptrs[first + lr];
        my_hi = row_ptrs[first + lr + 1];
        row = (first + lr) * bs + ib;
        if (Advanced) acc = c[row * c_stride] * beta;
    }
    for (int64_t zt = z_begin; zt < z_end; zt += tb) {
        const int64_t zt_end = min(zt + tb, z_end);
        const int64_t e_begin = zt * bs2, e_end = zt_end * bs2;
        // pairs are counted from the 16-byte boundary at or below vals: element e sits in slot e + misalign
        const int64_t q0 = (e_begin + misalign) >> 1;
        double v[4][2];
        bool ok[4][2];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t e0 = 2 * (q0 + u * block + tid) - misalign;
            ok[u][0] = e0 >= e_begin && e0 < e_end;
            ok[u][1] = e0 + 1 >= e_begin && e0 + 1 < e_end;
            if (ok[u][0] && ok[u][1]) {
                const double2 p = *reinterpret_cast<const double2*>(vals + e0);
                v[u][0] = p.x;
                v[u][1] = p.y;
            } else {
                v[u][0] = ok[u][0] ? vals[e0] : 0.0;
                v[u][1] = ok[u][1] ? vals[e0 + 1] : 0.0;
            }
        }
        int at[4][2];
        double x[4][2];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                at[u][h] = 0;
                x[u][h] = 0.0;
                if (ok[u][h]) {
                    const int loc = static_cast<int>(2 * (q0 + u * block + tid) - misalign + h - e_begin);
                    const int zl = loc / bs2;
                    const int rem = loc - zl * bs2;
                    const int jb = rem / bs;
                    const int64_t col = col_idxs[zt + zl];
                    at[u][h] = zl * pitch + rem;
                    x[u][h] = b[(col * bs + jb) * b_stride];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (ok[u][h]) prod[at[u][h]] = Advanced ? (alpha * v[u][h]) * x[u][h] : v[u][h] * x[u][h];
            }
        }
        __syncthreads();
        if (owner) {
            const int64_t lo = max(my_lo, zt), hi = min(my_hi, zt_end);
            for (int64_t z = lo; z < hi; ++z) {
                const double* p = prod + static_cast<int>(z - zt) * pitch + ib;
                if (BS) {
#pragma unroll
                    for (int jb = 0; jb < (BS ? BS : 1); ++jb) acc += p[jb * BS];
                } else {
                    for (int jb = 0; jb < bs; ++jb) acc += p[jb * bs];
                }
            }
        }
        __syncthreads();
    }
    if (owner) c[row * c_stride] = acc;
}

// bs > lds_max_bs: one thread per scalar row, the block column (bs contiguous values) read by bs adjacent lanes
template <bool Advanced>
__global__ __launch_bounds__(block) void fbcsr_spmv_direct_kernel(
    int64_t nrows, int bs, const int32_t* __restrict__ row_ptrs, const int32_t* __restrict__ col_idxs,
    const double* __restrict__ vals, const double* __restrict__ b, int64_t b_stride, double* __restrict__ c,
    int64_t c_stride, const double* __restrict__ alpha_p, const double* __restrict__ beta_p)
{
    b += blockIdx.y;
    c += blockIdx.y;
    double alpha = 1.0, beta = 0.0;
    if (Advanced) {
        alpha = alpha_p[0];
        beta = beta_p[0];
    }
    const int64_t bs2 = static_cast<int64_t>(bs) * bs;
    for (int64_t row = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; row < nrows;
         row += static_cast<int64_t>(gridDim.x) * block) {
        const int64_t brow = row / bs;
        const int ib = static_cast<int>(row - brow * bs);
        double acc = Advanced ? c[row * c_stride] * beta : 0.0;
        for (int64_t z = row_ptrs[brow]; z < row_ptrs[brow + 1]; ++z) {
            const int64_t col = col_idxs[z];
            const double* v = vals + z * bs2 + ib;
            for (int jb = 0; jb < bs; ++jb) {
                const double x = b[(col * bs + jb) * b_stride];
                acc += Advanced ? (alpha * v[static_cast<int64_t>(jb) * bs]) * x : v[static_cast<int64_t>(jb) * bs] * x;
            }
        }
        c[row * c_stride] = acc;
    }
}

template <int BS>
void launch_lds(hipStream_t s, dim3 grid, int64_t nbrows, int bs, const int32_t* row_ptrs, const int32_t* col_idxs,
                const double* vals, const double* b, int64_t b_stride, double* c, int64_t c_stride,
                const double* alpha, const double* beta)
{
    const int misalign = static_cast<int>((reinterpret_cast<uintptr_t>(vals) >> 3) & 1);
    if (alpha != nullptr) {
        hipLaunchKernelGGL((fbcsr_spmv_kernel<BS, true>), grid, dim3(block), 0, s, nbrows, bs, row_ptrs, col_idxs, vals,
                           misalign, b, b_stride, c, c_stride, alpha, beta);
    } else {
        hipLaunchKernelGGL((fbcsr_spmv_kernel<BS, false>), grid, dim3(block), 0, s, nbrows, bs, row_ptrs, col_idxs, vals,
                           misalign, b, b_stride, c, c_stride, alpha, beta);
    }
}

// index of the segment of ptrs[0 .. n] that holds x: the r with ptrs[r] <= x < ptrs[r + 1] (empty segments skipped)
__device__ __forceinline__ int64_t segment_of(const int32_t* __restrict__ ptrs, int64_t n, int64_t x)
{
    int64_t lo = 0, hi = n + 1;  // first j in [0, n] with ptrs[j] > x
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ptrs[mid] > x) {
            hi = mid;
        } else {
            lo = mid + 1;
        }
    }
    return lo - 1;
}

// ---- csr -> fbcsr ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(block) void block_keys_kernel(int64_t nrows, int bs, int64_t nbcols,
                                                          const int32_t* __restrict__ row_ptrs,
                                                          const int32_t* __restrict__ col_idxs,
                                                          uint64_t* __restrict__ keys, uint32_t* __restrict__ src)
{
    for (int64_t row = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; row < nrows;
         row += static_cast<int64_t>(gridDim.x) * block) {
        const uint64_t brow = static_cast<uint64_t>(row / bs);
        for (int64_t nz = row_ptrs[row]; nz < row_ptrs[row + 1]; ++nz) {
            keys[nz] = brow * static_cast<uint64_t>(nbcols) + static_cast<uint64_t>(col_idxs[nz] / bs);
            src[nz] = static_cast<uint32_t>(nz);
        }
    }
}

__global__ __launch_bounds__(block) void block_heads_kernel(int64_t n, const uint64_t* __restrict__ keys,
                                                           int32_t* __restrict__ head)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * block) {
        head[i] = i == 0 || keys[i] != keys[i - 1] ? 1 : 0;
    }
}

// "set row pointers by jumps in block row index" (csr_kernels.cpp:497-522): the entry that opens block row R
// writes the pointers of R and of the empty block rows in front of it, the last entry those behind it
__global__ __launch_bounds__(block) void block_row_ptrs_kernel(int64_t n, int64_t nbrows, int64_t nbcols,
                                                              const uint64_t* __restrict__ keys,
                                                              const int32_t* __restrict__ head,
                                                              const int32_t* __restrict__ before,
                                                              int32_t* __restrict__ out_row_ptrs)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * block) {
        const int64_t brow = static_cast<int64_t>(keys[i] / static_cast<uint64_t>(nbcols));
        const int64_t prev = i == 0 ? -1 : static_cast<int64_t>(keys[i - 1] / static_cast<uint64_t>(nbcols));
        for (int64_t r = prev + 1; r <= brow; ++r) out_row_ptrs[r] = before[i];
        if (i == n - 1) {
            for (int64_t r = brow + 1; r <= nbrows; ++r) out_row_ptrs[r] = before[i] + head[i];
        }
    }
}

__global__ __launch_bounds__(block) void block_fill_kernel(int64_t n, int64_t nrows, int bs, int64_t nbcols,
                                                          const int32_t* __restrict__ row_ptrs,
                                                          const int32_t* __restrict__ col_idxs,
                                                          const double* __restrict__ vals,
                                                          const uint64_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ src,
                                                          const int32_t* __restrict__ head,
                                                          const int32_t* __restrict__ before,
                                                          int32_t* __restrict__ out_col_idxs,
                                                          double* __restrict__ out_vals)
{
    const int64_t bs2 = static_cast<int64_t>(bs) * bs;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * block) {
        const int64_t z = before[i] + head[i] - 1;
        const int64_t nz = src[i];
        if (head[i]) out_col_idxs[z] = static_cast<int32_t>(keys[i] % static_cast<uint64_t>(nbcols));
        const int64_t row = segment_of(row_ptrs, nrows, nz);
        out_vals[z * bs2 + row % bs + static_cast<int64_t>(col_idxs[nz] % bs) * bs] = vals[nz];
    }
}

// ---- fbcsr -> csr / dense ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(block) void to_csr_ptrs_kernel(int64_t nbrows, int bs, const int32_t* __restrict__ brow_ptrs,
                                                           int32_t* __restrict__ row_ptrs)
{
    const int64_t nrows = nbrows * bs;
    for (int64_t row = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; row <= nrows;
         row += static_cast<int64_t>(gridDim.x) * block) {
        if (row == nrows) {
            row_ptrs[row] = brow_ptrs[nbrows] * bs * bs;
        } else {
            const int64_t brow = row / bs;
            const int ib = static_cast<int>(row - brow * bs);
            row_ptrs[row] = brow_ptrs[brow] * bs * bs + (brow_ptrs[brow + 1] - brow_ptrs[brow]) * bs * ib;
        }
    }
}

// one thread per stored value; Dense = false: csr, true: result(row, col) of a row-major dense matrix
template <bool Dense>
__global__ __launch_bounds__(block) void scatter_values_kernel(int64_t nbrows, int64_t nelems, int bs,
                                                              const int32_t* __restrict__ brow_ptrs,
                                                              const int32_t* __restrict__ bcol_idxs,
                                                              const double* __restrict__ bvals,
                                                              int32_t* __restrict__ col_idxs,
                                                              double* __restrict__ out, int64_t stride)
{
    const int64_t bs2 = static_cast<int64_t>(bs) * bs;
    for (int64_t e = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; e < nelems;
         e += static_cast<int64_t>(gridDim.x) * block) {
        const int64_t z = e / bs2;
        const int rem = static_cast<int>(e - z * bs2);
        const int jb = rem / bs, ib = rem - jb * bs;
        const int64_t brow = segment_of(brow_ptrs, nbrows, z);
        const int64_t col = static_cast<int64_t>(bcol_idxs[z]) * bs + jb;
        if (Dense) {
            out[(brow * bs + ib) * stride + col] = bvals[e];
        } else {
            const int64_t start = brow_ptrs[brow], len = brow_ptrs[brow + 1] - start;
            const int64_t inz = start * bs2 + len * bs * ib + (z - start) * bs + jb;
            out[inz] = bvals[e];
            col_idxs[inz] = static_cast<int32_t>(col);
        }
    }
}

// ---- transpose / sort / diagonal ---------------------------------------------------------------------------------
__global__ __launch_bounds__(block) void iota_kernel(int64_t n, uint32_t* __restrict__ out)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * block) {
        out[i] = static_cast<uint32_t>(i);
    }
}

// t_row_ptrs[c] = number of blocks with a column below c = first position of c in the sorted columns
__global__ __launch_bounds__(block) void lower_bounds_kernel(int64_t nbcols, int64_t n,
                                                            const uint32_t* __restrict__ sorted_cols,
                                                            int32_t* __restrict__ ptrs)
{
    for (int64_t c = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; c <= nbcols;
         c += static_cast<int64_t>(gridDim.x) * block) {
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (static_cast<int64_t>(sorted_cols[mid]) < c) {
                lo = mid + 1;
            } else {
                hi = mid;
            }
        }
        ptrs[c] = static_cast<int32_t>(lo);
    }
}

__global__ __launch_bounds__(block) void transpose_blocks_kernel(int64_t nbrows, int64_t nelems, int bs,
                                                                const int32_t* __restrict__ row_ptrs,
                                                                const double* __restrict__ vals,
                                                                const uint32_t* __restrict__ src,
                                                                int32_t* __restrict__ t_col_idxs,
                                                                double* __restrict__ t_vals)
{
    const int64_t bs2 = static_cast<int64_t>(bs) * bs;
    for (int64_t e = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; e < nelems;
         e += static_cast<int64_t>(gridDim.x) * block) {
        const int64_t dest = e / bs2;
        const int rem = static_cast<int>(e - dest * bs2);
        const int jb = rem / bs, ib = rem - jb * bs;
        const int64_t z = src[dest];
        t_vals[e] = vals[z * bs2 + jb + static_cast<int64_t>(ib) * bs];
        if (rem == 0) t_col_idxs[dest] = static_cast<int32_t>(segment_of(row_ptrs, nbrows, z));
    }
}

// one thread per block row: insertion sort of the columns, perm[z] = where block z comes from
__global__ __launch_bounds__(block) void sort_block_rows_kernel(int64_t nbrows, const int32_t* __restrict__ row_ptrs,
                                                               int32_t* __restrict__ cols, int32_t* __restrict__ perm)
{
    for (int64_t row = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; row < nbrows;
         row += static_cast<int64_t>(gridDim.x) * block) {
        const int32_t begin = row_ptrs[row], end = row_ptrs[row + 1];
        for (int32_t i = begin; i < end; ++i) {
            const int32_t c = cols[i];
            int32_t j = i - 1;
            while (j >= begin && cols[j] > c) {
                cols[j + 1] = cols[j];
                perm[j + 1] = perm[j];
                --j;
            }
            cols[j + 1] = c;
            perm[j + 1] = i;
        }
    }
}

__global__ __launch_bounds__(block) void permute_blocks_kernel(int64_t nelems, int bs, const int32_t* __restrict__ perm,
                                                              const double* __restrict__ old_vals,
                                                              double* __restrict__ vals)
{
    const int64_t bs2 = static_cast<int64_t>(bs) * bs;
    for (int64_t e = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; e < nelems;
         e += static_cast<int64_t>(gridDim.x) * block) {
        const int64_t z = e / bs2;
        vals[e] = old_vals[perm[z] * bs2 + (e - z * bs2)];
    }
}

__global__ __launch_bounds__(block) void block_diagonal_kernel(int64_t nbdim, int bs, const int32_t* __restrict__ row_ptrs,
                                                              const int32_t* __restrict__ col_idxs,
                                                              const double* __restrict__ vals, double* __restrict__ diag)
{
    const int64_t bs2 = static_cast<int64_t>(bs) * bs;
    for (int64_t brow = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; brow < nbdim;
         brow += static_cast<int64_t>(gridDim.x) * block) {
        for (int64_t z = row_ptrs[brow]; z < row_ptrs[brow + 1]; ++z) {
            if (col_idxs[z] == brow) {
                for (int ib = 0; ib < bs; ++ib) diag[brow * bs + ib] = vals[z * bs2 + ib + static_cast<int64_t>(ib) * bs];
                break;
            }
        }
    }
}

int bits_of(uint64_t x)
{
    int bits = 0;
    while (bits < 64 && (x >> bits) != 0) ++bits;
    return bits;
}

// workspace of csr -> fbcsr: what the count call leaves for the fill call comes first
struct convert_ws {
    uint64_t* keys;
    uint32_t* src;
    int32_t* head;
    int32_t* before;
    uint64_t* keys_in;
    uint32_t* src_in;
    void* sort_ws;
    size_t sort_bytes;
    void* scan_ws;
    size_t scan_bytes;
    size_t total;
};

convert_ws carve_convert(void* base, int64_t nnz)
{
    const size_t n = static_cast<size_t>(nnz > 0 ? nnz : 1);
    char* p = static_cast<char*>(base);
    size_t at = 0;
    convert_ws w{};
    auto take = [&](size_t bytes) {
        char* r = p + at;
        at += align256(bytes);
        return static_cast<void*>(r);
    };
    w.keys = static_cast<uint64_t*>(take(8 * n));
    w.src = static_cast<uint32_t*>(take(4 * n));
    w.head = static_cast<int32_t*>(take(4 * n));
    w.before = static_cast<int32_t*>(take(4 * n));
    w.keys_in = static_cast<uint64_t*>(take(8 * n));
    w.src_in = static_cast<uint32_t*>(take(4 * n));
    w.sort_bytes = radix_sort_workspace_bytes(nnz, 8, true);
    w.sort_ws = take(w.sort_bytes);
    w.scan_bytes = scan_workspace_bytes(nnz);
    w.scan_ws = take(w.scan_bytes);
    w.total = at;
    return w;
}

}  // namespace
}  // namespace gkomi

using namespace gkomi;

extern "C" int gkomi_fbcsr_spmv_geometry(int64_t bs, int64_t* host_block_rows_per_workgroup,
                                         int64_t* host_blocks_per_tile)
{
    if (bs < 1 || bs > INT32_MAX) return GKOMI_EINVAL;
    const bool lds = bs <= lds_max_bs;
    if (host_block_rows_per_workgroup != nullptr) *host_block_rows_per_workgroup = lds ? block / bs : ceildiv(block, bs);
    if (host_blocks_per_tile != nullptr) *host_blocks_per_tile = lds ? tile_elems / (bs * bs) : 0;
    return GKOMI_SUCCESS;
}

extern "C" int gkomi_fbcsr_spmv_f64_i32(gkomi_stream_t s, int64_t nbrows, int64_t nbcols, int64_t bs, int64_t nbnz,
                                        const int32_t* row_ptrs, const int32_t* col_idxs, const double* vals,
                                        const double* b, int64_t b_stride, int64_t nrhs, double* c, int64_t c_stride,
                                        const double* alpha, const double* beta)
{
    if (bs < 1 || nbrows < 0 || nbcols < 0 || nrhs < 0 || nbnz < 0) return GKOMI_EINVAL;
    if ((alpha == nullptr) != (beta == nullptr)) return GKOMI_EINVAL;
    if (nbrows == 0 || nrhs == 0) return GKOMI_SUCCESS;
    if (row_ptrs == nullptr || c == nullptr || b_stride < nrhs || c_stride < nrhs) return GKOMI_EINVAL;
    if (nbnz > 0 && (col_idxs == nullptr || vals == nullptr || b == nullptr)) return GKOMI_EINVAL;
    if (reinterpret_cast<uintptr_t>(vals) & 7) return GKOMI_EINVAL;
    if (nrhs > 65535 || nbnz > INT32_MAX) return GKOMI_ENOTSUPPORTED;
    if (bs > INT32_MAX / bs || nbrows > INT64_MAX / bs) return GKOMI_ENOTSUPPORTED;
    hipStream_t stream = to_stream(s);
    const int ibs = static_cast<int>(bs);
    if (bs > lds_max_bs) {
        dim3 grid(grid_for(nbrows * bs, block, 1 << 20), static_cast<unsigned>(nrhs));
        if (alpha != nullptr) {
            hipLaunchKernelGGL(fbcsr_spmv_direct_kernel<true>, grid, dim3(block), 0, stream, nbrows * bs, ibs, row_ptrs,
                               col_idxs, vals, b, b_stride, c, c_stride, alpha, beta);
        } else {
            hipLaunchKernelGGL(fbcsr_spmv_direct_kernel<false>, grid, dim3(block), 0, stream, nbrows * bs, ibs, row_ptrs,
                               col_idxs, vals, b, b_stride, c, c_stride, alpha, beta);
        }
        return check_launch();
    }
    const int64_t nwg = ceildiv(nbrows, block / bs);
    if (nwg > INT32_MAX) return GKOMI_ENOTSUPPORTED;
    dim3 grid(static_cast<unsigned>(nwg), static_cast<unsigned>(nrhs));
    switch (ibs) {  // the block sizes the reference compiles (core/base/block_sizes.hpp:56); the rest: same code, bs at run time
    case 2: launch_lds<2>(stream, grid, nbrows, ibs, row_ptrs, col_idxs, vals, b, b_stride, c, c_stride, alpha, beta); break;
    case 3: launch_lds<3>(stream, grid, nbrows, ibs, row_ptrs, col_idxs, vals, b, b_stride, c, c_stride, alpha, beta); break;
    case 4: launch_lds<4>(stream, grid, nbrows, ibs, row_ptrs, col_idxs, vals, b, b_stride, c, c_stride, alpha, beta); break;
    case 7: launch_lds<7>(stream, grid, nbrows, ibs, row_ptrs, col_idxs, vals, b, b_stride, c, c_stride, alpha, beta); break;
    default: launch_lds<0>(stream, grid, nbrows, ibs, row_ptrs, col_idxs, vals, b, b_stride, c, c_stride, alpha, beta); break;
    }
    return check_launch();
}

extern "C" int gkomi_fbcsr_matrix_apply_cb(void* ctx_, gkomi_stream_t s, int64_t nrhs, const double* alpha,
                                           const double* b, int64_t b_stride, const double* beta, double* c,
                                           int64_t c_stride)
{
    const gkomi_fbcsr_ctx* m = static_cast<const gkomi_fbcsr_ctx*>(ctx_);
    if (m == nullptr) return GKOMI_EINVAL;
    return gkomi_fbcsr_spmv_f64_i32(s, m->nbrows, m->nbcols, m->bs, m->nbnz, m->row_ptrs, m->col_idxs, m->vals, b,
                                    b_stride, nrhs, c, c_stride, alpha, beta);
}

extern "C" size_t gkomi_csr_convert_to_fbcsr_workspace_bytes(int64_t nnz)
{
    if (nnz < 0) return 0;
    return carve_convert(nullptr, nnz).total;
}

extern "C" int gkomi_csr_convert_to_fbcsr_i32(gkomi_stream_t s, int64_t nrows, int64_t ncols, int64_t bs, int64_t nnz,
                                              const int32_t* row_ptrs, const int32_t* col_idxs, const double* vals,
                                              int32_t* out_row_ptrs, int32_t* out_col_idxs, double* out_vals,
                                              int64_t* host_nbnz, void* workspace, size_t workspace_bytes)
{
    if (bs < 1 || nrows < 0 || ncols < 0 || nnz < 0 || host_nbnz == nullptr) return GKOMI_EINVAL;
    if (nrows % bs != 0 || ncols % bs != 0) return GKOMI_EINVAL;  // Fbcsr's constructor (core/matrix/fbcsr.cpp)
    if ((out_col_idxs == nullptr) != (out_vals == nullptr)) return GKOMI_EINVAL;
    if (nnz > INT32_MAX || bs > INT32_MAX / bs) return GKOMI_ENOTSUPPORTED;
    const bool count = out_col_idxs == nullptr;
    const int64_t nbrows = nrows / bs, nbcols = ncols / bs;
    hipStream_t stream = to_stream(s);
    if (nnz == 0) {
        if (!count) return GKOMI_SUCCESS;
        if (out_row_ptrs == nullptr) return GKOMI_EINVAL;
        *host_nbnz = 0;
        return static_cast<int>(hipMemsetAsync(out_row_ptrs, 0, sizeof(int32_t) * (nbrows + 1), stream));
    }
    if (row_ptrs == nullptr || col_idxs == nullptr) return GKOMI_EINVAL;
    const convert_ws w = carve_convert(workspace, nnz);
    if (workspace == nullptr || workspace_bytes < w.total) return GKOMI_EWORKSPACE;
    const dim3 grid_nnz(grid_for(nnz, block, 1 << 16));
    const int ibs = static_cast<int>(bs);
    if (count) {
        if (out_row_ptrs == nullptr) return GKOMI_EINVAL;
        hipLaunchKernelGGL(block_keys_kernel, dim3(grid_for(nrows, block, 1 << 16)), dim3(block), 0, stream, nrows, ibs,
                           nbcols, row_ptrs, col_idxs, w.keys_in, w.src_in);
        GKOMI_TRY(check_launch());
        // "sort by block in row-major order" (:489-491); entries of one block keep their order, which the
        // scatter below does not depend on
        const int end_bit = bits_of(static_cast<uint64_t>(nbrows) * static_cast<uint64_t>(nbcols));
        GKOMI_TRY(radix_sort_u64(stream, nnz, w.keys_in, w.keys, w.src_in, w.src, end_bit, w.sort_ws, w.sort_bytes));
        hipLaunchKernelGGL(block_heads_kernel, grid_nnz, dim3(block), 0, stream, nnz, w.keys, w.head);
        GKOMI_TRY(check_launch());
        GKOMI_TRY(exclusive_sum_i32(stream, w.head, w.before, nnz, w.scan_ws, w.scan_bytes));
        hipLaunchKernelGGL(block_row_ptrs_kernel, grid_nnz, dim3(block), 0, stream, nnz, nbrows, nbcols, w.keys, w.head,
                           w.before, out_row_ptrs);
        GKOMI_TRY(check_launch());
        int32_t tail[2] = {0, 0};
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(&tail[0], w.before + (nnz - 1), sizeof(int32_t), hipMemcpyDeviceToHost, stream)));
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(&tail[1], w.head + (nnz - 1), sizeof(int32_t), hipMemcpyDeviceToHost, stream)));
        GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
        *host_nbnz = static_cast<int64_t>(tail[0]) + tail[1];
        return GKOMI_SUCCESS;
    }
    if (vals == nullptr || *host_nbnz < 0) return GKOMI_EINVAL;
    // "entries not present in a touched block are explicit zeros" (value_vec.resize, :510)
    GKOMI_TRY(static_cast<int>(hipMemsetAsync(out_vals, 0, sizeof(double) * static_cast<size_t>(*host_nbnz) * bs * bs, stream)));
    hipLaunchKernelGGL(block_fill_kernel, grid_nnz, dim3(block), 0, stream, nnz, nrows, ibs, nbcols, row_ptrs, col_idxs,
                       vals, w.keys, w.src, w.head, w.before, out_col_idxs, out_vals);
    return check_launch();
}

extern "C" int gkomi_fbcsr_convert_to_csr_i32(gkomi_stream_t s, int64_t nbrows, int64_t bs, int64_t nbnz,
                                              const int32_t* row_ptrs, const int32_t* col_idxs, const double* vals,
                                              int32_t* csr_row_ptrs, int32_t* csr_col_idxs, double* csr_vals)
{
    if (bs < 1 || nbrows < 0 || nbnz < 0) return GKOMI_EINVAL;
    if (bs > INT32_MAX / bs || nbnz > INT32_MAX / (bs * bs) || nbrows > INT32_MAX / bs) return GKOMI_ENOTSUPPORTED;
    if (csr_row_ptrs == nullptr || (nbrows > 0 && row_ptrs == nullptr)) return GKOMI_EINVAL;
    if (nbnz > 0 && (col_idxs == nullptr || vals == nullptr || csr_col_idxs == nullptr || csr_vals == nullptr)) return GKOMI_EINVAL;
    hipStream_t stream = to_stream(s);
    if (nbrows == 0) return static_cast<int>(hipMemsetAsync(csr_row_ptrs, 0, sizeof(int32_t), stream));
    hipLaunchKernelGGL(to_csr_ptrs_kernel, dim3(grid_for(nbrows * bs + 1, block, 1 << 16)), dim3(block), 0, stream, nbrows,
                       static_cast<int>(bs), row_ptrs, csr_row_ptrs);
    GKOMI_TRY(check_launch());
    if (nbnz == 0) return GKOMI_SUCCESS;
    const int64_t nelems = nbnz * bs * bs;
    hipLaunchKernelGGL(scatter_values_kernel<false>, dim3(grid_for(nelems, block, 1 << 16)), dim3(block), 0, stream, nbrows,
                       nelems, static_cast<int>(bs), row_ptrs, col_idxs, vals, csr_col_idxs, csr_vals, int64_t{0});
    return check_launch();
}

extern "C" int gkomi_fbcsr_fill_in_dense_f64_i32(gkomi_stream_t s, int64_t nbrows, int64_t nbcols, int64_t bs,
                                                 int64_t nbnz, const int32_t* row_ptrs, const int32_t* col_idxs,
                                                 const double* vals, double* result, int64_t result_stride)
{
    if (bs < 1 || nbrows < 0 || nbcols < 0 || nbnz < 0) return GKOMI_EINVAL;
    if (bs > INT32_MAX / bs || nbnz > INT64_MAX / (bs * bs) || nbcols > INT64_MAX / bs) return GKOMI_ENOTSUPPORTED;
    if (nbrows == 0 || nbnz == 0) return GKOMI_SUCCESS;
    if (row_ptrs == nullptr || col_idxs == nullptr || vals == nullptr || result == nullptr || result_stride < nbcols * bs) return GKOMI_EINVAL;
    const int64_t nelems = nbnz * bs * bs;
    hipLaunchKernelGGL(scatter_values_kernel<true>, dim3(grid_for(nelems, block, 1 << 16)), dim3(block), 0, to_stream(s), nbrows,
                       nelems, static_cast<int>(bs), row_ptrs, col_idxs, vals, static_cast<int32_t*>(nullptr), result, result_stride);
    return check_launch();
}

extern "C" size_t gkomi_fbcsr_transpose_workspace_bytes(int64_t nbnz)
{
    if (nbnz < 0) return 0;
    const size_t n = static_cast<size_t>(nbnz > 0 ? nbnz : 1);
    return 4 * align256(4 * n) + radix_sort_workspace_bytes(nbnz, 4, true);
}

extern "C" int gkomi_fbcsr_transpose_f64_i32(gkomi_stream_t s, int64_t nbrows, int64_t nbcols, int64_t bs, int64_t nbnz,
                                             const int32_t* row_ptrs, const int32_t* col_idxs, const double* vals,
                                             int32_t* t_row_ptrs, int32_t* t_col_idxs, double* t_vals, void* workspace,
                                             size_t workspace_bytes)
{
    if (bs < 1 || nbrows < 0 || nbcols < 0 || nbnz < 0 || t_row_ptrs == nullptr) return GKOMI_EINVAL;
    if (nbnz > INT32_MAX || bs > INT32_MAX / bs || nbnz > INT64_MAX / (bs * bs)) return GKOMI_ENOTSUPPORTED;
    hipStream_t stream = to_stream(s);
    if (nbnz == 0) return static_cast<int>(hipMemsetAsync(t_row_ptrs, 0, sizeof(int32_t) * (nbcols + 1), stream));
    if (row_ptrs == nullptr || col_idxs == nullptr || vals == nullptr || t_col_idxs == nullptr || t_vals == nullptr) return GKOMI_EINVAL;
    if (workspace == nullptr || workspace_bytes < gkomi_fbcsr_transpose_workspace_bytes(nbnz)) return GKOMI_EWORKSPACE;
    char* p = static_cast<char*>(workspace);
    const size_t piece = align256(4 * static_cast<size_t>(nbnz));
    uint32_t* src_in = reinterpret_cast<uint32_t*>(p);
    uint32_t* cols_sorted = reinterpret_cast<uint32_t*>(p + piece);
    uint32_t* src = reinterpret_cast<uint32_t*>(p + 2 * piece);
    void* sort_ws = p + 4 * piece;
    const size_t sort_bytes = radix_sort_workspace_bytes(nbnz, 4, true);
    const dim3 grid(grid_for(nbnz, block, 1 << 16));
    hipLaunchKernelGGL(iota_kernel, grid, dim3(block), 0, stream, nbnz, src_in);
    GKOMI_TRY(check_launch());
    // the counting order of convert_fbcsr_to_fbcsc (:332-345): within a column, blocks in storage order = a stable sort
    GKOMI_TRY(radix_sort_u32(stream, nbnz, reinterpret_cast<const uint32_t*>(col_idxs), cols_sorted, src_in, src,
                             bits_of(static_cast<uint64_t>(nbcols)), sort_ws, sort_bytes));
    hipLaunchKernelGGL(lower_bounds_kernel, dim3(grid_for(nbcols + 1, block, 1 << 16)), dim3(block), 0, stream, nbcols, nbnz,
                       cols_sorted, t_row_ptrs);
    GKOMI_TRY(check_launch());
    const int64_t nelems = nbnz * bs * bs;
    hipLaunchKernelGGL(transpose_blocks_kernel, dim3(grid_for(nelems, block, 1 << 16)), dim3(block), 0, stream, nbrows, nelems,
                       static_cast<int>(bs), row_ptrs, vals, src, t_col_idxs, t_vals);
    return check_launch();
}

extern "C" int gkomi_fbcsr_is_sorted_by_column_index_i32(gkomi_stream_t s, int64_t nbrows, const int32_t* row_ptrs,
                                                         const int32_t* col_idxs, void* workspace,
                                                         size_t workspace_bytes, int* host_is_sorted)
{
    // the same loop over block rows and block columns as csr::is_sorted_by_column_index
    return gkomi_csr_is_sorted_by_column_index_i32(s, nbrows, row_ptrs, col_idxs, workspace, workspace_bytes, host_is_sorted);
}

extern "C" size_t gkomi_fbcsr_sort_workspace_bytes(int64_t nbnz, int64_t bs)
{
    if (nbnz < 0 || bs < 1) return 0;
    const size_t n = static_cast<size_t>(nbnz > 0 ? nbnz : 1);
    return align256(4 * n) + align256(8 * n * static_cast<size_t>(bs) * static_cast<size_t>(bs));
}

extern "C" int gkomi_fbcsr_sort_by_column_index_f64_i32(gkomi_stream_t s, int64_t nbrows, int64_t bs, int64_t nbnz,
                                                        const int32_t* row_ptrs, int32_t* col_idxs, double* vals,
                                                        void* workspace, size_t workspace_bytes)
{
    if (bs < 1 || nbrows < 0 || nbnz < 0) return GKOMI_EINVAL;
    if (nbnz > INT32_MAX || bs > INT32_MAX / bs || nbnz > INT64_MAX / (bs * bs)) return GKOMI_ENOTSUPPORTED;
    if (nbrows == 0 || nbnz == 0) return GKOMI_SUCCESS;
    if (row_ptrs == nullptr || col_idxs == nullptr || vals == nullptr) return GKOMI_EINVAL;
    if (workspace == nullptr || workspace_bytes < gkomi_fbcsr_sort_workspace_bytes(nbnz, bs)) return GKOMI_EWORKSPACE;
    hipStream_t stream = to_stream(s);
    int32_t* perm = static_cast<int32_t*>(workspace);
    double* old_vals = reinterpret_cast<double*>(static_cast<char*>(workspace) + align256(4 * static_cast<size_t>(nbnz)));
    const int64_t nelems = nbnz * bs * bs;
    GKOMI_TRY(static_cast<int>(hipMemcpyAsync(old_vals, vals, sizeof(double) * nelems, hipMemcpyDeviceToDevice, stream)));
    hipLaunchKernelGGL(sort_block_rows_kernel, dim3(grid_for(nbrows, block, 1 << 16)), dim3(block), 0, stream, nbrows, row_ptrs,
                       col_idxs, perm);
    GKOMI_TRY(check_launch());
    hipLaunchKernelGGL(permute_blocks_kernel, dim3(grid_for(nelems, block, 1 << 16)), dim3(block), 0, stream, nelems,
                       static_cast<int>(bs), perm, old_vals, vals);
    return check_launch();
}

extern "C" int gkomi_fbcsr_extract_diagonal_f64_i32(gkomi_stream_t s, int64_t nbrows, int64_t nbcols, int64_t bs,
                                                    const int32_t* row_ptrs, const int32_t* col_idxs,
                                                    const double* vals, double* diag)
{
    if (bs < 1 || nbrows < 0 || nbcols < 0) return GKOMI_EINVAL;
    if (bs > INT32_MAX / bs) return GKOMI_ENOTSUPPORTED;
    const int64_t nbdim = nbrows < nbcols ? nbrows : nbcols;
    if (nbdim == 0) return GKOMI_SUCCESS;
    if (row_ptrs == nullptr || diag == nullptr) return GKOMI_EINVAL;
    hipLaunchKernelGGL(block_diagonal_kernel, dim3(grid_for(nbdim, block, 1 << 16)), dim3(block), 0, to_stream(s), nbdim,
                       static_cast<int>(bs), row_ptrs, col_idxs, vals, diag);
    return check_launch();
}
