// Dense<double> times Dense<double> and Dense::transpose for gfx950.  Replaces gko::kernels::hip::dense::simple_apply,
// apply, transpose and conj_transpose (core/matrix/dense_kernels.hpp:55-64, 225-234; the HIP backend's apply is a vendor
// gemm call, hip/matrix/dense_kernels.hip.cpp:153-205) with the sums of reference/matrix/dense_kernels.cpp:70-121:
//   simple:   c(i,j) = (+0.0) + a(i,0) b(0,j) + a(i,1) b(1,j) + ...            one chain, ascending l
//   advanced: c(i,j) = c(i,j) * beta + (alpha a(i,0)) b(0,j) + ...             beta == 0 still multiplies
// Product and sum are rounded separately (-ffp-contract=off, no fma, no MFMA: v_mfma_f64 fuses), and the chain of an
// element ends exactly at k -- a padded +0.0 product would turn a -0.0 of c * beta into +0.0.
//
// tile (n > 16): a workgroup of 256 threads owns a 64 x 64 tile of C, a thread a 4 x 4 block of it in registers.  A and B
//   go through LDS in steps of 16 values of l, double buffered: the loads of step s + 1 are in flight while step s is
//   computed, one barrier per step.  The A tile sits l-major (pitch 68 doubles: the four rows of a thread are one 32-byte
//   read, and the writes of a wave, which differ in row and in groups of four l, fall on two lanes per bank at most), the
//   B tile l-major by nature.  2 x (16 x 68 + 16 x 64) x 8 = 33 KB of LDS: four workgroups per CU.
// narrow (n <= 16): one thread per row of C with up to 16 accumulators, 256 rows per workgroup.  The rows of A arrive
//   coalesced -- 16 lanes on the 128 contiguous bytes of a row's chunk -- in an LDS image of pitch 17 (odd: the 32 rows a
//   half-wave walks start on 32 different banks), the B chunk beside it; the next chunk's loads are issued before the
//   current one is walked.  The rows of c enter (advanced) and leave through the same image, so that they too are read
//   and written lane after lane.  Bandwidth-bound on A.
// split: k is cut into chunks of `split_chunk`; chunk z's partial is the same ordered chain, from +0.0, over
//   [z L, min(k, (z + 1) L)), computed by the kernel above that the shape would get (grid = tiles x chunks) into the
//   workspace; a second kernel adds the partials to c * beta (or +0.0) in ascending z.  No atomics, no workgroup waits
//   for another, and the order depends on (m, n, k) alone.
// transpose: 64 x 64 tiles through an LDS image of pitch 65, rows of `in` read and rows of `out` written coalesced.
#include "common.hpp"

#include <climits>

namespace gkomi {
namespace {

constexpr int block = 256;
// tile kernel
constexpr int tile_m = 64, tile_n = 64, tile_k = 16;
constexpr int a_pitch = tile_m + 4;
// narrow kernel
constexpr int narrow_max_n = 16;
constexpr int narrow_rows = block, narrow_k = 16;
constexpr int narrow_pitch = narrow_k + 1;
// split
constexpr int64_t split_chunk = 2048;
// the automatic rule (profiles/dense_gemm_probe.md): split when the ordered launch has at most this many
// workgroups (half the CUs) and k is at least two chunks -- there the split was 1.8 to 50 times faster
constexpr int64_t split_max_workgroups = 128;
constexpr int64_t split_min_k = 2 * split_chunk;

enum gemm_mode { simple = 0, advanced = 1, partial_scaled = 2 };  // partial_scaled: from +0.0, a scaled by alpha

struct gemm_args {
    int64_t m, n, k;
    int64_t chunk_len;  // columns of A per chunk (k itself for an ordered launch)
    int64_t tiles;      // workgroups per chunk
    const double* a;
    int64_t a_stride;
    const double* b;
    int64_t b_stride;
    double* c;
    int64_t c_stride;
    int64_t c_chunk_stride;  // partials of chunk z start at c + z * c_chunk_stride
    const double* alpha;
    const double* beta;
};

template <int Mode>
__global__ __launch_bounds__(block) void gemm_tile_kernel(const gemm_args g)
{
    __shared__ __attribute__((aligned(32))) double as[2][tile_k * a_pitch];
    __shared__ __attribute__((aligned(32))) double bs[2][tile_k * tile_n];
    const int tid = threadIdx.x;
    const int64_t chunk = blockIdx.x / g.tiles;
    const int64_t tile = blockIdx.x - chunk * g.tiles;
    const int64_t tiles_n = (g.n + tile_n - 1) / tile_n;
    const int64_t m0 = tile / tiles_n * tile_m, n0 = tile % tiles_n * tile_n;
    const int64_t k_begin = chunk * g.chunk_len;
    const int64_t k_len = min(g.chunk_len, g.k - k_begin);
    const double* __restrict__ a = g.a + k_begin;
    const double* __restrict__ b = g.b + k_begin * g.b_stride;
    double* __restrict__ c = g.c + chunk * g.c_chunk_stride;
    double alpha = 1.0, beta = 0.0;
    if (Mode != simple) alpha = g.alpha[0];
    if (Mode == advanced) beta = g.beta[0];

    // loads: A -- row tid / 4 of the tile, four consecutive l; B -- l = tid / 16, four consecutive columns
    const int a_row = tid >> 2, a_l = (tid & 3) * 4;
    const int b_l = tid >> 4, b_col = (tid & 15) * 4;
    const bool a_row_ok = m0 + a_row < g.m;
    const double* a_src = a + (m0 + a_row) * g.a_stride + a_l;
    const double* b_src = b + b_l * g.b_stride + n0 + b_col;
    double ra[4], rb[4];
    auto load = [&](int64_t k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ra[i] = a_row_ok && k0 + a_l + i < k_len ? a_src[k0 + i] : 0.0;
            rb[i] = k0 + b_l < k_len && n0 + b_col + i < g.n ? b_src[k0 * g.b_stride + i] : 0.0;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            as[buf][(a_l + i) * a_pitch + a_row] = Mode != simple ? alpha * ra[i] : ra[i];
            bs[buf][b_l * tile_n + b_col + i] = rb[i];
        }
    };

    // the 4 x 4 block of this thread
    const int ty = tid >> 4, tx = tid & 15;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[i][j] = 0.0;
            if (Mode == advanced) {
                const int64_t row = m0 + ty * 4 + i, col = n0 + tx * 4 + j;
                if (row < g.m && col < g.n) acc[i][j] = c[row * g.c_stride + col] * beta;
            }
        }
    }

    const int64_t nsteps = (k_len + tile_k - 1) / tile_k;
    if (nsteps > 0) {
        load(0);
        store(0);
    }
    __syncthreads();
    for (int64_t s = 0; s < nsteps; ++s) {
        const int buf = static_cast<int>(s & 1);
        const bool more = s + 1 < nsteps;
        if (more) load((s + 1) * tile_k);
        const double* pa = as[buf] + ty * 4;
        const double* pb = bs[buf] + tx * 4;
        const int kk = static_cast<int>(min(static_cast<int64_t>(tile_k), k_len - s * tile_k));
        auto step = [&](int l) {
            double va[4], vb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                va[i] = pa[l * a_pitch + i];
                vb[i] = pb[l * tile_n + i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = acc[i][j] + va[i] * vb[j];
            }
        };
        if (kk == tile_k) {
#pragma unroll
            for (int l = 0; l < tile_k; ++l) step(l);
        } else {
            for (int l = 0; l < kk; ++l) step(l);  // the chain ends at k: no padded products
        }
        if (more) store(buf ^ 1);
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t row = m0 + ty * 4 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t col = n0 + tx * 4 + j;
            if (row < g.m && col < g.n) c[row * g.c_stride + col] = acc[i][j];
        }
    }
}

// NB: accumulators per thread, the next power of two at or above n; columns n .. NB - 1 are computed and dropped
template <int NB, int Mode>
__global__ __launch_bounds__(block) void gemm_narrow_kernel(const gemm_args g)
{
    __shared__ double as[narrow_rows * narrow_pitch];
    __shared__ __attribute__((aligned(16))) double bs[narrow_k * NB];
    const int tid = threadIdx.x;
    const int64_t chunk = blockIdx.x / g.tiles;
    const int64_t row0 = (blockIdx.x - chunk * g.tiles) * narrow_rows;
    const int64_t k_begin = chunk * g.chunk_len;
    const int64_t k_len = min(g.chunk_len, g.k - k_begin);
    const double* __restrict__ a = g.a + k_begin;
    const double* __restrict__ b = g.b + k_begin * g.b_stride;
    double* __restrict__ c = g.c + chunk * g.c_chunk_stride;
    double alpha = 1.0, beta = 0.0;
    if (Mode != simple) alpha = g.alpha[0];
    if (Mode == advanced) beta = g.beta[0];
    const int n = static_cast<int>(g.n);

    // loads: element e = u * 256 + tid of the 256 x 16 chunk of A is (row e / 16, l = e % 16)
    constexpr int per_thread = narrow_rows * narrow_k / block;
    const int ld_l = tid & (narrow_k - 1), ld_row = tid >> 4;  // + 16 rows per u
    const int b_l = tid / NB, b_j = tid - b_l * NB;
    double ra[per_thread], rb = 0.0;
    auto load = [&](int64_t k0) {
#pragma unroll
        for (int u = 0; u < per_thread; ++u) {
            const int64_t row = row0 + ld_row + u * (block / narrow_k);
            ra[u] = row < g.m && k0 + ld_l < k_len ? a[row * g.a_stride + k0 + ld_l] : 0.0;
        }
        rb = tid < narrow_k * NB && k0 + b_l < k_len && b_j < n ? b[(k0 + b_l) * g.b_stride + b_j] : 0.0;
    };
    auto store = [&]() {
#pragma unroll
        for (int u = 0; u < per_thread; ++u) {
            as[(ld_row + u * (block / narrow_k)) * narrow_pitch + ld_l] = Mode != simple ? alpha * ra[u] : ra[u];
        }
        if (tid < narrow_k * NB) bs[tid] = rb;
    };

    const int64_t row = row0 + tid;
    const bool owner = row < g.m;
    // the rows of c this workgroup owns enter and leave through the LDS image, n contiguous values per row and lane after
    // lane (a thread reading or writing its own row would touch one 8-byte piece of 64 different lines per access)
    const int c_elems = static_cast<int>(min(static_cast<int64_t>(narrow_rows), g.m - row0)) * n;
    double acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = 0.0;
    if (Mode == advanced) {
        for (int e = tid; e < c_elems; e += block) {
            const int r = e / n, j = e - r * n;
            as[r * narrow_pitch + j] = c[(row0 + r) * g.c_stride + j];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            if (owner && j < n) acc[j] = as[tid * narrow_pitch + j] * beta;
        }
        __syncthreads();
    }
    if (k_len > 0) load(0);
    for (int64_t k0 = 0; k0 < k_len; k0 += narrow_k) {
        store();
        __syncthreads();
        if (k0 + narrow_k < k_len) load(k0 + narrow_k);
        const int kk = static_cast<int>(min(static_cast<int64_t>(narrow_k), k_len - k0));
        const double* pa = as + tid * narrow_pitch;
        auto step = [&](int l) {
            const double va = pa[l];
#pragma unroll
            for (int j = 0; j < NB; ++j) acc[j] = acc[j] + va * bs[l * NB + j];
        };
        if (kk == narrow_k) {
#pragma unroll
            for (int l = 0; l < narrow_k; ++l) step(l);
        } else {
            for (int l = 0; l < kk; ++l) step(l);
        }
        __syncthreads();
    }
    // (the loop's last barrier is behind every read of `as`)
#pragma unroll
    for (int j = 0; j < NB; ++j) as[tid * narrow_pitch + j] = acc[j];
    __syncthreads();
    for (int e = tid; e < c_elems; e += block) {
        const int r = e / n, j = e - r * n;
        c[(row0 + r) * g.c_stride + j] = as[r * narrow_pitch + j];
    }
}

// c(i,j) = c(i,j) * beta (or +0.0), then + partial z of (i,j) for ascending z
template <bool Advanced>
__global__ __launch_bounds__(block) void gemm_split_sum_kernel(int64_t m, int64_t n, int64_t nchunks,
                                                              const double* __restrict__ partials,
                                                              double* __restrict__ c, int64_t c_stride,
                                                              const double* __restrict__ beta_p)
{
    const int64_t mn = m * n;
    for (int64_t e = blockIdx.x * static_cast<int64_t>(block) + threadIdx.x; e < mn;
         e += static_cast<int64_t>(gridDim.x) * block) {
        const int64_t row = e / n, col = e - row * n;
        double acc = 0.0;
        if (Advanced) acc = c[row * c_stride + col] * beta_p[0];
        for (int64_t z = 0; z < nchunks; ++z) acc = acc + partials[z * mn + e];
        c[row * c_stride + col] = acc;
    }
}

constexpr int tr_tile = 64;

__global__ __launch_bounds__(block) void transpose_kernel(int64_t nrows, int64_t ncols, int64_t tiles_c,
                                                         const double* __restrict__ in, int64_t in_stride,
                                                         double* __restrict__ out, int64_t out_stride)
{
    __shared__ double t[tr_tile][tr_tile + 1];
    const int64_t tr = blockIdx.x / tiles_c, tc = blockIdx.x - tr * tiles_c;
    const int64_t r0 = tr * tr_tile, c0 = tc * tr_tile;
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
#pragma unroll
    for (int u = 0; u < tr_tile * 64 / block; ++u) {
        const int i = y + u * (block / 64);
        if (r0 + i < nrows && c0 + x < ncols) t[i][x] = in[(r0 + i) * in_stride + c0 + x];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < tr_tile * 64 / block; ++u) {
        const int i = y + u * (block / 64);
        if (c0 + i < ncols && r0 + x < nrows) out[(c0 + i) * out_stride + r0 + x] = t[x][i];
    }
}

int64_t ordered_workgroups(int64_t m, int64_t n)
{
    if (n <= narrow_max_n) return ceildiv(m, narrow_rows);
    return ceildiv(m, tile_m) * ceildiv(n, tile_n);
}

// 1 tile, 2 narrow, 3 split
int plan(int64_t m, int64_t n, int64_t k, int mode)
{
    const int ordered = n <= narrow_max_n ? 2 : 1;
    if (mode == 2) return 3;
    if (mode == 1 || k <= split_chunk) return ordered;
    if (m == 0 || n == 0) return ordered;
    return ordered_workgroups(m, n) <= split_max_workgroups && k >= split_min_k ? 3 : ordered;
}

template <int Mode>
void launch_ordered(hipStream_t s, unsigned grid, const gemm_args& g)
{
    if (g.n > narrow_max_n) {
        hipLaunchKernelGGL(gemm_tile_kernel<Mode>, dim3(grid), dim3(block), 0, s, g);
    } else if (g.n > 8) {
        hipLaunchKernelGGL((gemm_narrow_kernel<16, Mode>), dim3(grid), dim3(block), 0, s, g);
    } else if (g.n > 4) {
        hipLaunchKernelGGL((gemm_narrow_kernel<8, Mode>), dim3(grid), dim3(block), 0, s, g);
    } else if (g.n > 2) {
        hipLaunchKernelGGL((gemm_narrow_kernel<4, Mode>), dim3(grid), dim3(block), 0, s, g);
    } else if (g.n > 1) {
        hipLaunchKernelGGL((gemm_narrow_kernel<2, Mode>), dim3(grid), dim3(block), 0, s, g);
    } else {
        hipLaunchKernelGGL((gemm_narrow_kernel<1, Mode>), dim3(grid), dim3(block), 0, s, g);
    }
}

}  // namespace
}  // namespace gkomi

using namespace gkomi;

extern "C" int64_t gkomi_dense_gemm_split_chunk(void) { return split_chunk; }

extern "C" int gkomi_dense_gemm_geometry(int64_t* host_tile_m, int64_t* host_tile_n, int64_t* host_tile_k,
                                         int64_t* host_narrow_max_n, int64_t* host_narrow_rows,
                                         int64_t* host_narrow_k)
{
    if (host_tile_m != nullptr) *host_tile_m = tile_m;
    if (host_tile_n != nullptr) *host_tile_n = tile_n;
    if (host_tile_k != nullptr) *host_tile_k = tile_k;
    if (host_narrow_max_n != nullptr) *host_narrow_max_n = narrow_max_n;
    if (host_narrow_rows != nullptr) *host_narrow_rows = narrow_rows;
    if (host_narrow_k != nullptr) *host_narrow_k = narrow_k;
    return GKOMI_SUCCESS;
}

extern "C" int64_t gkomi_dense_gemm_plan(int64_t m, int64_t n, int64_t k, int mode)
{
    if (m < 0 || n < 0 || k < 0 || mode < 0 || mode > 2) return GKOMI_EINVAL;
    return plan(m, n, k, mode);
}

extern "C" size_t gkomi_dense_gemm_workspace_bytes(int64_t m, int64_t n, int64_t k, int mode)
{
    if (m <= 0 || n <= 0 || k < 0 || mode < 0 || mode > 2) return 0;
    if (plan(m, n, k, mode) != 3) return 0;
    return sizeof(double) * static_cast<size_t>(ceildiv(k, split_chunk)) * static_cast<size_t>(m) * static_cast<size_t>(n);
}

extern "C" int gkomi_dense_gemm_f64(gkomi_stream_t s, int64_t m, int64_t n, int64_t k, const double* a,
                                    int64_t a_stride, const double* b, int64_t b_stride, double* c, int64_t c_stride,
                                    const double* alpha, const double* beta, int mode, void* workspace,
                                    size_t workspace_bytes)
{
    if (m < 0 || n < 0 || k < 0 || mode < 0 || mode > 2) return GKOMI_EINVAL;
    if ((alpha == nullptr) != (beta == nullptr)) return GKOMI_EINVAL;
    if (a_stride < k || b_stride < n || c_stride < n) return GKOMI_EINVAL;
    if (m == 0 || n == 0) return GKOMI_SUCCESS;
    if (c == nullptr || (k > 0 && (a == nullptr || b == nullptr))) return GKOMI_EINVAL;
    if (m > INT64_MAX / n) return GKOMI_ENOTSUPPORTED;
    const bool adv = alpha != nullptr;
    const int kind = plan(m, n, k, mode);
    const int64_t wgs = ordered_workgroups(m, n);
    hipStream_t stream = to_stream(s);
    gemm_args g{m, n, k, k, wgs, a, a_stride, b, b_stride, c, c_stride, 0, alpha, beta};
    if (kind != 3) {
        if (wgs > INT32_MAX) return GKOMI_ENOTSUPPORTED;
        if (adv) {
            launch_ordered<advanced>(stream, static_cast<unsigned>(wgs), g);
        } else {
            launch_ordered<simple>(stream, static_cast<unsigned>(wgs), g);
        }
        return check_launch();
    }
    const int64_t nchunks = ceildiv(k, split_chunk);
    if (nchunks > 0 && (wgs > INT32_MAX / nchunks || m * n > INT64_MAX / 8 / nchunks)) return GKOMI_ENOTSUPPORTED;
    if (workspace_bytes < gkomi_dense_gemm_workspace_bytes(m, n, k, mode) || (nchunks > 0 && workspace == nullptr)) {
        return GKOMI_EWORKSPACE;
    }
    double* partials = static_cast<double*>(workspace);
    if (nchunks > 0) {
        g.chunk_len = split_chunk;
        g.c = partials;
        g.c_stride = n;
        g.c_chunk_stride = m * n;
        if (adv) {
            launch_ordered<partial_scaled>(stream, static_cast<unsigned>(wgs * nchunks), g);
        } else {
            launch_ordered<simple>(stream, static_cast<unsigned>(wgs * nchunks), g);
        }
        GKOMI_TRY(check_launch());
    }
    const dim3 grid(grid_for(m * n, block));
    if (adv) {
        hipLaunchKernelGGL(gemm_split_sum_kernel<true>, grid, dim3(block), 0, stream, m, n, nchunks, partials, c, c_stride, beta);
    } else {
        hipLaunchKernelGGL(gemm_split_sum_kernel<false>, grid, dim3(block), 0, stream, m, n, nchunks, partials, c, c_stride, beta);
    }
    return check_launch();
}

extern "C" int gkomi_dense_transpose_f64(gkomi_stream_t s, int64_t nrows, int64_t ncols, const double* in,
                                         int64_t in_stride, double* out, int64_t out_stride)
{
    if (nrows < 0 || ncols < 0) return GKOMI_EINVAL;
    if (in_stride < ncols || out_stride < nrows) return GKOMI_EINVAL;
    if (nrows == 0 || ncols == 0) return GKOMI_SUCCESS;
    if (in == nullptr || out == nullptr) return GKOMI_EINVAL;
    const int64_t tiles_r = ceildiv(nrows, tr_tile), tiles_c = ceildiv(ncols, tr_tile);
    if (tiles_r > INT32_MAX / tiles_c) return GKOMI_ENOTSUPPORTED;
    hipLaunchKernelGGL(transpose_kernel, dim3(static_cast<unsigned>(tiles_r * tiles_c)), dim3(block), 0, to_stream(s), nrows,
                       ncols, tiles_c, in, in_stride, out, out_stride);
    return check_launch();
}

extern "C" int gkomi_dense_matrix_apply_cb(void* ctx_, gkomi_stream_t s, int64_t nrhs, const double* alpha,
                                           const double* b, int64_t b_stride, const double* beta, double* c,
                                           int64_t c_stride)
{
    const gkomi_dense_ctx* d = static_cast<const gkomi_dense_ctx*>(ctx_);
    if (d == nullptr || d->workspace_bytes < 0) return GKOMI_EINVAL;
    return gkomi_dense_gemm_f64(s, d->nrows, nrhs, d->ncols, d->vals, d->stride, b, b_stride, c, c_stride, alpha, beta,
                                static_cast<int>(d->mode), d->workspace, static_cast<size_t>(d->workspace_bytes));
}
