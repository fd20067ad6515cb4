// The setup of the sparse direct solver: elimination forest, symbolic Cholesky, lu_factorization
// (core/factorization/elimination_forest.cpp:44-207, core/factorization/symbolic.cpp:66-93,
//  core/factorization/lu.cpp:85-145; the reference's HIP kernels are
//  common/cuda_hip/factorization/cholesky_kernels.hpp.inc:34-149 and lu_kernels.hpp.inc:36-154).
//
// Elimination forest: host code, as in the reference (compute_elim_forest clones the matrix to the master
// executor).  Loop for loop elimination_forest.cpp:44-152, so the order of the children and the postorder are
// the reference's.  Only entries col < row are read.
//
// Symbolic Cholesky.  Row `row` of L holds the nodes on the forest paths from every lower column of A's row up to
// (not including) `row`, and the diagonal last.  As in the reference's kernels the lower columns are mapped to
// their postorder indices and sorted; consecutive pairs (node, next_node) are then independent: each climbs
// postorder_parents while node < next_node.  The last pair ends at the row's own postorder index, so a row of A
// need not store its diagonal, and since the sort is ours, rows of A need not be sorted (the reference
// executor's semantics, reference/factorization/cholesky_kernels.cpp:58-128; a repeated column climbs nothing).
//   * one wave (64 lanes) per row for every kernel here: the reference's config::warp_size tile.  Rows of A
//     usually hold 3-30 lower entries, so a group of 8 or 16 lanes may keep more lanes busy; this width is
//     UNMEASURED.
//   * the sort is a rank sort inside the wave (every lane counts the keys in front of its own): m * m / 64 steps
//     for a row of m lower entries, no vendor library.  Fine for the rows of meshes and grids; a row of tens of
//     thousands of lower entries would be slow, not wrong.
//   * a climb stops at a parent that is not larger than its node: a forest that is not one (cycles, indices out
//     of range) ends in GKOMI_EINVAL, never in an endless loop or an access out of range.
//   * factorize checks every position against the row's range before it stores: it writes exactly
//     [out_row_ptrs[row], out_row_ptrs[row + 1]), and reports row_ptrs that do not fit with GKOMI_EINVAL.
// No kernel here waits on another workgroup.
//
// lu_factorization::initialize: zero, scatter A by binary search in the (sorted) factor row, diag_idxs.
// lu_factorization::factorize: see gkomi.h -- compute_lu of ilu.hip on the filled pattern, no second kernel.
#include "common.hpp"

#include <numeric>
#include <vector>

#include "internal.hpp"

namespace gkomi {
namespace {

constexpr int sym_block = 256;
constexpr int sym_rows = sym_block / wave_size;  // rows per workgroup: a wave each
constexpr int max_sym_grid = 1 << 16;

// ---- elimination forest (host) ---------------------------------------------------------------------

struct disjoint_sets {
    std::vector<int32_t> up, size;
    explicit disjoint_sets(int32_t n) : up(static_cast<size_t>(n)), size(static_cast<size_t>(n), 1)
    {
        std::iota(up.begin(), up.end(), 0);
    }
    int32_t find(int32_t x)
    {
        int32_t rep = x;
        while (up[rep] != rep) rep = up[rep];
        while (up[x] != rep) {
            const int32_t next = up[x];
            up[x] = rep;
            x = next;
        }
        return rep;
    }
    // both are representatives; returns the representative of the union
    int32_t join(int32_t a, int32_t b)
    {
        if (a == b) return a;
        if (size[a] < size[b]) std::swap(a, b);
        up[b] = a;
        size[a] += size[b];
        return a;
    }
};

// GKOMI_EINVAL for a lower column < 0 or row_ptrs that decrease
int forest_host(int32_t n, const int32_t* row_ptrs, const int32_t* cols, int32_t* parent, int32_t* child_ptr,
                int32_t* child, int32_t* postorder, int32_t* inv_postorder, int32_t* postorder_parent)
{
    // parents (elimination_forest.cpp:44-78)
    {
        disjoint_sets subtrees(n);
        std::vector<int32_t> subtree_root(static_cast<size_t>(n));
        const int32_t unattached = n;
        for (int32_t row = 0; row < n; ++row) {
            subtree_root[row] = row;
            parent[row] = unattached;
            int32_t row_rep = row;
            if (row_ptrs[row + 1] < row_ptrs[row] || row_ptrs[row] < 0) return GKOMI_EINVAL;
            for (int32_t nz = row_ptrs[row]; nz < row_ptrs[row + 1]; ++nz) {
                const int32_t col = cols[nz];
                if (col < 0) return GKOMI_EINVAL;
                if (col < row) {
                    const int32_t col_rep = subtrees.find(col);
                    const int32_t col_root = subtree_root[col_rep];
                    if (parent[col_root] == unattached && col_root != row) {
                        parent[col_root] = row;
                        row_rep = subtrees.join(row_rep, col_rep);
                        subtree_root[row_rep] = row;
                    }
                }
            }
        }
    }
    // children (:81-102): child_ptr has n + 2 entries, the roots are the children of the pseudo-root n
    std::fill_n(child_ptr, static_cast<size_t>(n) + 2, 0);
    for (int32_t i = 0; i < n; ++i) {
        const int32_t p = parent[i];
        if (p < n) ++child_ptr[p + 2];
    }
    std::partial_sum(child_ptr, child_ptr + n + 2, child_ptr);
    for (int32_t i = 0; i < n; ++i) {
        const int32_t p = parent[i];
        child[child_ptr[p + 1]] = i;
        ++child_ptr[p + 1];
    }
    // postorder (:105-139)
    {
        std::vector<int32_t> current_child(static_cast<size_t>(n) + 1, 0);
        int32_t postorder_idx = 0;
        for (int32_t tree = child_ptr[n]; tree < child_ptr[n + 1]; ++tree) {
            int32_t cur_node = child[tree];
            while (cur_node < n) {
                const int32_t first_child = child_ptr[cur_node];
                const int32_t num_children = child_ptr[cur_node + 1] - first_child;
                if (current_child[cur_node] >= num_children) {
                    postorder[postorder_idx] = cur_node;
                    inv_postorder[cur_node] = postorder_idx;
                    cur_node = parent[cur_node];
                    ++postorder_idx;
                } else {
                    const int32_t old_node = cur_node;
                    cur_node = child[first_child + current_child[old_node]];
                    ++current_child[old_node];
                }
            }
        }
    }
    // postorder parents (:142-152)
    for (int32_t row = 0; row < n; ++row) {
        postorder_parent[inv_postorder[row]] = parent[row] == n ? n : inv_postorder[parent[row]];
    }
    return GKOMI_SUCCESS;
}

// ---- symbolic Cholesky ---------------------------------------------------------------------------------

struct symbolic_header {
    int32_t flags;  // != 0: a column or a forest index out of range, a parent that does not climb, row_ptrs that do not fit
    int32_t pad_;
    unsigned long long total;  // sum of row_nnz in 64 bits
};

struct symbolic_layout {
    size_t mapped, sorted, lower_cnt, total;
};

symbolic_layout make_symbolic_layout(int64_t n, int64_t nnz)
{
    symbolic_layout l{};
    size_t off = 256;
    const size_t entries = align256(sizeof(int32_t) * static_cast<size_t>(nnz > 0 ? nnz : 1));
    l.mapped = off; off += entries;
    l.sorted = off; off += entries;
    l.lower_cnt = off; off += align256(sizeof(int32_t) * static_cast<size_t>(n > 0 ? n : 1));
    l.total = off;
    return l;
}

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1; }

// mapped[row_ptrs[row] + 0 .. lower_cnt[row]) = inv_postorder[col] of the entries col < row of the row, in
// storage order (build_postorder_cols, cholesky_kernels.hpp.inc:34-59, without the diagonal and the sentinels)
__global__ __launch_bounds__(sym_block) void lu_map_lower_kernel(int32_t n, int32_t nnz,
                                                                const int32_t* __restrict__ row_ptrs,
                                                                const int32_t* __restrict__ cols,
                                                                const int32_t* __restrict__ inv_postorder,
                                                                int32_t* __restrict__ mapped,
                                                                int32_t* __restrict__ lower_cnt,
                                                                symbolic_header* __restrict__ header)
{
    const int wave = threadIdx.x / wave_size, lane = threadIdx.x % wave_size;
    for (int64_t row64 = static_cast<int64_t>(blockIdx.x) * sym_rows + wave; row64 < n;
         row64 += static_cast<int64_t>(gridDim.x) * sym_rows) {
        const int row = static_cast<int>(row64);
        const int begin = row_ptrs[row];
        int end = row_ptrs[row + 1];
        int cnt = 0;
        bool bad = false;
        if (begin < 0 || end < begin || end > nnz) {  // the row is not inside the arrays: treated as empty
            bad = true;
            end = begin;
        }
        for (int base = begin; base < end; base += wave_size) {
            const int nz = base + lane;
            const int col = nz < end ? cols[nz] : row;
            bool lower = col < row;
            int p = 0;
            if (lower) {
                if (col < 0) {
                    bad = true;
                    lower = false;
                } else {
                    p = inv_postorder[col];
                    if (p < 0 || p >= n) {
                        bad = true;
                        lower = false;
                    }
                }
            }
            const unsigned long long mask = __ballot(lower);
            if (lower) mapped[begin + cnt + __popcll(mask & lanes_below(lane))] = p;
            cnt += __popcll(mask);
        }
        if (lane == 0) lower_cnt[row] = cnt;
        if (bad) atomicOr(&header->flags, 1);
    }
}

// sorted[...] = mapped[...] of every row in ascending order: the rank of a key is the number of keys in front of it
__global__ __launch_bounds__(sym_block) void lu_sort_lower_kernel(int32_t n, const int32_t* __restrict__ row_ptrs,
                                                                 const int32_t* __restrict__ lower_cnt,
                                                                 const int32_t* __restrict__ mapped,
                                                                 int32_t* __restrict__ sorted)
{
    const int wave = threadIdx.x / wave_size, lane = threadIdx.x % wave_size;
    for (int64_t row64 = static_cast<int64_t>(blockIdx.x) * sym_rows + wave; row64 < n;
         row64 += static_cast<int64_t>(gridDim.x) * sym_rows) {
        const int row = static_cast<int>(row64);
        const int m = lower_cnt[row];
        const int32_t* src = mapped + row_ptrs[row];
        int32_t* dst = sorted + row_ptrs[row];
        for (int i = lane; i < m; i += wave_size) {
            const int key = src[i];
            int rank = 0;
            for (int j = 0; j < m; ++j) {
                const int other = src[j];
                rank += (other < key || (other == key && j < i)) ? 1 : 0;
            }
            dst[rank] = key;  // rank < m: at most m - 1 keys are in front of one
        }
    }
}

// the climb of both kernels: from `node` to its postorder parent, or -1 if that is no step upwards
__device__ __forceinline__ int climb(const int32_t* __restrict__ postorder_parent, int node)
{
    const int p = postorder_parent[node];
    return p > node ? p : -1;
}

// cholesky_symbolic_count_kernel (cholesky_kernels.hpp.inc:75-106)
__global__ __launch_bounds__(sym_block) void lu_symbolic_count_kernel(int32_t n, const int32_t* __restrict__ row_ptrs,
                                                                     const int32_t* __restrict__ lower_cnt,
                                                                     const int32_t* __restrict__ sorted,
                                                                     const int32_t* __restrict__ inv_postorder,
                                                                     const int32_t* __restrict__ postorder_parent,
                                                                     int32_t* __restrict__ row_nnz,
                                                                     symbolic_header* __restrict__ header)
{
    const int wave = threadIdx.x / wave_size, lane = threadIdx.x % wave_size;
    for (int64_t row64 = static_cast<int64_t>(blockIdx.x) * sym_rows + wave; row64 < n;
         row64 += static_cast<int64_t>(gridDim.x) * sym_rows) {
        const int row = static_cast<int>(row64);
        const int m = lower_cnt[row];
        const int32_t* s = sorted + row_ptrs[row];
        int last = inv_postorder[row];
        bool bad = false;
        if (last < 0 || last >= n) {
            bad = true;
            last = -1;  // nothing climbs
        }
        int count = 0;
        for (int i = lane; i < m; i += wave_size) {
            int node = s[i];                              // in [0, n): lu_map_lower_kernel
            const int next = i + 1 < m ? s[i + 1] : last;  // < n
            while (node < next) {
                ++count;
                node = climb(postorder_parent, node);
                if (node < 0) {
                    bad = true;
                    break;
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off, 64);
        if (lane == 0) {
            row_nnz[row] = count + 1;  // the diagonal
            atomicAdd(&header->total, static_cast<unsigned long long>(count) + 1);
        }
        if (bad) atomicOr(&header->flags, 2);
    }
}

// cholesky_symbolic_factorize_kernel (cholesky_kernels.hpp.inc:109-149)
__global__ __launch_bounds__(sym_block) void lu_symbolic_factorize_kernel(
    int32_t n, const int32_t* __restrict__ row_ptrs, const int32_t* __restrict__ lower_cnt,
    const int32_t* __restrict__ sorted, const int32_t* __restrict__ postorder,
    const int32_t* __restrict__ inv_postorder, const int32_t* __restrict__ postorder_parent,
    const int32_t* __restrict__ out_row_ptrs, int32_t* __restrict__ out_cols, symbolic_header* __restrict__ header)
{
    const int wave = threadIdx.x / wave_size, lane = threadIdx.x % wave_size;
    const unsigned long long prefix_mask = lanes_below(lane);
    for (int64_t row64 = static_cast<int64_t>(blockIdx.x) * sym_rows + wave; row64 < n;
         row64 += static_cast<int64_t>(gridDim.x) * sym_rows) {
        const int row = static_cast<int>(row64);
        const int m = lower_cnt[row];
        const int32_t* s = sorted + row_ptrs[row];
        int last = inv_postorder[row];
        bool bad = false;
        if (last < 0 || last >= n) {
            bad = true;
            last = -1;
        }
        int out_base = out_row_ptrs[row];
        const int out_diag = out_row_ptrs[row + 1] - 1;  // the lower entries go in front of it
        for (int base = 0; base < m; base += wave_size) {
            const int i = base + lane;
            int node = i < m ? s[i] : -1;
            const int next = i < m ? (i + 1 < m ? s[i + 1] : last) : -1;
            bool pred = node < next;
            unsigned long long mask = __ballot(pred);
            while (mask) {
                if (pred) {
                    const int out_nz = out_base + __popcll(mask & prefix_mask);
                    if (out_nz < out_diag) {
                        out_cols[out_nz] = postorder[node];
                    } else {
                        bad = true;
                    }
                    node = climb(postorder_parent, node);
                    if (node < 0) bad = true;
                    pred = node >= 0 && node < next;
                }
                out_base += __popcll(mask);
                mask = __ballot(pred);
            }
        }
        if (lane == 0) {
            if (out_base == out_diag) {
                out_cols[out_base] = row;
            } else {
                bad = true;
            }
        }
        if (bad) atomicOr(&header->flags, 4);
    }
}

int run_map_and_sort(hipStream_t stream, int32_t n, int32_t nnz, const int32_t* row_ptrs, const int32_t* col_idxs,
                     const int32_t* inv_postorder, char* ws, const symbolic_layout& l)
{
    GKOMI_TRY(static_cast<int>(hipMemsetAsync(ws, 0, 256, stream)));
    const dim3 grid(grid_for(n, sym_rows, max_sym_grid));
    hipLaunchKernelGGL(lu_map_lower_kernel, grid, dim3(sym_block), 0, stream, n, nnz, row_ptrs, col_idxs, inv_postorder,
                       reinterpret_cast<int32_t*>(ws + l.mapped), reinterpret_cast<int32_t*>(ws + l.lower_cnt),
                       reinterpret_cast<symbolic_header*>(ws));
    hipLaunchKernelGGL(lu_sort_lower_kernel, grid, dim3(sym_block), 0, stream, n, row_ptrs,
                       reinterpret_cast<const int32_t*>(ws + l.lower_cnt), reinterpret_cast<const int32_t*>(ws + l.mapped),
                       reinterpret_cast<int32_t*>(ws + l.sorted));
    return check_launch();
}

int read_header(hipStream_t stream, const void* ws, symbolic_header* h)
{
    GKOMI_TRY(static_cast<int>(hipMemcpyAsync(h, ws, sizeof(*h), hipMemcpyDeviceToHost, stream)));
    return static_cast<int>(hipStreamSynchronize(stream));
}

// ---- lu_factorization::initialize (lu_kernels.hpp.inc:36-78) ---------------------------------------------
// flags |= 1: an entry of A without a place in the factor's row (skipped), |= 2: a factor row without diagonal
__global__ __launch_bounds__(sym_block) void lu_initialize_kernel(
    int32_t n, const int32_t* __restrict__ a_row_ptrs, const int32_t* __restrict__ a_cols,
    const double* __restrict__ a_vals, int32_t factor_nnz, const int32_t* __restrict__ f_row_ptrs, const int32_t* __restrict__ f_cols,
    double* __restrict__ f_vals, int32_t* __restrict__ diag_idxs, int32_t* __restrict__ flags)
{
    const int wave = threadIdx.x / wave_size, lane = threadIdx.x % wave_size;
    for (int64_t row64 = static_cast<int64_t>(blockIdx.x) * sym_rows + wave; row64 < n;
         row64 += static_cast<int64_t>(gridDim.x) * sym_rows) {
        const int row = static_cast<int>(row64);
        const int f_begin = f_row_ptrs[row];
        int f_end = f_row_ptrs[row + 1];
        const int a_end = a_row_ptrs[row + 1];
        int bad = 0;
        if (f_begin < 0 || f_end < f_begin || f_end > factor_nnz) {  // not inside the factor: an empty row
            bad = 2;
            f_end = f_begin;
        }
        for (int nz = a_row_ptrs[row] + lane; nz < a_end; nz += wave_size) {
            const int at = find_col(f_cols, f_begin, f_end, a_cols[nz]);
            if (at >= 0) {
                f_vals[at] = a_vals[nz];
            } else {
                bad = 1;
            }
        }
        if (lane == 0) {
            const int d = find_col(f_cols, f_begin, f_end, row);
            diag_idxs[row] = d;
            if (d < 0) bad |= 2;
        }
        if (bad) atomicOr(flags, bad);
    }
}

bool too_large(int64_t n) { return n > INT32_MAX - 1024; }

}  // namespace
}  // namespace gkomi

using namespace gkomi;

extern "C" int gkomi_elimination_forest_host_i32(int64_t n, const int32_t* host_row_ptrs,
                                                 const int32_t* host_col_idxs, int32_t* parents,
                                                 int32_t* child_ptrs, int32_t* children, int32_t* postorder,
                                                 int32_t* inv_postorder, int32_t* postorder_parents)
{
    if (n < 0 || host_row_ptrs == nullptr || child_ptrs == nullptr) return GKOMI_EINVAL;
    if (too_large(n)) return GKOMI_ENOTSUPPORTED;
    if (n > 0 && (parents == nullptr || children == nullptr || postorder == nullptr || inv_postorder == nullptr ||
                  postorder_parents == nullptr)) {
        return GKOMI_EINVAL;
    }
    if (n > 0 && host_row_ptrs[n] > host_row_ptrs[0] && host_col_idxs == nullptr) return GKOMI_EINVAL;
    return forest_host(static_cast<int32_t>(n), host_row_ptrs, host_col_idxs, parents, child_ptrs, children, postorder,
                       inv_postorder, postorder_parents);
}

extern "C" int gkomi_elimination_forest_i32(gkomi_stream_t s, int64_t n, const int32_t* row_ptrs,
                                            const int32_t* col_idxs, int32_t* parents, int32_t* child_ptrs,
                                            int32_t* children, int32_t* postorder, int32_t* inv_postorder,
                                            int32_t* postorder_parents)
{
    if (n < 0 || row_ptrs == nullptr || child_ptrs == nullptr) return GKOMI_EINVAL;
    if (too_large(n)) return GKOMI_ENOTSUPPORTED;
    if (n > 0 && (parents == nullptr || children == nullptr || postorder == nullptr || inv_postorder == nullptr ||
                  postorder_parents == nullptr)) {
        return GKOMI_EINVAL;
    }
    hipStream_t stream = to_stream(s);
    const size_t m = static_cast<size_t>(n);
    std::vector<int32_t> rp(m + 1);
    GKOMI_TRY(static_cast<int>(hipMemcpyAsync(rp.data(), row_ptrs, sizeof(int32_t) * (m + 1), hipMemcpyDeviceToHost, stream)));
    GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
    for (size_t i = 0; i < m; ++i) {
        if (rp[i] < 0 || rp[i + 1] < rp[i]) return GKOMI_EINVAL;
    }
    // the entries [rp[0], rp[n]) at their own positions
    const size_t first = static_cast<size_t>(rp[0] > 0 ? rp[0] : 0), end = static_cast<size_t>(rp[m] > 0 ? rp[m] : 0);
    if (end > first && col_idxs == nullptr) return GKOMI_EINVAL;
    std::vector<int32_t> ci(end);
    if (end > first) {
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(ci.data() + first, col_idxs + first, sizeof(int32_t) * (end - first),
                                                  hipMemcpyDeviceToHost, stream)));
        GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
    }
    std::vector<int32_t> out(6 * m + 2);
    int32_t* h_parents = out.data();
    int32_t* h_children = h_parents + m;
    int32_t* h_postorder = h_children + m;
    int32_t* h_inv = h_postorder + m;
    int32_t* h_pp = h_inv + m;
    int32_t* h_child_ptrs = h_pp + m;
    GKOMI_TRY(forest_host(static_cast<int32_t>(n), rp.data(), ci.data(), h_parents, h_child_ptrs, h_children, h_postorder,
                          h_inv, h_pp));
    const struct {
        int32_t* dst;
        const int32_t* src;
        size_t count;
    } copies[] = {{parents, h_parents, m},     {children, h_children, m}, {postorder, h_postorder, m},
                  {inv_postorder, h_inv, m},   {postorder_parents, h_pp, m}, {child_ptrs, h_child_ptrs, m + 2}};
    for (const auto& c : copies) {
        if (c.count == 0) continue;
        GKOMI_TRY(static_cast<int>(hipMemcpyAsync(c.dst, c.src, sizeof(int32_t) * c.count, hipMemcpyHostToDevice, stream)));
    }
    return static_cast<int>(hipStreamSynchronize(stream));  // `out` leaves scope
}

extern "C" size_t gkomi_cholesky_symbolic_workspace_bytes(int64_t n, int64_t nnz)
{
    if (n < 0 || nnz < 0 || too_large(n) || nnz > INT32_MAX) return 0;
    return make_symbolic_layout(n, nnz).total;
}

extern "C" int gkomi_cholesky_symbolic_count_i32(gkomi_stream_t s, int64_t n, int64_t nnz, const int32_t* row_ptrs,
                                                 const int32_t* col_idxs, const int32_t* inv_postorder,
                                                 const int32_t* postorder_parents, int32_t* row_nnz, void* workspace,
                                                 size_t workspace_bytes, int64_t* host_factor_nnz)
{
    if (n < 0 || nnz < 0 || host_factor_nnz == nullptr) return GKOMI_EINVAL;
    *host_factor_nnz = 0;
    if (too_large(n) || nnz > INT32_MAX) return GKOMI_ENOTSUPPORTED;
    if (n == 0) return GKOMI_SUCCESS;
    if (row_ptrs == nullptr || (nnz > 0 && col_idxs == nullptr) || inv_postorder == nullptr ||
        postorder_parents == nullptr || row_nnz == nullptr) {
        return GKOMI_EINVAL;
    }
    const symbolic_layout l = make_symbolic_layout(n, nnz);
    if (workspace == nullptr || workspace_bytes < l.total) return GKOMI_EWORKSPACE;
    hipStream_t stream = to_stream(s);
    char* ws = static_cast<char*>(workspace);
    const int32_t n32 = static_cast<int32_t>(n);
    GKOMI_TRY(run_map_and_sort(stream, n32, static_cast<int32_t>(nnz), row_ptrs, col_idxs, inv_postorder, ws, l));
    hipLaunchKernelGGL(lu_symbolic_count_kernel, dim3(grid_for(n, sym_rows, max_sym_grid)), dim3(sym_block), 0, stream,
                       n32, row_ptrs, reinterpret_cast<const int32_t*>(ws + l.lower_cnt),
                       reinterpret_cast<const int32_t*>(ws + l.sorted), inv_postorder, postorder_parents, row_nnz,
                       reinterpret_cast<symbolic_header*>(ws));
    GKOMI_TRY(check_launch());
    symbolic_header h{};
    GKOMI_TRY(read_header(stream, ws, &h));
    if (h.flags != 0) return GKOMI_EINVAL;
    *host_factor_nnz = static_cast<int64_t>(h.total);
    // the caller's prefix sum is 32 bits wide
    if (h.total > static_cast<unsigned long long>(INT32_MAX)) return GKOMI_ENOTSUPPORTED;
    return GKOMI_SUCCESS;
}

extern "C" int gkomi_cholesky_symbolic_factorize_i32(gkomi_stream_t s, int64_t n, int64_t nnz, const int32_t* row_ptrs,
                                                     const int32_t* col_idxs, const int32_t* postorder,
                                                     const int32_t* inv_postorder, const int32_t* postorder_parents,
                                                     const int32_t* out_row_ptrs, int32_t* out_cols, void* workspace,
                                                     size_t workspace_bytes)
{
    if (n < 0 || nnz < 0) return GKOMI_EINVAL;
    if (too_large(n) || nnz > INT32_MAX) return GKOMI_ENOTSUPPORTED;
    if (n == 0) return GKOMI_SUCCESS;
    if (row_ptrs == nullptr || (nnz > 0 && col_idxs == nullptr) || postorder == nullptr || inv_postorder == nullptr ||
        postorder_parents == nullptr || out_row_ptrs == nullptr || out_cols == nullptr) {
        return GKOMI_EINVAL;
    }
    const symbolic_layout l = make_symbolic_layout(n, nnz);
    if (workspace == nullptr || workspace_bytes < l.total) return GKOMI_EWORKSPACE;
    hipStream_t stream = to_stream(s);
    char* ws = static_cast<char*>(workspace);
    const int32_t n32 = static_cast<int32_t>(n);
    GKOMI_TRY(run_map_and_sort(stream, n32, static_cast<int32_t>(nnz), row_ptrs, col_idxs, inv_postorder, ws, l));
    hipLaunchKernelGGL(lu_symbolic_factorize_kernel, dim3(grid_for(n, sym_rows, max_sym_grid)), dim3(sym_block), 0, stream,
                       n32, row_ptrs, reinterpret_cast<const int32_t*>(ws + l.lower_cnt),
                       reinterpret_cast<const int32_t*>(ws + l.sorted), postorder, inv_postorder, postorder_parents,
                       out_row_ptrs, out_cols, reinterpret_cast<symbolic_header*>(ws));
    GKOMI_TRY(check_launch());
    symbolic_header h{};
    GKOMI_TRY(read_header(stream, ws, &h));
    return h.flags != 0 ? GKOMI_EINVAL : GKOMI_SUCCESS;
}

extern "C" int gkomi_lu_initialize_f64_i32(gkomi_stream_t s, int64_t n, const int32_t* a_row_ptrs,
                                           const int32_t* a_col_idxs, const double* a_vals, int64_t factor_nnz,
                                           const int32_t* f_row_ptrs, const int32_t* f_col_idxs, double* f_vals,
                                           int32_t* diag_idxs, void* workspace, size_t workspace_bytes)
{
    if (n < 0 || factor_nnz < 0) return GKOMI_EINVAL;
    if (too_large(n) || factor_nnz > INT32_MAX) return GKOMI_ENOTSUPPORTED;
    if (n == 0) return GKOMI_SUCCESS;
    if (a_row_ptrs == nullptr || f_row_ptrs == nullptr || diag_idxs == nullptr ||
        (factor_nnz > 0 && (f_col_idxs == nullptr || f_vals == nullptr))) {
        return GKOMI_EINVAL;
    }
    if (workspace == nullptr || workspace_bytes < sizeof(int32_t)) return GKOMI_EWORKSPACE;
    hipStream_t stream = to_stream(s);
    int32_t* flags = static_cast<int32_t*>(workspace);
    GKOMI_TRY(static_cast<int>(hipMemsetAsync(flags, 0, sizeof(int32_t), stream)));
    if (factor_nnz > 0) {
        GKOMI_TRY(static_cast<int>(hipMemsetAsync(f_vals, 0, sizeof(double) * static_cast<size_t>(factor_nnz), stream)));
    }
    hipLaunchKernelGGL(lu_initialize_kernel, dim3(grid_for(n, sym_rows, max_sym_grid)), dim3(sym_block), 0, stream,
                       static_cast<int32_t>(n), a_row_ptrs, a_col_idxs, a_vals, static_cast<int32_t>(factor_nnz), f_row_ptrs, f_col_idxs, f_vals, diag_idxs,
                       flags);
    GKOMI_TRY(check_launch());
    int32_t h = 0;
    GKOMI_TRY(static_cast<int>(hipMemcpyAsync(&h, flags, sizeof(h), hipMemcpyDeviceToHost, stream)));
    GKOMI_TRY(static_cast<int>(hipStreamSynchronize(stream)));
    return h != 0 ? GKOMI_EINVAL : GKOMI_SUCCESS;
}

extern "C" int gkomi_lu_factorize_f64_i32(gkomi_stream_t s, int64_t n, const int32_t* f_row_ptrs,
                                          const int32_t* f_col_idxs, double* f_vals, const void* analysis_workspace,
                                          size_t workspace_bytes)
{
    return ilu_compute_lu(to_stream(s), n, f_row_ptrs, f_col_idxs, f_vals, analysis_workspace, workspace_bytes);
}

// Lu::generate without a symbolic factorization and without symmetric_sparsity (core/factorization/lu.cpp:94-99)
extern "C" int gkomi_lu_symbolic_supported(int has_symbolic, int symmetric_sparsity)
{
    return has_symbolic != 0 || symmetric_sparsity != 0 ? GKOMI_SUCCESS : GKOMI_ENOTSUPPORTED;
}
