// Diagnostic build (not shipped): the product's nonzero-split SpMV kernel as the cold apply of the 1M-row matrix
// runs it (int32, 256 threads, 1536-nonzero tile, nontemporal streams, one contiguous eighth of the tiles per XCD),
// compiled once per value of GKOMI_GATHER_PROBE: 0 the product, 1 the gather of b at lane-linear stand-in
// addresses, to price what the layout of the gather costs on the same box (tools/gather_probe.py).
#include "../repo-8852-ginkgo_amd/csrc/csr_spmv.hip"

extern "C" int probe_launch(void* stream, int nrows, int nnz, const int32_t* row_ptrs, const int32_t* col_idxs,
                            const double* vals, const double* b, double* c, const int32_t* srow, int over)
{
    using namespace gkomi;
    constexpr int Block = 256, Tile = 1536;
    const int ntiles = nnz / Tile + 1;
    const int per = static_cast<int>(ceildiv(ntiles, num_xcd));
    dim3 grid(static_cast<unsigned>(ceildiv(ntiles, num_xcd * per) * num_xcd * per), 1);
    hipLaunchKernelGGL((csr_split_kernel<int32_t, Block, Tile, split_max_over, false, true, false, true, true>), grid,
                       dim3(Block), 0, static_cast<hipStream_t>(stream), nrows, nnz, row_ptrs, col_idxs, vals, b,
                       int64_t{1}, c, int64_t{1}, nullptr, nullptr, srow, ntiles, per, over);
    return static_cast<int>(hipGetLastError());
}
