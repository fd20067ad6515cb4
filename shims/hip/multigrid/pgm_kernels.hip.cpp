// hip/multigrid/pgm_kernels.hip.cpp: the eleven kernels of core/multigrid/pgm_kernels.hpp for <double, int32>.  Arrays and
// matrices go through as their device pointers; the counts the reference hands back through host pointers (num_unagg,
// num_agg, coarse_nnz) are read back by the entry points, which block for that -- the reference's HIP kernels copy them
// back the same way.  Scratch is allocated here, per call.
#include "../gkomi_bindings.hpp"

namespace gko {
namespace kernels {
namespace hip {
namespace pgm {
namespace {
using Csr = matrix::Csr<double, int32>;
using Diag = matrix::Diagonal<double>;
}  // namespace

void match_edge(std::shared_ptr<const HipExecutor> exec, const array<int32>& strongest_neighbor, array<int32>& agg)
{
    GKOMI_CALL(gkomi_pgm_match_edge_i32(GKOMI_NULL_STREAM, agg.get_num_elems(), strongest_neighbor.get_const_data(), agg.get_data()));
}

void count_unagg(std::shared_ptr<const HipExecutor> exec, const array<int32>& agg, int32* num_unagg)
{
    array<char> ws(exec, 8);
    int64_t count = 0;
    GKOMI_CALL(gkomi_pgm_count_unagg_i32(GKOMI_NULL_STREAM, agg.get_num_elems(), agg.get_const_data(), &count, ws.get_data(), ws.get_num_elems()));
    *num_unagg = static_cast<int32>(count);
}

void renumber(std::shared_ptr<const HipExecutor> exec, array<int32>& agg, int32* num_agg)
{
    array<char> ws(exec, gkomi_pgm_renumber_workspace_bytes(agg.get_num_elems()) + 8);
    int64_t count = 0;
    GKOMI_CALL(gkomi_pgm_renumber_i32(GKOMI_NULL_STREAM, agg.get_num_elems(), agg.get_data(), &count, ws.get_data(), ws.get_num_elems()));
    *num_agg = static_cast<int32>(count);
}

void sort_agg(std::shared_ptr<const HipExecutor> exec, int32 num, int32* row_idxs, int32* col_idxs)
{
    array<char> ws(exec, gkomi_pgm_sort_workspace_bytes(num) + 8);
    GKOMI_CALL(gkomi_pgm_sort_agg_i32(GKOMI_NULL_STREAM, num, row_idxs, col_idxs, ws.get_data(), ws.get_num_elems()));
    GKOMI_CALL(gkomi_synchronize(GKOMI_NULL_STREAM));  // the scratch goes away with this scope
}

void map_row(std::shared_ptr<const HipExecutor> exec, size_type num_fine_row, const int32* fine_row_ptrs, const int32* agg, int32* row_idxs)
{
    GKOMI_CALL(gkomi_pgm_map_row_i32(GKOMI_NULL_STREAM, num_fine_row, fine_row_ptrs, agg, row_idxs));
}

void map_col(std::shared_ptr<const HipExecutor> exec, size_type nnz, const int32* fine_col_idxs, const int32* agg, int32* col_idxs)
{
    GKOMI_CALL(gkomi_pgm_map_col_i32(GKOMI_NULL_STREAM, nnz, fine_col_idxs, agg, col_idxs));
}

void count_unrepeated_nnz(std::shared_ptr<const HipExecutor> exec, size_type nnz, const int32* row_idxs, const int32* col_idxs,
                          size_type* coarse_nnz)
{
    array<char> ws(exec, gkomi_pgm_coarse_coo_workspace_bytes(nnz) + 8);
    int64_t count = 0;
    GKOMI_CALL(gkomi_pgm_count_unrepeated_nnz_i32(GKOMI_NULL_STREAM, nnz, row_idxs, col_idxs, &count, ws.get_data(), ws.get_num_elems()));
    *coarse_nnz = static_cast<size_type>(count);
}

void find_strongest_neighbor(std::shared_ptr<const HipExecutor> exec, const Csr* weight_mtx, const Diag* diag, array<int32>& agg,
                             array<int32>& strongest_neighbor)
{
    // the entry point adds the number of absorbed rows to a counter, which this interface has no use for
    array<int32> counter(exec, 2);
    const int32 zero[2] = {0, 0};
    exec->copy_from(exec->get_master().get(), 2, zero, counter.get_data());
    GKOMI_CALL(gkomi_pgm_find_strongest_neighbor_f64_i32(GKOMI_NULL_STREAM, agg.get_num_elems(), weight_mtx->get_num_stored_elements(),
                                                         weight_mtx->get_const_row_ptrs(), weight_mtx->get_const_col_idxs(),
                                                         weight_mtx->get_const_values(), diag->get_const_values(), agg.get_data(),
                                                         strongest_neighbor.get_data(), counter.get_data(), 8));
    GKOMI_CALL(gkomi_synchronize(GKOMI_NULL_STREAM));
}

void assign_to_exist_agg(std::shared_ptr<const HipExecutor> exec, const Csr* weight_mtx, const Diag* diag, array<int32>& agg,
                         array<int32>& intermediate_agg)
{
    array<char> ws(exec, gkomi_pgm_assign_workspace_bytes(agg.get_num_elems()) + 8);
    GKOMI_CALL(gkomi_pgm_assign_to_exist_agg_f64_i32(GKOMI_NULL_STREAM, agg.get_num_elems(), weight_mtx->get_num_stored_elements(),
                                                     weight_mtx->get_const_row_ptrs(), weight_mtx->get_const_col_idxs(),
                                                     weight_mtx->get_const_values(), diag->get_const_values(), agg.get_data(),
                                                     intermediate_agg.get_num_elems() > 0 ? intermediate_agg.get_data() : nullptr,
                                                     ws.get_data(), ws.get_num_elems()));
    GKOMI_CALL(gkomi_synchronize(GKOMI_NULL_STREAM));
}

void sort_row_major(std::shared_ptr<const HipExecutor> exec, size_type nnz, int32* row_idxs, int32* col_idxs, double* vals)
{
    array<char> ws(exec, gkomi_pgm_sort_workspace_bytes(nnz) + 8);
    GKOMI_CALL(gkomi_pgm_sort_row_major_f64_i32(GKOMI_NULL_STREAM, nnz, row_idxs, col_idxs, vals, ws.get_data(), ws.get_num_elems()));
    GKOMI_CALL(gkomi_synchronize(GKOMI_NULL_STREAM));
}

void compute_coarse_coo(std::shared_ptr<const HipExecutor> exec, size_type fine_nnz, const int32* row_idxs, const int32* col_idxs,
                        const double* vals, matrix::Coo<double, int32>* coarse_coo)
{
    array<char> ws(exec, gkomi_pgm_coarse_coo_workspace_bytes(fine_nnz) + 8);
    GKOMI_CALL(gkomi_pgm_compute_coarse_coo_f64_i32(GKOMI_NULL_STREAM, fine_nnz, row_idxs, col_idxs, vals, coarse_coo->get_num_stored_elements(),
                                                    coarse_coo->get_row_idxs(), coarse_coo->get_col_idxs(), coarse_coo->get_values(),
                                                    ws.get_data(), ws.get_num_elems()));
    GKOMI_CALL(gkomi_synchronize(GKOMI_NULL_STREAM));
}

}  // namespace pgm
}  // namespace hip
}  // namespace kernels
}  // namespace gko
