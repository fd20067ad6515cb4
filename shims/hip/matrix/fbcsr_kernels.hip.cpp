// hip/matrix/fbcsr_kernels.hip.cpp: the <double, int32> instantiations of core/matrix/fbcsr_kernels.hpp and
// csr::convert_to_fbcsr (core/matrix/csr_kernels.hpp).  The reference's HIP spmv hands the matrix to a vendor bsrmv
// (:164,222); these go to csrc/fbcsr.hip, bit-identical to reference/matrix/fbcsr_kernels.cpp.
#include "../gkomi_bindings.hpp"

namespace gko {
namespace kernels {
namespace hip {
namespace fbcsr {
namespace {

using Mtx = matrix::Fbcsr<double, int32>;

// count, size the arrays, fill: the two calls of gkomi_csr_convert_to_fbcsr_i32
void blocks_from_csr(std::shared_ptr<const Executor> exec, size_type nrows, size_type ncols, int bs, size_type nnz, const int32* row_ptrs,
                     const int32* col_idxs, const double* vals, array<int32>& out_row_ptrs, array<int32>& out_col_idxs,
                     array<double>& out_values)
{
    array<char> ws(exec, gkomi_csr_convert_to_fbcsr_workspace_bytes(nnz) + 8);
    int64_t nbnz = 0;
    out_row_ptrs.resize_and_reset(bs > 0 ? nrows / bs + 1 : 1);
    GKOMI_CALL(gkomi_csr_convert_to_fbcsr_i32(GKOMI_NULL_STREAM, nrows, ncols, bs, nnz, row_ptrs, col_idxs, vals, out_row_ptrs.get_data(),
                                              nullptr, nullptr, &nbnz, ws.get_data(), ws.get_num_elems()));
    out_col_idxs.resize_and_reset(static_cast<size_type>(nbnz));
    out_values.resize_and_reset(static_cast<size_type>(nbnz) * bs * bs);
    if (nbnz > 0) {
        GKOMI_CALL(gkomi_csr_convert_to_fbcsr_i32(GKOMI_NULL_STREAM, nrows, ncols, bs, nnz, row_ptrs, col_idxs, vals, out_row_ptrs.get_data(),
                                                  out_col_idxs.get_data(), out_values.get_data(), &nbnz, ws.get_data(), ws.get_num_elems()));
    }
}

}  // namespace

void spmv(std::shared_ptr<const HipExecutor> exec, const Mtx* a, const matrix::Dense<double>* b, matrix::Dense<double>* c)
{
    GKOMI_CALL(gkomi_fbcsr_spmv_f64_i32(GKOMI_NULL_STREAM, a->get_num_block_rows(), a->get_num_block_cols(), a->get_block_size(),
                                        a->get_num_stored_blocks(), a->get_const_row_ptrs(), a->get_const_col_idxs(), a->get_const_values(),
                                        b->get_const_values(), b->get_stride(), b->get_size()[1], c->get_values(), c->get_stride(), nullptr,
                                        nullptr));
}

void advanced_spmv(std::shared_ptr<const HipExecutor> exec, const matrix::Dense<double>* alpha, const Mtx* a, const matrix::Dense<double>* b,
                   const matrix::Dense<double>* beta, matrix::Dense<double>* c)
{
    GKOMI_CALL(gkomi_fbcsr_spmv_f64_i32(GKOMI_NULL_STREAM, a->get_num_block_rows(), a->get_num_block_cols(), a->get_block_size(),
                                        a->get_num_stored_blocks(), a->get_const_row_ptrs(), a->get_const_col_idxs(), a->get_const_values(),
                                        b->get_const_values(), b->get_stride(), b->get_size()[1], c->get_values(), c->get_stride(),
                                        alpha->get_const_values(), beta->get_const_values()));
}

// row-major sorted, duplicate-free entries (what Fbcsr::read hands over): row indices -> pointers, then csr::convert_to_fbcsr's loop
void fill_in_matrix_data(std::shared_ptr<const HipExecutor> exec, device_matrix_data<double, int32>& data, int block_size,
                         array<int32>& row_ptrs, array<int32>& col_idxs, array<double>& values)
{
    const auto size = data.get_size();
    array<int32> csr_row_ptrs(exec, size[0] + 1);
    array<char> ws(exec, gkomi_prefix_sum_workspace_bytes(size[0] + 1) + 8);
    GKOMI_CALL(gkomi_convert_idxs_to_ptrs_i32(GKOMI_NULL_STREAM, data.get_const_row_idxs(), data.get_num_elems(), size[0], csr_row_ptrs.get_data(),
                                              ws.get_data(), ws.get_num_elems()));
    blocks_from_csr(exec, size[0], size[1], block_size, data.get_num_elems(), csr_row_ptrs.get_const_data(), data.get_const_col_idxs(),
                    data.get_const_values(), row_ptrs, col_idxs, values);
}

void fill_in_dense(std::shared_ptr<const HipExecutor> exec, const Mtx* source, matrix::Dense<double>* result)
{
    GKOMI_CALL(gkomi_fbcsr_fill_in_dense_f64_i32(GKOMI_NULL_STREAM, source->get_num_block_rows(), source->get_num_block_cols(),
                                                 source->get_block_size(), source->get_num_stored_blocks(), source->get_const_row_ptrs(),
                                                 source->get_const_col_idxs(), source->get_const_values(), result->get_values(),
                                                 result->get_stride()));
}

void convert_to_csr(std::shared_ptr<const HipExecutor> exec, const Mtx* source, matrix::Csr<double, int32>* result)
{
    GKOMI_CALL(gkomi_fbcsr_convert_to_csr_i32(GKOMI_NULL_STREAM, source->get_num_block_rows(), source->get_block_size(),
                                              source->get_num_stored_blocks(), source->get_const_row_ptrs(), source->get_const_col_idxs(),
                                              source->get_const_values(), result->get_row_ptrs(), result->get_col_idxs(), result->get_values()));
}

void transpose(std::shared_ptr<const HipExecutor> exec, const Mtx* orig, Mtx* trans)
{
    array<char> ws(exec, gkomi_fbcsr_transpose_workspace_bytes(orig->get_num_stored_blocks()) + 8);
    GKOMI_CALL(gkomi_fbcsr_transpose_f64_i32(GKOMI_NULL_STREAM, orig->get_num_block_rows(), orig->get_num_block_cols(), orig->get_block_size(),
                                             orig->get_num_stored_blocks(), orig->get_const_row_ptrs(), orig->get_const_col_idxs(),
                                             orig->get_const_values(), trans->get_row_ptrs(), trans->get_col_idxs(), trans->get_values(),
                                             ws.get_data(), ws.get_num_elems()));
}

// real values: conj is the identity
void conj_transpose(std::shared_ptr<const HipExecutor> exec, const Mtx* orig, Mtx* trans) { transpose(exec, orig, trans); }

void is_sorted_by_column_index(std::shared_ptr<const HipExecutor> exec, const Mtx* to_check, bool* is_sorted)
{
    array<char> ws(exec, 8);
    int sorted = 1;
    GKOMI_CALL(gkomi_fbcsr_is_sorted_by_column_index_i32(GKOMI_NULL_STREAM, to_check->get_num_block_rows(), to_check->get_const_row_ptrs(),
                                                         to_check->get_const_col_idxs(), ws.get_data(), ws.get_num_elems(), &sorted));
    *is_sorted = sorted != 0;
}

void sort_by_column_index(std::shared_ptr<const HipExecutor> exec, Mtx* to_sort)
{
    array<char> ws(exec, gkomi_fbcsr_sort_workspace_bytes(to_sort->get_num_stored_blocks(), to_sort->get_block_size()) + 8);
    GKOMI_CALL(gkomi_fbcsr_sort_by_column_index_f64_i32(GKOMI_NULL_STREAM, to_sort->get_num_block_rows(), to_sort->get_block_size(),
                                                        to_sort->get_num_stored_blocks(), to_sort->get_const_row_ptrs(), to_sort->get_col_idxs(),
                                                        to_sort->get_values(), ws.get_data(), ws.get_num_elems()));
}

void extract_diagonal(std::shared_ptr<const HipExecutor> exec, const Mtx* orig, matrix::Diagonal<double>* diag)
{
    GKOMI_CALL(gkomi_fbcsr_extract_diagonal_f64_i32(GKOMI_NULL_STREAM, orig->get_num_block_rows(), orig->get_num_block_cols(),
                                                    orig->get_block_size(), orig->get_const_row_ptrs(), orig->get_const_col_idxs(),
                                                    orig->get_const_values(), diag->get_values()));
}

}  // namespace fbcsr

namespace csr {

void convert_to_fbcsr(std::shared_ptr<const HipExecutor> exec, const matrix::Csr<double, int32>* source, int bs, array<int32>& row_ptrs,
                      array<int32>& col_idxs, array<double>& values)
{
    fbcsr::blocks_from_csr(exec, source->get_size()[0], source->get_size()[1], bs, source->get_num_stored_elements(), source->get_const_row_ptrs(),
                           source->get_const_col_idxs(), source->get_const_values(), row_ptrs, col_idxs, values);
}

}  // namespace csr
}  // namespace hip
}  // namespace kernels
}  // namespace gko
