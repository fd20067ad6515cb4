// hip/factorization/cholesky_kernels.hip.cpp: cholesky::cholesky_symbolic_count / cholesky_symbolic_factorize
// (core/factorization/cholesky_kernels.hpp; common/cuda_hip/factorization/cholesky_kernels.hpp.inc:34-149), the two
// kernels of factorization::symbolic_cholesky (core/factorization/symbolic.cpp:66-93).  The reference sorts the
// postorder columns with the vendor library's csrsort; the library sorts inside its own kernels and links none.
#include "../gkomi_bindings.hpp"

namespace gko {
namespace kernels {
namespace hip {
namespace cholesky {

void cholesky_symbolic_count(std::shared_ptr<const HipExecutor> exec, const matrix::Csr<double, int32>* mtx,
                             const factorization::elimination_forest<int32>& forest, int32* row_nnz, array<int32>& tmp_storage)
{
    const int64_t n = static_cast<int64_t>(mtx->get_size()[0]);
    const int64_t nnz = static_cast<int64_t>(mtx->get_num_stored_elements());
    // the reference keeps postorder_cols and lower_ends here for the factorize call; the library's two entries
    // keep nothing between the calls, so this is scratch
    const size_t bytes = gkomi_cholesky_symbolic_workspace_bytes(n, nnz);
    tmp_storage.resize_and_reset((bytes + sizeof(int32) - 1) / sizeof(int32));
    int64_t factor_nnz = 0;
    // blocks (the sum of row_nnz is checked against the 32-bit prefix sum that follows)
    GKOMI_CALL(gkomi_cholesky_symbolic_count_i32(GKOMI_NULL_STREAM, n, nnz, mtx->get_const_row_ptrs(), mtx->get_const_col_idxs(),
                                                 forest.inv_postorder.get_const_data(), forest.postorder_parents.get_const_data(), row_nnz,
                                                 tmp_storage.get_data(), tmp_storage.get_num_elems() * sizeof(int32), &factor_nnz));
}

void cholesky_symbolic_factorize(std::shared_ptr<const HipExecutor> exec, const matrix::Csr<double, int32>* mtx,
                                 const factorization::elimination_forest<int32>& forest, matrix::Csr<double, int32>* l_factor,
                                 const array<int32>& tmp_storage)
{
    const int64_t n = static_cast<int64_t>(mtx->get_size()[0]);
    const int64_t nnz = static_cast<int64_t>(mtx->get_num_stored_elements());
    // tmp_storage is const here and the library's entry writes its scratch: a workspace of this call's own
    array<char> ws(exec, gkomi_cholesky_symbolic_workspace_bytes(n, nnz));
    // blocks, so ws may leave scope
    GKOMI_CALL(gkomi_cholesky_symbolic_factorize_i32(GKOMI_NULL_STREAM, n, nnz, mtx->get_const_row_ptrs(), mtx->get_const_col_idxs(),
                                                     forest.postorder.get_const_data(), forest.inv_postorder.get_const_data(),
                                                     forest.postorder_parents.get_const_data(), l_factor->get_const_row_ptrs(),
                                                     l_factor->get_col_idxs(), ws.get_data(), ws.get_num_elems()));
}

}  // namespace cholesky
}  // namespace hip
}  // namespace kernels
}  // namespace gko
