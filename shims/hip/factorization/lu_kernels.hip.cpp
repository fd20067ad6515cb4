// hip/factorization/lu_kernels.hip.cpp: lu_factorization::initialize / factorize (core/factorization/lu_kernels.hpp;
// common/cuda_hip/factorization/lu_kernels.hpp.inc:36-154), the numeric phase of experimental::factorization::Lu
// (core/factorization/lu.cpp:131-143).  The library finds columns by binary search in the sorted factor rows, so the
// lookup_* arguments (csr::build_lookup_offsets / build_lookup, which stay unbound) are accepted and unused.  The
// reference's factorize spin-waits on flags of other workgroups; the library's is level-scheduled
// (gkomi_ilu_analyse_i32 + the numeric phase of the exact ILU(0), which on a pattern closed under fill is LU) and waits
// on no other workgroup.
#include "../gkomi_bindings.hpp"

namespace gko {
namespace kernels {
namespace hip {
namespace lu_factorization {

void initialize(std::shared_ptr<const HipExecutor> exec, const matrix::Csr<double, int32>* mtx, const int32* factor_lookup_offsets,
                const int64* factor_lookup_descs, const int32* factor_lookup_storage, int32* diag_idxs,
                matrix::Csr<double, int32>* factors)
{
    const int64_t n = static_cast<int64_t>(mtx->get_size()[0]);
    array<char> flag(exec, 8);
    // blocks on the flag: an entry of A without a place in the factor is an error here (lookup_unsafe in the reference)
    GKOMI_CALL(gkomi_lu_initialize_f64_i32(GKOMI_NULL_STREAM, n, mtx->get_const_row_ptrs(), mtx->get_const_col_idxs(),
                                           mtx->get_const_values(), static_cast<int64_t>(factors->get_num_stored_elements()),
                                           factors->get_const_row_ptrs(), factors->get_const_col_idxs(), factors->get_values(), diag_idxs,
                                           flag.get_data(), flag.get_num_elems()));
}

void factorize(std::shared_ptr<const HipExecutor> exec, const int32* lookup_offsets, const int64* lookup_descs,
               const int32* lookup_storage, const int32* diag_idxs, matrix::Csr<double, int32>* factors, array<int>& tmp_storage)
{
    const int64_t n = static_cast<int64_t>(factors->get_size()[0]);
    // the reference keeps n ready flags in tmp_storage; here it holds the level analysis of the factor's pattern
    const size_t bytes = gkomi_ilu_analysis_workspace_bytes(n);
    tmp_storage.resize_and_reset((bytes + sizeof(int) - 1) / sizeof(int));
    int64_t info[6] = {};
    GKOMI_CALL(gkomi_ilu_analyse_i32(GKOMI_NULL_STREAM, n, factors->get_const_row_ptrs(), factors->get_const_col_idxs(),
                                     tmp_storage.get_data(), tmp_storage.get_num_elems() * sizeof(int), info));
    GKOMI_CALL(gkomi_lu_factorize_f64_i32(GKOMI_NULL_STREAM, n, factors->get_const_row_ptrs(), factors->get_const_col_idxs(),
                                          factors->get_values(), tmp_storage.get_const_data(), tmp_storage.get_num_elems() * sizeof(int)));
}

}  // namespace lu_factorization
}  // namespace hip
}  // namespace kernels
}  // namespace gko
