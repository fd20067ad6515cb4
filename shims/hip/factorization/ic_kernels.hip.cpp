// hip/factorization/ic_kernels.hip.cpp: ic_factorization::compute (core/factorization/ic_kernels.hpp;
// reference/factorization/ic_kernels.cpp:53-100), where the reference's HIP backend calls the vendor library's
// csric0.  In place on the lower triangle of a sorted matrix with explicit diagonal (core/factorization/ic.cpp:81-90).
#include "../gkomi_bindings.hpp"

namespace gko {
namespace kernels {
namespace hip {
namespace ic_factorization {

void compute(std::shared_ptr<const HipExecutor> exec, matrix::Csr<double, int32>* m)
{
    const int64_t n = static_cast<int64_t>(m->get_size()[0]);
    array<char> tmp(exec, gkomi_ilu_analysis_workspace_bytes(n));
    int64_t info[6] = {};
    GKOMI_CALL(gkomi_ilu_analyse_i32(GKOMI_NULL_STREAM, n, m->get_const_row_ptrs(), m->get_const_col_idxs(), tmp.get_data(),
                                     tmp.get_num_elems(), info));
    GKOMI_CALL(gkomi_ic_compute_f64_i32(GKOMI_NULL_STREAM, n, m->get_const_row_ptrs(), m->get_const_col_idxs(), m->get_values(),
                                        tmp.get_const_data(), tmp.get_num_elems()));
    exec->synchronize();  // tmp leaves scope
}

}  // namespace ic_factorization
}  // namespace hip
}  // namespace kernels
}  // namespace gko
