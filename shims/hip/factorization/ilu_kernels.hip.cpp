// hip/factorization/ilu_kernels.hip.cpp: ilu_factorization::compute_lu (core/factorization/ilu_kernels.hpp;
// reference/factorization/ilu_kernels.cpp:56-97), where the reference's HIP backend calls the vendor library's
// csrilu0.  In place on the values of a sorted matrix with explicit diagonal (core/factorization/ilu.cpp:80-89).
#include "../gkomi_bindings.hpp"

namespace gko {
namespace kernels {
namespace hip {
namespace ilu_factorization {

void compute_lu(std::shared_ptr<const HipExecutor> exec, matrix::Csr<double, int32>* m)
{
    // analysis (levels of the rows, blocking) and numeric phase in one call, like csrilu0 behind the reference's
    // binding; a caller that factorizes one pattern many times keeps the workspace (gkomi.h)
    const int64_t n = static_cast<int64_t>(m->get_size()[0]);
    array<char> tmp(exec, gkomi_ilu_analysis_workspace_bytes(n));
    int64_t info[6] = {};
    GKOMI_CALL(gkomi_ilu_analyse_i32(GKOMI_NULL_STREAM, n, m->get_const_row_ptrs(), m->get_const_col_idxs(), tmp.get_data(),
                                     tmp.get_num_elems(), info));
    GKOMI_CALL(gkomi_ilu_compute_lu_f64_i32(GKOMI_NULL_STREAM, n, m->get_const_row_ptrs(), m->get_const_col_idxs(), m->get_values(),
                                            tmp.get_const_data(), tmp.get_num_elems()));
    exec->synchronize();  // tmp leaves scope
}

}  // namespace ilu_factorization
}  // namespace hip
}  // namespace kernels
}  // namespace gko
