// hip/factorization/par_ict_*.hip.cpp: the two kernels of par_ict_factorization
// (core/factorization/par_ict_kernels.hpp), the ones core/factorization/par_ict.cpp:228-292 runs beside those of
// par_ilut_factorization.  They give the results of the REFERENCE executor (reference/factorization/par_ict_kernels.cpp),
// bit for bit: the sweep is the reference's sequential one, reproduced by a level schedule.  <double, int32>; the other
// instantiations stay the reference's stubs.
#include "../gkomi_bindings.hpp"

namespace gko {
namespace kernels {
namespace hip {
namespace par_ict_factorization {

void add_candidates(std::shared_ptr<const HipExecutor> exec, const matrix::Csr<double, int32>* llh, const matrix::Csr<double, int32>* a,
                    const matrix::Csr<double, int32>* l, matrix::Csr<double, int32>* l_new)
{
    const int64_t n = static_cast<int64_t>(a->get_size()[0]);
    array<char> ws(exec, gkomi_par_ict_add_candidates_workspace_bytes(n));
    int64_t l_nnz = 0;
    auto call = [&](bool fill) {
        GKOMI_CALL(gkomi_par_ict_add_candidates_f64_i32(
            GKOMI_NULL_STREAM, n, llh->get_const_row_ptrs(), llh->get_const_col_idxs(), llh->get_const_values(), a->get_const_row_ptrs(),
            a->get_const_col_idxs(), a->get_const_values(), l->get_const_row_ptrs(), l->get_const_col_idxs(), l->get_const_values(),
            l_new->get_row_ptrs(), fill ? l_new->get_col_idxs() : nullptr, fill ? l_new->get_values() : nullptr, &l_nnz, ws.get_data(),
            ws.get_num_elems()));
    };
    call(false);
    matrix::CsrBuilder<double, int32> l_builder{l_new};
    l_builder.get_col_idx_array().resize_and_reset(static_cast<size_type>(l_nnz));
    l_builder.get_value_array().resize_and_reset(static_cast<size_type>(l_nnz));
    if (n > 0) call(true);
}

void compute_factor(std::shared_ptr<const HipExecutor> exec, const matrix::Csr<double, int32>* a, matrix::Csr<double, int32>* l,
                    const matrix::Coo<double, int32>* l_coo)
{
    // the COO copy is not needed: the level schedule works on rows.  The analysis is repeated for every call (the
    // pattern changes with every call of par_ict.cpp).
    const int64_t n = static_cast<int64_t>(a->get_size()[0]);
    const int64_t l_nnz = static_cast<int64_t>(l->get_num_stored_elements());
    array<char> ws(exec, gkomi_par_ict_sweep_workspace_bytes(n, l_nnz));
    int64_t info[6] = {};
    GKOMI_CALL(gkomi_par_ict_analyse_i32(GKOMI_NULL_STREAM, n, l_nnz, l->get_const_row_ptrs(), l->get_const_col_idxs(), ws.get_data(),
                                         ws.get_num_elems(), info));
    GKOMI_CALL(gkomi_par_ict_compute_factor_f64_i32(GKOMI_NULL_STREAM, n, a->get_const_row_ptrs(), a->get_const_col_idxs(),
                                                    a->get_const_values(), l_nnz, l->get_const_row_ptrs(), l->get_const_col_idxs(),
                                                    l->get_values(), ws.get_const_data(), ws.get_num_elems()));
    exec->synchronize();  // the workspace leaves scope
}

}  // namespace par_ict_factorization
}  // namespace hip
}  // namespace kernels
}  // namespace gko
