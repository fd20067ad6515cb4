// hip/factorization/par_ilut_*.hip.cpp: the five kernels of par_ilut_factorization
// (core/factorization/par_ilut_kernels.hpp:56-96), the ones core/factorization/par_ilut.cpp:257-344 runs.  They give
// the results of the REFERENCE executor (reference/factorization/par_ilut_kernels.cpp), bit for bit: the sweep is the
// reference's sequential one, reproduced by a level schedule, and the approximate filter samples as the reference does.
#include "../gkomi_bindings.hpp"

namespace gko {
namespace kernels {
namespace hip {
namespace par_ilut_factorization {

void threshold_select(std::shared_ptr<const HipExecutor> exec, const matrix::Csr<double, int32>* m, int32 rank, array<double>& tmp,
                      array<double>& tmp2, double& threshold)
{
    // tmp is the workspace of the sort (keys and their sorted copy), tmp2 is not needed
    const int64_t nnz = static_cast<int64_t>(m->get_num_stored_elements());
    const size_t bytes = gkomi_par_ilut_select_workspace_bytes(nnz);
    tmp.resize_and_reset((bytes + sizeof(double) - 1) / sizeof(double));
    GKOMI_CALL(gkomi_par_ilut_threshold_select_f64(GKOMI_NULL_STREAM, nnz, m->get_const_values(), rank, tmp.get_data(),
                                                   tmp.get_num_elems() * sizeof(double), &threshold));
}

void threshold_filter(std::shared_ptr<const HipExecutor> exec, const matrix::Csr<double, int32>* m, double threshold,
                      matrix::Csr<double, int32>* m_out, matrix::Coo<double, int32>* m_out_coo, bool lower)
{
    // count, resize through the builders as reference/factorization/par_ilut_kernels.cpp:124-144 does, fill; `lower`
    // selects a kernel variant there and changes no result
    const int64_t n = static_cast<int64_t>(m->get_size()[0]);
    array<char> ws(exec, gkomi_par_ilut_filter_workspace_bytes(n));
    int64_t new_nnz = 0;
    GKOMI_CALL(gkomi_par_ilut_threshold_filter_f64_i32(GKOMI_NULL_STREAM, n, m->get_const_row_ptrs(), m->get_const_col_idxs(),
                                                       m->get_const_values(), threshold, m_out->get_row_ptrs(), nullptr, nullptr, nullptr,
                                                       &new_nnz, ws.get_data(), ws.get_num_elems()));
    matrix::CsrBuilder<double, int32> builder{m_out};
    builder.get_col_idx_array().resize_and_reset(static_cast<size_type>(new_nnz));
    builder.get_value_array().resize_and_reset(static_cast<size_type>(new_nnz));
    int32* new_row_idxs = nullptr;
    if (m_out_coo != nullptr) {
        matrix::CooBuilder<double, int32> coo_builder{m_out_coo};
        coo_builder.get_row_idx_array().resize_and_reset(static_cast<size_type>(new_nnz));
        coo_builder.get_col_idx_array() = make_array_view(exec, static_cast<size_type>(new_nnz), m_out->get_col_idxs());
        coo_builder.get_value_array() = make_array_view(exec, static_cast<size_type>(new_nnz), m_out->get_values());
        new_row_idxs = m_out_coo->get_row_idxs();
    }
    if (new_nnz == 0) return;
    GKOMI_CALL(gkomi_par_ilut_threshold_filter_f64_i32(GKOMI_NULL_STREAM, n, m->get_const_row_ptrs(), m->get_const_col_idxs(),
                                                       m->get_const_values(), threshold, m_out->get_row_ptrs(), m_out->get_col_idxs(),
                                                       m_out->get_values(), new_row_idxs, &new_nnz, ws.get_data(), ws.get_num_elems()));
}

void threshold_filter_approx(std::shared_ptr<const HipExecutor> exec, const matrix::Csr<double, int32>* m, int32 rank, array<double>& tmp,
                             double& threshold, matrix::Csr<double, int32>* m_out, matrix::Coo<double, int32>* m_out_coo)
{
    // the threshold of the sample (tmp: splitters and histogram), then the same filter
    const size_t bytes = gkomi_par_ilut_approx_workspace_bytes();
    tmp.resize_and_reset((bytes + sizeof(double) - 1) / sizeof(double));
    GKOMI_CALL(gkomi_par_ilut_threshold_approx_f64(GKOMI_NULL_STREAM, static_cast<int64_t>(m->get_num_stored_elements()),
                                                   m->get_const_values(), rank, tmp.get_data(), tmp.get_num_elems() * sizeof(double),
                                                   &threshold));
    threshold_filter(exec, m, threshold, m_out, m_out_coo, true);
}

void compute_l_u_factors(std::shared_ptr<const HipExecutor> exec, const matrix::Csr<double, int32>* a, matrix::Csr<double, int32>* l,
                         const matrix::Coo<double, int32>* l_coo, matrix::Csr<double, int32>* u, const matrix::Coo<double, int32>* u_coo,
                         matrix::Csr<double, int32>* u_csc)
{
    // the COO copies are not needed: the level schedule works on rows.  U is read by rows; u_csc gets its values after
    // the sweep.  The analysis is repeated for every call (the patterns change with every call of par_ilut.cpp).
    const int64_t n = static_cast<int64_t>(a->get_size()[0]);
    const int64_t l_nnz = static_cast<int64_t>(l->get_num_stored_elements()), u_nnz = static_cast<int64_t>(u->get_num_stored_elements());
    array<char> ws(exec, gkomi_par_ilut_sweep_workspace_bytes(n, l_nnz, u_nnz));
    int64_t info[6] = {};
    GKOMI_CALL(gkomi_par_ilut_analyse_i32(GKOMI_NULL_STREAM, n, l_nnz, l->get_const_row_ptrs(), l->get_const_col_idxs(), u_nnz,
                                          u->get_const_row_ptrs(), u->get_const_col_idxs(), ws.get_data(), ws.get_num_elems(), info));
    GKOMI_CALL(gkomi_par_ilut_compute_l_u_factors_f64_i32(
        GKOMI_NULL_STREAM, n, a->get_const_row_ptrs(), a->get_const_col_idxs(), a->get_const_values(), l_nnz, l->get_const_row_ptrs(),
        l->get_const_col_idxs(), l->get_values(), u_nnz, u->get_const_row_ptrs(), u->get_const_col_idxs(), u->get_values(),
        u_csc->get_const_row_ptrs(), u_csc->get_const_col_idxs(), u_csc->get_values(), ws.get_const_data(), ws.get_num_elems()));
    exec->synchronize();  // the workspace leaves scope
}

void add_candidates(std::shared_ptr<const HipExecutor> exec, const matrix::Csr<double, int32>* lu, const matrix::Csr<double, int32>* a,
                    const matrix::Csr<double, int32>* l, const matrix::Csr<double, int32>* u, matrix::Csr<double, int32>* l_new,
                    matrix::Csr<double, int32>* u_new)
{
    const int64_t n = static_cast<int64_t>(a->get_size()[0]);
    array<char> ws(exec, gkomi_par_ilut_add_candidates_workspace_bytes(n));
    int64_t l_nnz = 0, u_nnz = 0;
    auto call = [&](bool fill) {
        GKOMI_CALL(gkomi_par_ilut_add_candidates_f64_i32(
            GKOMI_NULL_STREAM, n, lu->get_const_row_ptrs(), lu->get_const_col_idxs(), lu->get_const_values(), a->get_const_row_ptrs(),
            a->get_const_col_idxs(), a->get_const_values(), l->get_const_row_ptrs(), l->get_const_col_idxs(), l->get_const_values(),
            u->get_const_row_ptrs(), u->get_const_col_idxs(), u->get_const_values(), l_new->get_row_ptrs(),
            fill ? l_new->get_col_idxs() : nullptr, fill ? l_new->get_values() : nullptr, u_new->get_row_ptrs(),
            fill ? u_new->get_col_idxs() : nullptr, fill ? u_new->get_values() : nullptr, &l_nnz, &u_nnz, ws.get_data(), ws.get_num_elems()));
    };
    call(false);
    matrix::CsrBuilder<double, int32> l_builder{l_new};
    matrix::CsrBuilder<double, int32> u_builder{u_new};
    l_builder.get_col_idx_array().resize_and_reset(static_cast<size_type>(l_nnz));
    l_builder.get_value_array().resize_and_reset(static_cast<size_type>(l_nnz));
    u_builder.get_col_idx_array().resize_and_reset(static_cast<size_type>(u_nnz));
    u_builder.get_value_array().resize_and_reset(static_cast<size_type>(u_nnz));
    if (n > 0) call(true);
}

}  // namespace par_ilut_factorization
}  // namespace hip
}  // namespace kernels
}  // namespace gko
