// hip/preconditioner/isai_kernels.hip.cpp: the five kernels of isai (core/preconditioner/isai_kernels.hpp), the ones
// core/preconditioner/isai.cpp:121-265 runs.  They give the results of the REFERENCE executor
// (reference/preconditioner/isai_kernels.cpp), bit for bit: the dense systems of the short rows are solved by the
// reference's substitution and elimination, operation for operation.  <double, int32>; the other instantiations stay
// the reference's stubs.
#include "../gkomi_bindings.hpp"

namespace gko {
namespace kernels {
namespace hip {
namespace isai {

void generate_tri_inverse(std::shared_ptr<const HipExecutor> exec, const matrix::Csr<double, int32>* input, matrix::Csr<double, int32>* inverse,
                          int32* excess_rhs_ptrs, int32* excess_nz_ptrs, bool lower)
{
    const int64_t n = static_cast<int64_t>(input->get_size()[0]);
    array<char> ws(exec, gkomi_isai_generate_workspace_bytes(n) + 8);
    GKOMI_CALL(gkomi_isai_generate_tri_inverse_f64_i32(GKOMI_NULL_STREAM, n, input->get_const_row_ptrs(), input->get_const_col_idxs(),
                                                       input->get_const_values(), inverse->get_const_row_ptrs(), inverse->get_const_col_idxs(),
                                                       inverse->get_values(), excess_rhs_ptrs, excess_nz_ptrs, lower ? 1 : 0, ws.get_data(),
                                                       ws.get_num_elems()));
    exec->synchronize();  // the workspace leaves scope
}

void generate_general_inverse(std::shared_ptr<const HipExecutor> exec, const matrix::Csr<double, int32>* input,
                              matrix::Csr<double, int32>* inverse, int32* excess_rhs_ptrs, int32* excess_nz_ptrs, bool spd)
{
    const int64_t n = static_cast<int64_t>(input->get_size()[0]);
    array<char> ws(exec, gkomi_isai_generate_workspace_bytes(n) + 8);
    GKOMI_CALL(gkomi_isai_generate_general_inverse_f64_i32(GKOMI_NULL_STREAM, n, input->get_const_row_ptrs(), input->get_const_col_idxs(),
                                                           input->get_const_values(), inverse->get_const_row_ptrs(),
                                                           inverse->get_const_col_idxs(), inverse->get_values(), excess_rhs_ptrs, excess_nz_ptrs,
                                                           spd ? 1 : 0, ws.get_data(), ws.get_num_elems()));
    exec->synchronize();  // the workspace leaves scope
}

void generate_excess_system(std::shared_ptr<const HipExecutor>, const matrix::Csr<double, int32>* input, const matrix::Csr<double, int32>* inverse,
                            const int32* excess_rhs_ptrs, const int32* excess_nz_ptrs, matrix::Csr<double, int32>* excess_system,
                            matrix::Dense<double>* excess_rhs, size_type e_start, size_type e_end)
{
    GKOMI_CALL(gkomi_isai_generate_excess_system_f64_i32(
        GKOMI_NULL_STREAM, static_cast<int64_t>(input->get_size()[0]), input->get_const_row_ptrs(), input->get_const_col_idxs(),
        input->get_const_values(), inverse->get_const_row_ptrs(), inverse->get_const_col_idxs(), excess_rhs_ptrs, excess_nz_ptrs,
        static_cast<int64_t>(excess_rhs->get_size()[0]), static_cast<int64_t>(excess_system->get_num_stored_elements()),
        excess_system->get_row_ptrs(), excess_system->get_col_idxs(), excess_system->get_values(), excess_rhs->get_values(),
        static_cast<int64_t>(e_start), static_cast<int64_t>(e_end)));
}

void scale_excess_solution(std::shared_ptr<const HipExecutor>, const int32* excess_block_ptrs, matrix::Dense<double>* excess_solution,
                           size_type e_start, size_type e_end)
{
    // the kernel's interface has no row count: the range itself bounds what is read
    GKOMI_CALL(gkomi_isai_scale_excess_solution_f64_i32(GKOMI_NULL_STREAM, static_cast<int64_t>(e_end), excess_block_ptrs,
                                                        excess_solution->get_values(), static_cast<int64_t>(e_start),
                                                        static_cast<int64_t>(e_end)));
}

void scatter_excess_solution(std::shared_ptr<const HipExecutor>, const int32* excess_block_ptrs, const matrix::Dense<double>* excess_solution,
                             matrix::Csr<double, int32>* inverse, size_type e_start, size_type e_end)
{
    GKOMI_CALL(gkomi_isai_scatter_excess_solution_f64_i32(GKOMI_NULL_STREAM, static_cast<int64_t>(inverse->get_size()[0]), excess_block_ptrs,
                                                          excess_solution->get_const_values(), inverse->get_const_row_ptrs(),
                                                          inverse->get_values(), static_cast<int64_t>(e_start), static_cast<int64_t>(e_end)));
}

}  // namespace isai
}  // namespace hip
}  // namespace kernels
}  // namespace gko
