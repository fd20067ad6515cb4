// hip/solver/multigrid_kernels.hip.cpp: the three kernels of core/solver/multigrid_kernels.hpp for double.  Every Dense
// goes through as get_values() / get_stride(); check_stop's bool& is one device byte read back here, the only
// synchronisation (the reference's HIP kernel reads its flag back the same way).
#include "../gkomi_bindings.hpp"

namespace gko {
namespace kernels {
namespace hip {
namespace multigrid {
namespace {
using Vec = matrix::Dense<double>;
#define V(m) (m)->get_values(), (m)->get_stride()
#define C(m) (m)->get_const_values(), (m)->get_stride()
}  // namespace

void kcycle_step_1(std::shared_ptr<const HipExecutor> exec, const Vec* alpha, const Vec* rho, const Vec* v, Vec* g, Vec* d, Vec* e)
{
    GKOMI_CALL(gkomi_multigrid_kcycle_step_1_f64(GKOMI_NULL_STREAM, g->get_size()[0], g->get_size()[1], alpha->get_const_values(),
                                                 rho->get_const_values(), C(v), V(g), V(d), V(e)));
}

void kcycle_step_2(std::shared_ptr<const HipExecutor> exec, const Vec* alpha, const Vec* rho, const Vec* gamma, const Vec* beta,
                   const Vec* zeta, const Vec* d, Vec* e)
{
    GKOMI_CALL(gkomi_multigrid_kcycle_step_2_f64(GKOMI_NULL_STREAM, e->get_size()[0], e->get_size()[1], alpha->get_const_values(),
                                                 rho->get_const_values(), gamma->get_const_values(), beta->get_const_values(),
                                                 zeta->get_const_values(), C(d), V(e)));
}

void kcycle_check_stop(std::shared_ptr<const HipExecutor> exec, const Vec* old_norm, const Vec* new_norm, const double rel_tol,
                       bool& is_stop)
{
    array<char> flag(exec, 1);
    GKOMI_CALL(gkomi_multigrid_kcycle_check_stop_f64(GKOMI_NULL_STREAM, old_norm->get_size()[1], old_norm->get_const_values(),
                                                     new_norm->get_const_values(), rel_tol,
                                                     reinterpret_cast<uint8_t*>(flag.get_data())));
    char host = 0;
    exec->get_master()->copy_from(exec.get(), 1, flag.get_const_data(), &host);
    is_stop = host != 0;
}

#undef V
#undef C
}  // namespace multigrid
}  // namespace hip
}  // namespace kernels
}  // namespace gko
