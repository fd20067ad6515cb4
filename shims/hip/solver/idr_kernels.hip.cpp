// hip/solver/idr_kernels.hip.cpp: the five kernels of core/solver/idr_kernels.hpp for double.  The layouts of the
// library's entry points are the reference's (m: s x (s nrhs); g, u: n x (s nrhs); subspace_vectors: s x n; f, c:
// s x nrhs), so every Dense goes through as get_values() / get_stride(): no copy.
#include "../gkomi_bindings.hpp"

#include <random>
#include <vector>

namespace gko {
namespace kernels {
namespace hip {
namespace {
inline uint8_t* raw(array<stopping_status>* s) { return reinterpret_cast<uint8_t*>(s->get_data()); }
inline const uint8_t* raw(const array<stopping_status>* s) { return reinterpret_cast<const uint8_t*>(s->get_const_data()); }
using Vec = matrix::Dense<double>;
#define V(m) (m)->get_values(), (m)->get_stride()
#define C(m) (m)->get_const_values(), (m)->get_stride()
}  // namespace

namespace idr {

// The library never draws random numbers: without `deterministic` the rows of P are drawn here on the host, as the
// reference executor draws them (reference/solver/idr_kernels.cpp:155-163), and copied over; then m = identity
// pattern, statuses reset, P orthonormalised in row order on the device.
void initialize(std::shared_ptr<const HipExecutor> exec, const size_type nrhs, Vec* m, Vec* subspace_vectors, bool deterministic,
                array<stopping_status>* stop_status)
{
    const auto rows = subspace_vectors->get_size()[0], cols = subspace_vectors->get_size()[1];
    if (!deterministic) {
        std::normal_distribution<double> dist(0.0, 1.0);
        std::default_random_engine gen(std::random_device{}());
        std::vector<double> host(cols);
        for (size_type row = 0; row < rows; ++row) {
            for (auto& value : host) value = dist(gen);
            exec->copy_from(exec->get_master().get(), cols, host.data(), subspace_vectors->get_values() + row * subspace_vectors->get_stride());
        }
    }
    GKOMI_CALL(gkomi_idr_initialize_f64(GKOMI_NULL_STREAM, cols, nrhs, rows, V(m), V(subspace_vectors), raw(stop_status)));
}

void step_1(std::shared_ptr<const HipExecutor> exec, const size_type nrhs, const size_type k, const Vec* m, const Vec* f, const Vec* residual,
            const Vec* g, Vec* c, Vec* v, const array<stopping_status>* stop_status)
{
    GKOMI_CALL(gkomi_idr_step_1_f64(GKOMI_NULL_STREAM, residual->get_size()[0], nrhs, m->get_size()[0], k, C(m), C(f), C(residual), C(g),
                                    V(c), V(v), raw(stop_status)));
}

void step_2(std::shared_ptr<const HipExecutor> exec, const size_type nrhs, const size_type k, const Vec* omega, const Vec* preconditioned_vector,
            const Vec* c, Vec* u, const array<stopping_status>* stop_status)
{
    GKOMI_CALL(gkomi_idr_step_2_f64(GKOMI_NULL_STREAM, u->get_size()[0], nrhs, c->get_size()[0], k, omega->get_const_values(),
                                    C(preconditioned_vector), C(c), V(u), raw(stop_status)));
}

void step_3(std::shared_ptr<const HipExecutor> exec, const size_type nrhs, const size_type k, const Vec* p, Vec* g, Vec* g_k, Vec* u, Vec* m,
            Vec* f, Vec* alpha, Vec* residual, Vec* x, const array<stopping_status>* stop_status)
{
    const size_type s = m->get_size()[0];
    array<char> workspace(exec, gkomi_idr_step_3_workspace_bytes(nrhs, s));
    GKOMI_CALL(gkomi_idr_step_3_f64(GKOMI_NULL_STREAM, g->get_size()[0], nrhs, s, k, C(p), V(g), V(g_k), V(u), V(m), V(f), alpha->get_values(),
                                    V(residual), V(x), raw(stop_status), workspace.get_data(), workspace.get_num_elems()));
}

void compute_omega(std::shared_ptr<const HipExecutor> exec, const size_type nrhs, const double kappa, const Vec* tht, const Vec* residual_norm,
                   Vec* omega, const array<stopping_status>* stop_status)
{
    GKOMI_CALL(gkomi_idr_compute_omega_f64(GKOMI_NULL_STREAM, nrhs, kappa, tht->get_const_values(), residual_norm->get_const_values(),
                                           omega->get_values(), raw(stop_status)));
}

}  // namespace idr
}  // namespace hip
}  // namespace kernels
}  // namespace gko
