// Runs the multigrid shims (shims/hip/solver/multigrid_kernels.hip.cpp) on the device, each once, on a 3 x 3 block with
// padded strides whose columns are a plain one, one with rho = 0 (step 1 leaves g and e, d = e is still written) and,
// for step 2, one with beta - gamma^2 / rho = 0 (e is left); the expected values are the expressions of
// reference/solver/multigrid_kernels.cpp:53-119 evaluated on the host in the same order.  check_stop is run at
// new == rel_tol * old (stops) and just above it (does not).
// Prints one "ran <kernel> ok|WRONG" line per kernel like shim_smoke2.cpp and returns the number of wrong ones.
#include "prelude_mirror.hpp"
#include <cmath>
#include <cstdio>
#include <vector>

namespace gko { namespace kernels { namespace hip { namespace multigrid {
using Vec = matrix::Dense<double>;
void kcycle_step_1(std::shared_ptr<const HipExecutor>, const Vec*, const Vec*, const Vec*, Vec*, Vec*, Vec*);
void kcycle_step_2(std::shared_ptr<const HipExecutor>, const Vec*, const Vec*, const Vec*, const Vec*, const Vec*, const Vec*, Vec*);
void kcycle_check_stop(std::shared_ptr<const HipExecutor>, const Vec*, const Vec*, const double, bool&);
}}}}

using namespace gko;
namespace k = gko::kernels::hip::multigrid;
using Vec = matrix::Dense<double>;

static int wrong = 0;
static void ran(const char* name, bool ok)
{
    std::printf("ran %s %s\n", name, ok ? "ok" : "WRONG");
    if (!ok) ++wrong;
}
static std::unique_ptr<Vec> on_device(std::shared_ptr<const Executor> exec, dim<2> size, size_type stride, std::vector<double> buffer)
{
    auto d = Vec::create(exec, size, stride);
    exec->copy_from(exec->get_master().get(), buffer.size(), buffer.data(), d->get_values());
    return d;
}
static std::vector<double> buffer_of(const Vec* v)
{
    std::vector<double> out(v->get_num_stored_elements());
    auto exec = v->get_executor();
    exec->get_master()->copy_from(exec.get(), out.size(), v->get_const_values(), out.data());
    return out;
}

int main()
{
    auto hip = HipExecutor::create(0, ReferenceExecutor::create());
    constexpr size_type n = 3, nrhs = 3, stride = 4;
    const double pad = -9.0;
    const std::vector<double> alpha{1.5, 2.0, 0.75}, rho{2.0, 0.0, 4.0}, gamma{0.5, 0.25, 2.0}, beta{3.0, 1.0, 1.0}, zeta{0.75, 0.5, 0.25};
    std::vector<double> v(n * stride, pad), g(n * stride, pad), d(n * stride, pad), e(n * stride, pad);
    for (size_type i = 0; i < n; ++i) {
        for (size_type j = 0; j < nrhs; ++j) {
            v[i * stride + j] = 1.0 + 0.5 * i - 0.25 * j;
            g[i * stride + j] = 2.0 - 0.125 * i + j;
            d[i * stride + j] = 7.0;
            e[i * stride + j] = 0.5 + i * 0.375 - 0.0625 * j;
        }
    }
    auto row = [&](const std::vector<double>& s) { return on_device(hip, dim<2>(1, nrhs), nrhs, s); };
    auto block = [&](const std::vector<double>& s) { return on_device(hip, dim<2>(n, nrhs), stride, s); };
    {
        auto wg = g, wd = d, we = e;
        for (size_type j = 0; j < nrhs; ++j) {
            const double temp = alpha[j] / rho[j];
            for (size_type i = 0; i < n; ++i) {
                if (std::isfinite(temp)) {
                    wg[i * stride + j] -= temp * v[i * stride + j];
                    we[i * stride + j] *= temp;
                }
                wd[i * stride + j] = we[i * stride + j];
            }
        }
        auto dg = block(g), dd = block(d), de = block(e);
        k::kcycle_step_1(hip, row(alpha).get(), row(rho).get(), block(v).get(), dg.get(), dd.get(), de.get());
        ran("multigrid::kcycle_step_1", buffer_of(dg.get()) == wg && buffer_of(dd.get()) == wd && buffer_of(de.get()) == we &&
                                            wg[1] == g[1] && we[1] == e[1] && wd[1] == e[1]);
    }
    {
        auto we = e;
        for (size_type j = 0; j < nrhs; ++j) {
            const double scalar_d = zeta[j] / (beta[j] - gamma[j] * gamma[j] / rho[j]);
            const double scalar_e = 1.0 - gamma[j] / alpha[j] * scalar_d;
            if (std::isfinite(scalar_d) && std::isfinite(scalar_e)) {
                for (size_type i = 0; i < n; ++i) we[i * stride + j] = scalar_e * e[i * stride + j] + scalar_d * d[i * stride + j];
            }
        }
        auto de = block(e);
        k::kcycle_step_2(hip, row(alpha).get(), row(rho).get(), row(gamma).get(), row(beta).get(), row(zeta).get(), block(d).get(), de.get());
        ran("multigrid::kcycle_step_2", buffer_of(de.get()) == we && we[0] != e[0] && we[2] == e[2]);
    }
    {
        const std::vector<double> old_norm{1.0, 2.0, 3.0};
        std::vector<double> new_norm{0.25, 0.5, 0.75};
        bool equal = false, above = true;
        k::kcycle_check_stop(hip, row(old_norm).get(), row(new_norm).get(), 0.25, equal);
        new_norm[2] = std::nextafter(new_norm[2], 1.0);
        k::kcycle_check_stop(hip, row(old_norm).get(), row(new_norm).get(), 0.25, above);
        ran("multigrid::kcycle_check_stop", equal && !above);
    }
    return wrong;
}
