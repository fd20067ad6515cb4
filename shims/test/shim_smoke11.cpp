// Runs the dense GEMM and transpose shims (shims/hip/matrix/dense_kernels.hip.cpp) on the device, each once, on the
// values of the reference's own tests (reference/test/matrix/dense_kernels.cpp: AppliesToDense :206-221,
// AppliesLinearCombinationToDense :244-263 with the untouched stride slot, NonSquareMatrixIsTransposable :2149-2156).
// Prints one "ran <kernel> ok|WRONG" line per kernel like shim_smoke2.cpp and returns the number of wrong ones.
#include "prelude_mirror.hpp"
#include <cstdio>
#include <vector>

namespace gko { namespace kernels { namespace hip { namespace dense {
using Vec = matrix::Dense<double>;
void simple_apply(std::shared_ptr<const HipExecutor>, const Vec*, const Vec*, Vec*);
void apply(std::shared_ptr<const HipExecutor>, const Vec*, const Vec*, const Vec*, const Vec*, Vec*);
void transpose(std::shared_ptr<const HipExecutor>, const Vec*, Vec*);
void conj_transpose(std::shared_ptr<const HipExecutor>, const Vec*, Vec*);
}}}}

using namespace gko;
namespace k = gko::kernels::hip;
using Vec = matrix::Dense<double>;

static int wrong = 0;
static void ran(const char* name, bool ok)
{
    std::printf("ran %s %s\n", name, ok ? "ok" : "WRONG");
    if (!ok) ++wrong;
}
// a rows x cols matrix on the device whose buffer (rows x stride) holds `buffer`
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
    auto mtx1 = on_device(hip, dim<2>(2, 3), 4, {1.0, 2.0, 3.0, 0.0, 1.5, 2.5, 3.5, 0.0});
    auto mtx2 = on_device(hip, dim<2>(2, 2), 2, {1.0, -1.0, -2.0, 2.0});
    const std::vector<double> mtx3{1.0, 2.0, 3.0, -1.0, 0.5, 1.5, 2.5, 0.0};  // values[3] = -1: the stride slot
    {
        auto c = on_device(hip, dim<2>(2, 3), 4, mtx3);
        k::dense::simple_apply(hip, mtx2.get(), mtx1.get(), c.get());
        ran("dense::simple_apply", buffer_of(c.get()) == std::vector<double>{-0.5, -0.5, -0.5, -1.0, 1.0, 1.0, 1.0, 0.0});
    }
    {
        auto c = on_device(hip, dim<2>(2, 3), 4, mtx3);
        auto alpha = initialize<Vec>({-1.0}, hip), beta = initialize<Vec>({2.0}, hip);
        k::dense::apply(hip, alpha.get(), mtx2.get(), mtx1.get(), beta.get(), c.get());
        ran("dense::apply", buffer_of(c.get()) == std::vector<double>{2.5, 4.5, 6.5, -1.0, 0.0, 2.0, 4.0, 0.0});
    }
    {
        auto mtx4 = on_device(hip, dim<2>(2, 3), 4, {1.0, 3.0, 2.0, 9.0, 0.0, 5.0, 0.0, 9.0});
        const std::vector<double> want{1.0, 0.0, -7.0, 3.0, 5.0, -7.0, 2.0, 0.0, -7.0};
        auto t = on_device(hip, dim<2>(3, 2), 3, std::vector<double>(9, -7.0));
        k::dense::transpose(hip, mtx4.get(), t.get());
        ran("dense::transpose", buffer_of(t.get()) == want);
        auto t2 = on_device(hip, dim<2>(3, 2), 3, std::vector<double>(9, -7.0));
        k::dense::conj_transpose(hip, mtx4.get(), t2.get());
        ran("dense::conj_transpose", buffer_of(t2.get()) == want);
    }
    return wrong;
}
