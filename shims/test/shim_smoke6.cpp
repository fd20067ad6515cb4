// Runs the exact-factorization shims (shims/hip/factorization/ilu_kernels.hip.cpp, ic_kernels.hip.cpp) on the device,
// each once on a fixture of the reference's own tests whose factors are exactly representable
// (reference/test/factorization/ilu_kernels.cpp: mtx_small; ic_kernels.cpp: mtx_system's lower triangle with its
// diagonal).  Prints one "ran <kernel> ok|WRONG" line per kernel like shim_smoke2.cpp and returns the number of
// wrong ones.
#include "prelude_mirror.hpp"
#include <cstdio>
#include <vector>

namespace gko { namespace kernels { namespace hip {
namespace ilu_factorization { void compute_lu(std::shared_ptr<const HipExecutor>, matrix::Csr<double, int32>*); }
namespace ic_factorization { void compute(std::shared_ptr<const HipExecutor>, matrix::Csr<double, int32>*); }
}}}

using namespace gko;
using SpMtx = matrix::Csr<double, int32>;

static int wrong = 0;
static void ran(const char* name, bool ok)
{
    std::printf("ran %s %s\n", name, ok ? "ok" : "WRONG");
    if (!ok) ++wrong;
}

static std::unique_ptr<SpMtx> make(std::shared_ptr<const HipExecutor> hip, dim<2> size, std::vector<int32> rp, std::vector<int32> ci,
                                   std::vector<double> v)
{
    auto m = SpMtx::create(hip, size, v.size());
    auto host = hip->get_master().get();
    hip->copy_from(host, rp.size(), rp.data(), m->get_row_ptrs());
    hip->copy_from(host, ci.size(), ci.data(), m->get_col_idxs());
    hip->copy_from(host, v.size(), v.data(), m->get_values());
    return m;
}

static bool holds(const SpMtx* m, const std::vector<double>& v)
{
    auto exec = m->get_executor();
    std::vector<double> gv(v.size());
    exec->get_master()->copy_from(exec.get(), gv.size(), m->get_const_values(), gv.data());
    return gv == v;
}

int main()
{
    auto hip = HipExecutor::create(0, ReferenceExecutor::create());
    namespace k = gko::kernels::hip;
    {
        // {{4, 6, 8}, {2, 2, 5}, {1, 1, 1}} -> L \ U = {{4, 6, 8}, {0.5, -1, 1}, {0.25, 0.5, -1.5}}
        auto m = make(hip, dim<2>(3, 3), {0, 3, 6, 9}, {0, 1, 2, 0, 1, 2, 0, 1, 2}, {4, 6, 8, 2, 2, 5, 1, 1, 1});
        k::ilu_factorization::compute_lu(hip, m.get());
        ran("ilu_factorization::compute_lu", holds(m.get(), {4, 6, 8, 0.5, -1, 1, 0.25, 0.5, -1.5}));
    }
    {
        // {{9, 0, -6, 3}, {0, 36, 18, 24}, {-6, 18, 17, 14}, {-3, 24, 14, 18}}: the lower triangle becomes
        // {{3}, {0, 6}, {-2, 3, 2}, {-1, 4, 0, 1}}, the upper triangle stays
        auto m = make(hip, dim<2>(4, 4), {0, 3, 6, 10, 14}, {0, 2, 3, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3},
                      {9, -6, 3, 36, 18, 24, -6, 18, 17, 14, -3, 24, 14, 18});
        k::ic_factorization::compute(hip, m.get());
        ran("ic_factorization::compute", holds(m.get(), {3, -6, 3, 6, 18, 24, -2, 3, 2, 14, -1, 4, 0, 1}));
    }
    return wrong;
}
