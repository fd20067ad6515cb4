// Runs the two ParICT shims (shims/hip/factorization/par_ict_kernels.hip.cpp) on the device on 3 x 3 matrices whose
// answers are exactly representable and follow by hand from reference/factorization/par_ict_kernels.cpp:
//   A = {{4, 2, 1}, {2, 5, 0}, {1, 0, 3}}, L = {{2, 0, 0}, {1, 2, 0}, {0, 0, 1}}, so L L^T = {{4, 2, 0}, {2, 5, 0}, {0, 0, 1}}
//   has no entry (2, 0), A has: the candidate l(2, 0) = (1 - 0) / l(0, 0) = 0.5; every other entry is the one L stores.
//   The sweep of A2 = {{4, 2, 2}, {2, 5, 0}, {2, 0, 3.25}} on those candidates: l(0, 0) = sqrt(4), l(1, 0) = 2 / 2,
//   l(1, 1) = sqrt(5 - 1), l(2, 0) = 2 / 2, l(2, 2) = sqrt(3.25 - 1) = 1.5.
// Prints one "ran <kernel> ok|WRONG" line per kernel like shim_smoke8.cpp and returns the number of wrong ones.
#include "prelude_mirror.hpp"
#include <cstdio>
#include <vector>

namespace gko { namespace kernels { namespace hip { namespace par_ict_factorization {
void add_candidates(std::shared_ptr<const HipExecutor>, const matrix::Csr<double, int32>*, const matrix::Csr<double, int32>*, const matrix::Csr<double, int32>*,
                    matrix::Csr<double, int32>*);
void compute_factor(std::shared_ptr<const HipExecutor>, const matrix::Csr<double, int32>*, matrix::Csr<double, int32>*, const matrix::Coo<double, int32>*);
}}}}

using namespace gko;
using SpMtx = matrix::Csr<double, int32>;

static int wrong = 0;
static void ran(const char* name, bool ok)
{
    std::printf("ran %s %s\n", name, ok ? "ok" : "WRONG");
    if (!ok) ++wrong;
}

template <typename T>
static std::vector<T> to_host(std::shared_ptr<const Executor> exec, const T* data, size_type n)
{
    std::vector<T> out(n);
    if (n) exec->get_master()->copy_from(exec.get(), n, data, out.data());
    return out;
}

static std::unique_ptr<SpMtx> make(std::shared_ptr<const HipExecutor> hip, std::vector<int32> rp, std::vector<int32> ci, std::vector<double> v)
{
    auto m = SpMtx::create(hip, dim<2>(rp.size() - 1, rp.size() - 1), v.size());
    auto host = hip->get_master().get();
    hip->copy_from(host, rp.size(), rp.data(), m->get_row_ptrs());
    hip->copy_from(host, ci.size(), ci.data(), m->get_col_idxs());
    hip->copy_from(host, v.size(), v.data(), m->get_values());
    return m;
}

static bool is(std::shared_ptr<const HipExecutor> hip, const SpMtx* m, std::vector<int32> rp, std::vector<int32> ci, std::vector<double> v)
{
    return m->get_num_stored_elements() == v.size() && to_host<int32>(hip, m->get_const_row_ptrs(), rp.size()) == rp &&
           to_host<int32>(hip, m->get_const_col_idxs(), ci.size()) == ci && to_host<double>(hip, m->get_const_values(), v.size()) == v;
}

int main()
{
    auto hip = HipExecutor::create(0, ReferenceExecutor::create());
    namespace k = gko::kernels::hip::par_ict_factorization;
    auto a = make(hip, {0, 3, 5, 7}, {0, 1, 2, 0, 1, 0, 2}, {4, 2, 1, 2, 5, 1, 3});
    auto l = make(hip, {0, 1, 3, 4}, {0, 0, 1, 2}, {2, 1, 2, 1});
    auto lt = l->transpose();
    auto llh = SpMtx::create(hip, dim<2>(3, 3));
    l->apply(lt.get(), llh.get());
    auto l_new = SpMtx::create(hip, dim<2>(3, 3));
    k::add_candidates(hip, llh.get(), a.get(), l.get(), l_new.get());
    ran("par_ict_factorization::add_candidates", is(hip, l_new.get(), {0, 1, 3, 5}, {0, 0, 1, 0, 2}, {2, 1, 2, 0.5, 1}));
    auto a2 = make(hip, {0, 3, 5, 7}, {0, 1, 2, 0, 1, 0, 2}, {4, 2, 2, 2, 5, 2, 3.25});
    k::compute_factor(hip, a2.get(), l_new.get(), nullptr);
    ran("par_ict_factorization::compute_factor", is(hip, l_new.get(), {0, 1, 3, 5}, {0, 0, 1, 0, 2}, {2, 1, 2, 1, 1.5}));
    return wrong;
}
