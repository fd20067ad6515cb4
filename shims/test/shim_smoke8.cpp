// Runs the five ParILUT shims (shims/hip/factorization/par_ilut_kernels.hip.cpp) on the device on 3 x 3 matrices whose
// answers are exactly representable and follow by hand from reference/factorization/par_ilut_kernels.cpp:
//   M = {{0.5, 0, 0}, {-4, 2, 0}, {1, -3, 0.25}}: magnitudes 0.25 0.5 1 2 3 4, so rank 3 selects 2; the filter at 2 keeps
//   -4, 2, -3 and the two small diagonals; the approximate threshold of rank 5 is the largest splitter, 4.
//   A = {{4, 2, 0}, {2, 5, 1}, {1, 0, 3}}, L = {{1, 0, 0}, {0.5, 1, 0}, {0, 0, 1}}, U = {{4, 2, 0}, {0, 4, 1}, {0, 0, 3}}:
//   L U has no entry (2, 0), A has: the candidate l(2, 0) = (1 - 0) / u(0, 0) = 0.25.
//   The sweep of A2 = {{4, 2, 0}, {2, 6, 1}, {2, 0, 3}} on those candidates: l(1, 0) = 2 / 4, u(1, 1) = 6 - 0.5 * 2,
//   l(2, 0) = 2 / 4, everything else as stored.
// Prints one "ran <kernel> ok|WRONG" line per kernel like shim_smoke2.cpp and returns the number of wrong ones.
#include "prelude_mirror.hpp"
#include <cstdio>
#include <vector>

namespace gko { namespace kernels { namespace hip { namespace par_ilut_factorization {
void threshold_select(std::shared_ptr<const HipExecutor>, const matrix::Csr<double, int32>*, int32, array<double>&, array<double>&, double&);
void threshold_filter(std::shared_ptr<const HipExecutor>, const matrix::Csr<double, int32>*, double, matrix::Csr<double, int32>*, matrix::Coo<double, int32>*, bool);
void threshold_filter_approx(std::shared_ptr<const HipExecutor>, const matrix::Csr<double, int32>*, int32, array<double>&, double&, matrix::Csr<double, int32>*,
                             matrix::Coo<double, int32>*);
void compute_l_u_factors(std::shared_ptr<const HipExecutor>, const matrix::Csr<double, int32>*, matrix::Csr<double, int32>*, const matrix::Coo<double, int32>*,
                         matrix::Csr<double, int32>*, const matrix::Coo<double, int32>*, matrix::Csr<double, int32>*);
void add_candidates(std::shared_ptr<const HipExecutor>, const matrix::Csr<double, int32>*, const matrix::Csr<double, int32>*, const matrix::Csr<double, int32>*,
                    const matrix::Csr<double, int32>*, matrix::Csr<double, int32>*, matrix::Csr<double, int32>*);
}}}}

using namespace gko;
using SpMtx = matrix::Csr<double, int32>;
using CooMtx = matrix::Coo<double, int32>;

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
    namespace k = gko::kernels::hip::par_ilut_factorization;
    {
        auto m = make(hip, {0, 1, 3, 6}, {0, 0, 1, 0, 1, 2}, {0.5, -4, 2, 1, -3, 0.25});
        array<double> tmp(hip), tmp2(hip);
        double threshold = -1.0;
        k::threshold_select(hip, m.get(), 3, tmp, tmp2, threshold);
        ran("par_ilut_factorization::threshold_select", threshold == 2.0);
        auto out = SpMtx::create(hip, dim<2>(3, 3));
        auto coo = CooMtx::create(hip, dim<2>(3, 3));
        k::threshold_filter(hip, m.get(), 2.0, out.get(), coo.get(), true);
        ran("par_ilut_factorization::threshold_filter",
            is(hip, out.get(), {0, 1, 3, 5}, {0, 0, 1, 1, 2}, {0.5, -4, 2, -3, 0.25}) &&
                to_host<int32>(hip, coo->get_const_row_idxs(), 5) == std::vector<int32>({0, 1, 1, 2, 2}) &&
                to_host<int32>(hip, coo->get_const_col_idxs(), 5) == std::vector<int32>({0, 0, 1, 1, 2}));
        auto out2 = SpMtx::create(hip, dim<2>(3, 3));
        threshold = -1.0;
        k::threshold_filter_approx(hip, m.get(), 5, tmp, threshold, out2.get(), nullptr);
        ran("par_ilut_factorization::threshold_filter_approx", threshold == 4.0 && is(hip, out2.get(), {0, 1, 3, 4}, {0, 0, 1, 2}, {0.5, -4, 2, 0.25}));
    }
    {
        auto a = make(hip, {0, 2, 5, 7}, {0, 1, 0, 1, 2, 0, 2}, {4, 2, 2, 5, 1, 1, 3});
        auto l = make(hip, {0, 1, 3, 4}, {0, 0, 1, 2}, {1, 0.5, 1, 1});
        auto u = make(hip, {0, 2, 4, 5}, {0, 1, 1, 2, 2}, {4, 2, 4, 1, 3});
        auto lu = SpMtx::create(hip, dim<2>(3, 3));
        l->apply(u.get(), lu.get());
        auto l_new = SpMtx::create(hip, dim<2>(3, 3)), u_new = SpMtx::create(hip, dim<2>(3, 3));
        k::add_candidates(hip, lu.get(), a.get(), l.get(), u.get(), l_new.get(), u_new.get());
        ran("par_ilut_factorization::add_candidates", is(hip, l_new.get(), {0, 1, 3, 5}, {0, 0, 1, 0, 2}, {1, 0.5, 1, 0.25, 1}) &&
                                                           is(hip, u_new.get(), {0, 2, 4, 5}, {0, 1, 1, 2, 2}, {4, 2, 4, 1, 3}));
        auto a2 = make(hip, {0, 2, 5, 7}, {0, 1, 0, 1, 2, 0, 2}, {4, 2, 2, 6, 1, 2, 3});
        auto u_csc = u_new->transpose();
        k::compute_l_u_factors(hip, a2.get(), l_new.get(), nullptr, u_new.get(), nullptr, u_csc.get());
        ran("par_ilut_factorization::compute_l_u_factors", is(hip, l_new.get(), {0, 1, 3, 5}, {0, 0, 1, 0, 2}, {1, 0.5, 1, 0.5, 1}) &&
                                                                is(hip, u_new.get(), {0, 2, 4, 5}, {0, 1, 1, 2, 2}, {4, 2, 5, 1, 3}) &&
                                                                is(hip, u_csc.get(), {0, 1, 3, 5}, {0, 0, 1, 1, 2}, {4, 2, 5, 1, 3}));
    }
    return wrong;
}
