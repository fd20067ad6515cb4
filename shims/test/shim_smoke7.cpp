// Runs the direct solver's shims (shims/hip/factorization/cholesky_kernels.hip.cpp, lu_kernels.hip.cpp) on the
// device on the 10 x 10 "Example" pattern of the reference's own test (reference/test/factorization/cholesky_kernels.cpp:
// 86-149: row_nnz and the pattern of L), then lu_factorization::initialize / factorize on the 3 x 3 matrix of
// shim_smoke6.cpp, whose factors are exactly representable.  Prints one "ran <kernel> ok|WRONG" line per kernel like
// shim_smoke2.cpp and returns the number of wrong ones.
#include "prelude_mirror.hpp"
#include <algorithm>
#include <cstdio>
#include <vector>

namespace gko { namespace kernels { namespace hip {
namespace cholesky {
void cholesky_symbolic_count(std::shared_ptr<const HipExecutor>, const matrix::Csr<double, int32>*, const factorization::elimination_forest<int32>&, int32*,
                             array<int32>&);
void cholesky_symbolic_factorize(std::shared_ptr<const HipExecutor>, const matrix::Csr<double, int32>*, const factorization::elimination_forest<int32>&,
                                 matrix::Csr<double, int32>*, const array<int32>&);
}
namespace lu_factorization {
void initialize(std::shared_ptr<const HipExecutor>, const matrix::Csr<double, int32>*, const int32*, const int64*, const int32*, int32*, matrix::Csr<double, int32>*);
void factorize(std::shared_ptr<const HipExecutor>, const int32*, const int64*, const int32*, const int32*, matrix::Csr<double, int32>*, array<int>&);
}
}}}

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

static std::unique_ptr<SpMtx> make(std::shared_ptr<const HipExecutor> hip, dim<2> size, std::vector<int32> rp, std::vector<int32> ci, std::vector<double> v)
{
    auto m = SpMtx::create(hip, size, v.size());
    auto host = hip->get_master().get();
    hip->copy_from(host, rp.size(), rp.data(), m->get_row_ptrs());
    hip->copy_from(host, ci.size(), ci.data(), m->get_col_idxs());
    hip->copy_from(host, v.size(), v.data(), m->get_values());
    return m;
}

int main()
{
    auto hip = HipExecutor::create(0, ReferenceExecutor::create());
    namespace k = gko::kernels::hip;
    {
        const int pattern[10][10] = {{1, 0, 1, 0, 0, 0, 0, 1, 0, 0}, {0, 1, 0, 1, 0, 0, 0, 0, 0, 1}, {1, 0, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 1, 0, 0, 0, 0, 1, 1},
                                     {0, 1, 0, 0, 1, 0, 0, 0, 1, 1}, {0, 0, 0, 0, 0, 1, 0, 1, 0, 0}, {0, 0, 1, 0, 0, 1, 1, 0, 0, 0}, {1, 0, 0, 0, 0, 1, 0, 1, 1, 1},
                                     {0, 0, 0, 1, 1, 0, 0, 1, 1, 0}, {0, 1, 0, 1, 1, 0, 0, 1, 0, 1}};
        const int factor[10][10] = {{1, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 0, 0, 0, 0, 0, 0, 0, 0}, {1, 0, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 1, 0, 0, 0, 0, 0, 0},
                                    {0, 1, 0, 0, 1, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 1, 0, 0, 0, 0}, {0, 0, 1, 0, 0, 1, 1, 0, 0, 0}, {1, 0, 1, 0, 0, 1, 1, 1, 0, 0},
                                    {0, 0, 0, 1, 1, 0, 0, 1, 1, 0}, {0, 1, 0, 1, 1, 0, 0, 1, 1, 1}};
        std::vector<int32> rp{0}, ci;
        std::vector<double> v;
        for (int i = 0; i < 10; ++i) {
            for (int j = 0; j < 10; ++j) {
                if (pattern[i][j]) {
                    ci.push_back(j);
                    v.push_back(1.0);
                }
            }
            rp.push_back(static_cast<int32>(ci.size()));
        }
        auto mtx = make(hip, dim<2>(10, 10), rp, ci, v);
        auto forest = factorization::compute_elim_forest(mtx.get());
        array<int32> row_ptrs(hip, 11), tmp(hip, 0);
        row_ptrs.fill(0);
        k::cholesky::cholesky_symbolic_count(hip, mtx.get(), forest, row_ptrs.get_data(), tmp);
        auto counts = to_host<int32>(hip, row_ptrs.get_const_data(), 10);
        ran("cholesky::cholesky_symbolic_count", counts == std::vector<int32>({1, 1, 2, 1, 2, 1, 3, 5, 4, 6}));
        std::vector<int32> lrp{0};
        for (int i = 0; i < 10; ++i) lrp.push_back(lrp.back() + counts[i]);
        auto l_factor = make(hip, dim<2>(10, 10), lrp, std::vector<int32>(lrp.back(), -1), std::vector<double>(lrp.back(), 0.0));
        k::cholesky::cholesky_symbolic_factorize(hip, mtx.get(), forest, l_factor.get(), tmp);
        auto cols = to_host<int32>(hip, l_factor->get_const_col_idxs(), lrp.back());
        bool ok = lrp.back() == 26;
        for (int i = 0; i < 10 && ok; ++i) {
            std::vector<int32> got(cols.begin() + lrp[i], cols.begin() + lrp[i + 1]), want;
            ok = !got.empty() && got.back() == i;  // the diagonal last
            std::sort(got.begin(), got.end());
            for (int j = 0; j < 10; ++j) {
                if (factor[i][j]) want.push_back(j);
            }
            ok = ok && got == want;
        }
        ran("cholesky::cholesky_symbolic_factorize", ok);
    }
    {
        // {{4, 6, 8}, {2, 2, 5}, {1, 1, 1}} -> L \ U = {{4, 6, 8}, {0.5, -1, 1}, {0.25, 0.5, -1.5}}; A stores the rows
        // unsorted, the factor's pattern is sorted
        auto a = make(hip, dim<2>(3, 3), {0, 3, 6, 9}, {2, 0, 1, 1, 2, 0, 0, 1, 2}, {8, 4, 6, 2, 5, 2, 1, 1, 1});
        auto factors = make(hip, dim<2>(3, 3), {0, 3, 6, 9}, {0, 1, 2, 0, 1, 2, 0, 1, 2}, std::vector<double>(9, -7.0));
        array<int32> diag(hip, 3);
        k::lu_factorization::initialize(hip, a.get(), nullptr, nullptr, nullptr, diag.get_data(), factors.get());
        ran("lu_factorization::initialize", to_host<double>(hip, factors->get_const_values(), 9) == std::vector<double>({4, 6, 8, 2, 2, 5, 1, 1, 1}) &&
                                                to_host<int32>(hip, diag.get_const_data(), 3) == std::vector<int32>({0, 4, 8}));
        array<int> tmp(hip, 0);
        k::lu_factorization::factorize(hip, nullptr, nullptr, nullptr, diag.get_const_data(), factors.get(), tmp);
        ran("lu_factorization::factorize", to_host<double>(hip, factors->get_const_values(), 9) == std::vector<double>({4, 6, 8, 0.5, -1, 1, 0.25, 0.5, -1.5}));
    }
    return wrong;
}
