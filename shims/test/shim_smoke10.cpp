// Runs the five ISAI shims (shims/hip/preconditioner/isai_kernels.hip.cpp) on the device on matrices whose answers are
// exactly representable and follow by hand from reference/preconditioner/isai_kernels.cpp:
//   lower    L = {{2, 0, 0}, {1, -2, 0}, {-1, 1, -1}}: L^-1 = {{.5, 0, 0}, {.25, -.5, 0}, {-.25, -.5, -1}} on L's pattern;
//   general  diag(2, 4) -> diag(.5, .25); spd: {{4}} -> (1 / 4) / sqrt(1 / 4) = .5;
//   excess   the 34 x 34 identity whose last row holds 34 ones: that row is over the limit of 32, so the prefix arrays end
//            in 34 entries and 33 + 34 matches; its excess system has one entry 1 in each of the rows 0 ... 32, 34 entries
//            1 in row 33, and the right-hand side e_33;
//   scale    block {3, 4} times 1 / sqrt(4); scatter: block {11, 12} becomes row 1 of a matrix with rows {1}, {2, 3}, {4}.
// Prints one "ran <kernel> ok|WRONG" line per kernel like shim_smoke9.cpp and returns the number of wrong ones.
#include "prelude_mirror.hpp"
#include <cstdio>
#include <vector>

namespace gko { namespace kernels { namespace hip { namespace isai {
void generate_tri_inverse(std::shared_ptr<const HipExecutor>, const matrix::Csr<double, int32>*, matrix::Csr<double, int32>*, int32*, int32*, bool);
void generate_general_inverse(std::shared_ptr<const HipExecutor>, const matrix::Csr<double, int32>*, matrix::Csr<double, int32>*, int32*, int32*, bool);
void generate_excess_system(std::shared_ptr<const HipExecutor>, const matrix::Csr<double, int32>*, const matrix::Csr<double, int32>*, const int32*, const int32*,
                            matrix::Csr<double, int32>*, matrix::Dense<double>*, size_type, size_type);
void scale_excess_solution(std::shared_ptr<const HipExecutor>, const int32*, matrix::Dense<double>*, size_type, size_type);
void scatter_excess_solution(std::shared_ptr<const HipExecutor>, const int32*, const matrix::Dense<double>*, matrix::Csr<double, int32>*, size_type, size_type);
}}}}

using namespace gko;
using SpMtx = matrix::Csr<double, int32>;
using Vec = matrix::Dense<double>;

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

static std::unique_ptr<Vec> column(std::shared_ptr<const HipExecutor> hip, std::vector<double> v)
{
    auto x = Vec::create(hip, dim<2>(v.size(), 1));
    hip->copy_from(hip->get_master().get(), v.size(), v.data(), x->get_values());
    return x;
}

int main()
{
    auto hip = HipExecutor::create(0, ReferenceExecutor::create());
    namespace k = gko::kernels::hip::isai;
    {
        auto l = make(hip, {0, 1, 3, 6}, {0, 0, 1, 0, 1, 2}, {2, 1, -2, -1, 1, -1});
        auto inv = make(hip, {0, 1, 3, 6}, {0, 0, 1, 0, 1, 2}, {-1, -1, -1, -1, -1, -1});
        array<int32> a1(hip, 4), a2(hip, 4);
        k::generate_tri_inverse(hip, l.get(), inv.get(), a1.get_data(), a2.get_data(), true);
        ran("isai::generate_tri_inverse", to_host<double>(hip, inv->get_const_values(), 6) == std::vector<double>({.5, .25, -.5, -.25, -.5, -1}) &&
                                              a1.to_host() == std::vector<int32>(4, 0) && a2.to_host() == std::vector<int32>(4, 0));
    }
    {
        auto d = make(hip, {0, 1, 2}, {0, 1}, {2, 4});
        auto inv = make(hip, {0, 1, 2}, {0, 1}, {-1, -1});
        array<int32> a1(hip, 3), a2(hip, 3);
        k::generate_general_inverse(hip, d.get(), inv.get(), a1.get_data(), a2.get_data(), false);
        bool ok = to_host<double>(hip, inv->get_const_values(), 2) == std::vector<double>({.5, .25}) && a1.to_host() == std::vector<int32>(3, 0);
        auto s = make(hip, {0, 1}, {0}, {4});
        auto sinv = make(hip, {0, 1}, {0}, {-1});
        array<int32> b1(hip, 2), b2(hip, 2);
        k::generate_general_inverse(hip, s.get(), sinv.get(), b1.get_data(), b2.get_data(), true);
        ok = ok && to_host<double>(hip, sinv->get_const_values(), 1) == std::vector<double>({.5});
        ran("isai::generate_general_inverse", ok);
    }
    {
        const int32 n = 34;
        std::vector<int32> rp(n + 1), ci;
        for (int32 r = 0; r < n - 1; ++r) {
            rp[r] = r;
            ci.push_back(r);
        }
        rp[n - 1] = n - 1;
        for (int32 c = 0; c < n; ++c) ci.push_back(c);
        rp[n] = static_cast<int32>(ci.size());
        auto m = make(hip, rp, ci, std::vector<double>(ci.size(), 1.0));
        auto inv = make(hip, rp, ci, std::vector<double>(ci.size(), 0.0));
        array<int32> a1(hip, n + 1), a2(hip, n + 1);
        k::generate_tri_inverse(hip, m.get(), inv.get(), a1.get_data(), a2.get_data(), true);
        std::vector<int32> e1(n + 1, 0), e2(n + 1, 0);
        e1[n] = n;
        e2[n] = 2 * n - 1;
        bool ok = a1.to_host() == e1 && a2.to_host() == e2;
        auto sys = SpMtx::create(hip, dim<2>(n, n), 2 * n - 1);
        auto rhs = Vec::create(hip, dim<2>(n, 1));
        k::generate_excess_system(hip, m.get(), inv.get(), a1.get_const_data(), a2.get_const_data(), sys.get(), rhs.get(), 0, n);
        hip->synchronize();
        std::vector<double> want_rhs(n, 0.0);
        want_rhs[n - 1] = 1.0;
        ok = ok && to_host<int32>(hip, sys->get_const_row_ptrs(), n + 1) == to_host<int32>(hip, m->get_const_row_ptrs(), n + 1) &&
             to_host<int32>(hip, sys->get_const_col_idxs(), 2 * n - 1) == ci &&
             to_host<double>(hip, sys->get_const_values(), 2 * n - 1) == std::vector<double>(2 * n - 1, 1.0) &&
             to_host<double>(hip, rhs->get_const_values(), n) == want_rhs;
        ran("isai::generate_excess_system", ok);
    }
    {
        array<int32> ptrs(hip, {0, 0, 2, 2});
        auto sol = column(hip, {3, 4});
        k::scale_excess_solution(hip, ptrs.get_const_data(), sol.get(), 0, 3);
        hip->synchronize();
        ran("isai::scale_excess_solution", to_host<double>(hip, sol->get_const_values(), 2) == std::vector<double>({1.5, 2}));
        auto inv = make(hip, {0, 1, 3, 4}, {0, 0, 1, 2}, {1, 2, 3, 4});
        auto block = column(hip, {11, 12});
        k::scatter_excess_solution(hip, ptrs.get_const_data(), block.get(), inv.get(), 0, 3);
        hip->synchronize();
        ran("isai::scatter_excess_solution", to_host<double>(hip, inv->get_const_values(), 4) == std::vector<double>({1, 11, 12, 4}));
    }
    return wrong;
}
