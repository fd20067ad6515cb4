// The three sparse-sparse shims of shims/hip/matrix/csr_kernels.hip.cpp, each run once on the device on the
// fixtures of the reference's own tests (reference/test/matrix/csr_kernels.cpp:455-551: mtx 2 x 3, mtx2 with its
// explicit zero, mtx3 with unsorted rows), whose results are known.  Shared by shim_smoke2.cpp (which reports every
// kernel of INTEGRATION.md's list) and shim_smoke5.cpp (these three alone).
#pragma once
#include "prelude_mirror.hpp"
#include <vector>

namespace gko { namespace kernels { namespace hip { namespace csr {
void spgemm(std::shared_ptr<const HipExecutor>, const matrix::Csr<double, int32>*, const matrix::Csr<double, int32>*, matrix::Csr<double, int32>*);
void advanced_spgemm(std::shared_ptr<const HipExecutor>, const matrix::Dense<double>*, const matrix::Csr<double, int32>*, const matrix::Csr<double, int32>*,
                     const matrix::Dense<double>*, const matrix::Csr<double, int32>*, matrix::Csr<double, int32>*);
void spgeam(std::shared_ptr<const HipExecutor>, const matrix::Dense<double>*, const matrix::Csr<double, int32>*, const matrix::Dense<double>*,
            const matrix::Csr<double, int32>*, matrix::Csr<double, int32>*);
}}}}

namespace spgemm_cases {
using namespace gko;
using SpMtx = matrix::Csr<double, int32>;

inline std::unique_ptr<SpMtx> make(std::shared_ptr<const HipExecutor> hip, dim<2> size, std::vector<int32> rp, std::vector<int32> ci, std::vector<double> v)
{
    auto m = SpMtx::create(hip, size, v.size());
    auto host = hip->get_master().get();
    hip->copy_from(host, rp.size(), rp.data(), m->get_row_ptrs());
    hip->copy_from(host, ci.size(), ci.data(), m->get_col_idxs());
    hip->copy_from(host, v.size(), v.data(), m->get_values());
    return m;
}

inline bool holds(const SpMtx* m, const std::vector<int32>& rp, const std::vector<int32>& ci, const std::vector<double>& v)
{
    auto exec = m->get_executor();
    auto host = exec->get_master();
    if (m->get_num_stored_elements() != v.size()) return false;
    std::vector<int32> grp(rp.size()), gci(ci.size());
    std::vector<double> gv(v.size());
    host->copy_from(exec.get(), grp.size(), m->get_const_row_ptrs(), grp.data());
    host->copy_from(exec.get(), gci.size(), m->get_const_col_idxs(), gci.data());
    host->copy_from(exec.get(), gv.size(), m->get_const_values(), gv.data());
    return grp == rp && gci == ci && gv == v;
}

template <typename Report>
void run(std::shared_ptr<const HipExecutor> hip, Report ran)
{
    namespace k = gko::kernels::hip;
    auto mtx = make(hip, dim<2>(2, 3), {0, 3, 4}, {0, 1, 2, 1}, {1.0, 3.0, 2.0, 5.0});
    auto mtx3_unsorted = make(hip, dim<2>(3, 3), {0, 2, 5, 7}, {2, 1, 1, 2, 0, 2, 0}, {1.0, 2.0, 1.0, 8.0, 3.0, 3.0, 2.0});
    auto mtx2 = make(hip, dim<2>(2, 3), {0, 3, 5}, {0, 1, 2, 0, 1}, {1.0, 3.0, 2.0, 0.0, 5.0});
    {
        auto c = SpMtx::create(hip, dim<2>(2, 3));
        k::csr::spgemm(hip, mtx.get(), mtx3_unsorted.get(), c.get());
        ran("csr::spgemm", holds(c.get(), {0, 3, 6}, {0, 1, 2, 0, 1, 2}, {13.0, 5.0, 31.0, 15.0, 5.0, 40.0}));
    }
    {
        auto alpha = initialize<matrix::Dense<double>>({-1.0}, hip), beta = initialize<matrix::Dense<double>>({2.0}, hip);
        auto c = SpMtx::create(hip, dim<2>(2, 3));
        k::csr::advanced_spgemm(hip, alpha.get(), mtx.get(), mtx3_unsorted.get(), beta.get(), mtx2.get(), c.get());
        ran("csr::advanced_spgemm", holds(c.get(), {0, 3, 6}, {0, 1, 2, 0, 1, 2}, {-11.0, 1.0, -27.0, -15.0, 5.0, -40.0}));
    }
    {
        auto alpha = initialize<matrix::Dense<double>>({-3.0}, hip), beta = initialize<matrix::Dense<double>>({2.0}, hip);
        auto a = make(hip, dim<2>(7, 3), {0, 2, 4, 5, 6, 8, 10, 10}, {0, 2, 1, 2, 1, 0, 0, 2, 0, 1}, {2.0, 3.0, 1.0, -1.5, -2.0, 5.0, 1.0, 4.0, 2.0, -2.0});
        auto b = make(hip, dim<2>(7, 3), {0, 2, 4, 6, 8, 9, 9, 9}, {0, 1, 0, 2, 0, 2, 1, 2, 0}, {2.0, -2.0, 1.0, 4.0, 2.0, 3.0, 1.0, -1.5, 1.0});
        auto c = SpMtx::create(hip, dim<2>(7, 3));
        k::csr::spgeam(hip, alpha.get(), a.get(), beta.get(), b.get(), c.get());
        ran("csr::spgeam", holds(c.get(), {0, 3, 6, 9, 12, 14, 16, 16}, {0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 2, 0, 1},
                                 {-2.0, -4.0, -9.0, 2.0, -3.0, 12.5, 4.0, 6.0, 6.0, -15.0, 2.0, -3.0, -1.0, -12.0, -6.0, 6.0}));
    }
}
}  // namespace spgemm_cases
