// Runs the Pgm shims (shims/hip/multigrid/pgm_kernels.hip.cpp) on the device: Pgm::generate (core/multigrid/pgm.cpp:147-236)
// spelled out with the eleven kernels on the 5 x 5 matrix of reference/test/multigrid/pgm_kernels.cpp:129-181, every step
// held to that file's known answers -- strongest neighbours {2, 0, 0, 1, 2}, agg {0, 1, 0, 1, 0}, the coarse matrix
// {6, -5, -4, 5} -- and its MatchEdge, CountUnagg and Renumber cases.
// Prints one "ran <kernel> ok|WRONG" line per kernel like shim_smoke2.cpp and returns the number of wrong ones.
#include "prelude_mirror.hpp"
#include <cstdio>
#include <vector>

namespace gko { namespace kernels { namespace hip { namespace pgm {
using Csr = matrix::Csr<double, int32>;
using Diag = matrix::Diagonal<double>;
void match_edge(std::shared_ptr<const HipExecutor>, const array<int32>&, array<int32>&);
void count_unagg(std::shared_ptr<const HipExecutor>, const array<int32>&, int32*);
void renumber(std::shared_ptr<const HipExecutor>, array<int32>&, int32*);
void sort_agg(std::shared_ptr<const HipExecutor>, int32, int32*, int32*);
void map_row(std::shared_ptr<const HipExecutor>, size_type, const int32*, const int32*, int32*);
void map_col(std::shared_ptr<const HipExecutor>, size_type, const int32*, const int32*, int32*);
void count_unrepeated_nnz(std::shared_ptr<const HipExecutor>, size_type, const int32*, const int32*, size_type*);
void find_strongest_neighbor(std::shared_ptr<const HipExecutor>, const Csr*, const Diag*, array<int32>&, array<int32>&);
void assign_to_exist_agg(std::shared_ptr<const HipExecutor>, const Csr*, const Diag*, array<int32>&, array<int32>&);
void sort_row_major(std::shared_ptr<const HipExecutor>, size_type, int32*, int32*, double*);
void compute_coarse_coo(std::shared_ptr<const HipExecutor>, size_type, const int32*, const int32*, const double*, matrix::Coo<double, int32>*);
}}}}

using namespace gko;
namespace k = gko::kernels::hip::pgm;

static int wrong = 0;
static void ran(const char* name, bool ok)
{
    std::printf("ran %s %s\n", name, ok ? "ok" : "WRONG");
    if (!ok) ++wrong;
}
template <typename T>
static array<T> on_device(std::shared_ptr<const Executor> exec, const std::vector<T>& v)
{
    return array<T>(exec, v.begin(), v.end());
}
template <typename T>
static std::vector<T> host_of(const Executor* exec, const T* data, size_type n)
{
    std::vector<T> out(n);
    exec->get_master()->copy_from(exec, n, data, out.data());
    return out;
}
template <typename T>
static std::vector<T> host_of(const array<T>& a) { return host_of(a.get_executor().get(), a.get_const_data(), a.get_num_elems()); }

int main()
{
    auto hip = HipExecutor::create(0, ReferenceExecutor::create());
    using ints = std::vector<int32>;
    const ints rp{0, 3, 7, 10, 12, 15}, ci{0, 1, 2, 0, 1, 3, 4, 0, 2, 4, 1, 3, 1, 2, 4};
    const std::vector<double> fine{5, -3, -3, -3, 5, -2, -1, -3, 5, -1, -3, 5, -2, -2, 5};
    const std::vector<double> weights{5, 3, 3, 3, 5, 2.5, 1.5, 3, 5, 1.5, 2.5, 5, 1.5, 1.5, 5};
    auto w = matrix::Csr<double, int32>::create(hip, dim<2>(5, 5), 15);
    auto host = hip->get_master();
    hip->copy_from(host.get(), 6, rp.data(), w->get_row_ptrs());
    hip->copy_from(host.get(), 15, ci.data(), w->get_col_idxs());
    hip->copy_from(host.get(), 15, weights.data(), w->get_values());
    auto diag = matrix::Diagonal<double>::create(hip, 5);
    const std::vector<double> fives(5, 5.0);
    hip->copy_from(host.get(), 5, fives.data(), diag->get_values());
    {   // the reference's MatchEdge, CountUnagg and Renumber cases
        auto agg = on_device(hip, ints{-1, -1, -1, -1, -1});
        k::match_edge(hip, on_device(hip, ints{2, 0, 0, 1, 4}), agg);
        ran("pgm::match_edge", host_of(agg) == ints{0, -1, 0, -1, 4});
        int32 count = -1;
        k::count_unagg(hip, on_device(hip, ints{0, -1, 0, -1, -1}), &count);
        ran("pgm::count_unagg", count == 3);
        agg = on_device(hip, ints{0, 1, 0, 1, 4});
        k::renumber(hip, agg, &count);
        ran("pgm::renumber", count == 3 && host_of(agg) == ints{0, 1, 0, 1, 2});
    }
    // generate, max_iterations 2: two rounds leave row 4, which joins aggregate 0 through column 2 (the tie with column 1)
    auto agg = on_device(hip, ints{-1, -1, -1, -1, -1}), strongest = on_device(hip, ints{-1, -1, -1, -1, -1});
    array<int32> none(hip, 0);
    k::find_strongest_neighbor(hip, w.get(), diag.get(), agg, strongest);
    ran("pgm::find_strongest_neighbor", host_of(strongest) == ints{2, 0, 0, 1, 2} && host_of(agg) == ints{-1, -1, -1, -1, -1});
    k::match_edge(hip, strongest, agg);
    k::find_strongest_neighbor(hip, w.get(), diag.get(), agg, strongest);
    k::match_edge(hip, strongest, agg);
    bool two_rounds = host_of(agg) == ints{0, 1, 0, 1, -1};
    k::assign_to_exist_agg(hip, w.get(), diag.get(), agg, none);
    auto snapshot = on_device(hip, ints{0, 1, 0, 1, -1}), through = on_device(hip, ints{9, 9, 9, 9, 9});
    k::assign_to_exist_agg(hip, w.get(), diag.get(), snapshot, through);
    ran("pgm::assign_to_exist_agg", two_rounds && host_of(agg) == ints{0, 1, 0, 1, 0} && host_of(snapshot) == ints{0, 1, 0, 1, 0});
    int32 num_agg = 0;
    k::renumber(hip, agg, &num_agg);
    {   // the restriction: (agg[i], i) sorted
        auto rows = on_device(hip, host_of(agg)), cols = on_device(hip, ints{0, 1, 2, 3, 4});
        k::sort_agg(hip, 5, rows.get_data(), cols.get_data());
        ran("pgm::sort_agg", num_agg == 2 && host_of(rows) == ints{0, 0, 0, 1, 1} && host_of(cols) == ints{0, 2, 4, 1, 3});
    }
    array<int32> rows(hip, 15), cols(hip, 15);
    auto vals = on_device(hip, fine);
    auto drp = on_device(hip, rp), dci = on_device(hip, ci);
    k::map_row(hip, 5, drp.get_const_data(), agg.get_const_data(), rows.get_data());
    ran("pgm::map_row", host_of(rows) == ints{0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0});
    k::map_col(hip, 15, dci.get_const_data(), agg.get_const_data(), cols.get_data());
    ran("pgm::map_col", host_of(cols) == ints{0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 1, 0, 0});
    k::sort_row_major(hip, 15, rows.get_data(), cols.get_data(), vals.get_data());
    ran("pgm::sort_row_major", host_of(rows) == ints{0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1} &&
                                   host_of(cols) == ints{0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 1, 1, 1} &&
                                   host_of(vals) == std::vector<double>{5, -3, -3, 5, -1, -2, 5, -3, -2, -3, -1, 5, -2, -3, 5});
    size_type coarse_nnz = 0;
    k::count_unrepeated_nnz(hip, 15, rows.get_const_data(), cols.get_const_data(), &coarse_nnz);
    ran("pgm::count_unrepeated_nnz", coarse_nnz == 4);
    auto coo = matrix::Coo<double, int32>::create(hip, dim<2>(2, 2), 4);
    k::compute_coarse_coo(hip, 15, rows.get_const_data(), cols.get_const_data(), vals.get_const_data(), coo.get());
    ran("pgm::compute_coarse_coo", host_of(hip.get(), coo->get_const_row_idxs(), 4) == ints{0, 0, 1, 1} &&
                                       host_of(hip.get(), coo->get_const_col_idxs(), 4) == ints{0, 1, 0, 1} &&
                                       host_of(hip.get(), coo->get_const_values(), 4) == std::vector<double>{6, -5, -4, 5});
    return wrong;
}
