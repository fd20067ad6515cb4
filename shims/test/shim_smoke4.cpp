// Runs the Fbcsr shims (shims/hip/matrix/fbcsr_kernels.hip.cpp) on the device, each once, on a 6 x 8 matrix of 2 x 2
// blocks with unsorted block columns whose results are known in closed form.  Prints one "ran <kernel> ok|WRONG" line
// per kernel like shim_smoke2.cpp and returns the number of wrong ones.
#include "prelude_mirror.hpp"
#include <cstdio>
#include <vector>

namespace gko { namespace kernels { namespace hip {
using Vec = matrix::Dense<double>;
using Fb = matrix::Fbcsr<double, int32>;
namespace fbcsr {
void spmv(std::shared_ptr<const HipExecutor>, const Fb*, const Vec*, Vec*);
void advanced_spmv(std::shared_ptr<const HipExecutor>, const Vec*, const Fb*, const Vec*, const Vec*, Vec*);
void fill_in_matrix_data(std::shared_ptr<const HipExecutor>, device_matrix_data<double, int32>&, int, array<int32>&, array<int32>&, array<double>&);
void fill_in_dense(std::shared_ptr<const HipExecutor>, const Fb*, Vec*);
void convert_to_csr(std::shared_ptr<const HipExecutor>, const Fb*, matrix::Csr<double, int32>*);
void transpose(std::shared_ptr<const HipExecutor>, const Fb*, Fb*);
void conj_transpose(std::shared_ptr<const HipExecutor>, const Fb*, Fb*);
void is_sorted_by_column_index(std::shared_ptr<const HipExecutor>, const Fb*, bool*);
void sort_by_column_index(std::shared_ptr<const HipExecutor>, Fb*);
void extract_diagonal(std::shared_ptr<const HipExecutor>, const Fb*, matrix::Diagonal<double>*);
}
namespace csr {
void convert_to_fbcsr(std::shared_ptr<const HipExecutor>, const matrix::Csr<double, int32>*, int, array<int32>&, array<int32>&, array<double>&);
}
}}}

using namespace gko;
namespace k = gko::kernels::hip;
using Vec = matrix::Dense<double>;
using Fb = matrix::Fbcsr<double, int32>;

static int wrong = 0;
static void ran(const char* name, bool ok)
{
    std::printf("ran %s %s\n", name, ok ? "ok" : "WRONG");
    if (!ok) ++wrong;
}
template <typename T>
static bool same(const std::vector<T>& a, std::initializer_list<T> b) { return a == std::vector<T>(b); }
template <typename T>
static void upload(std::shared_ptr<const Executor> exec, T* dst, std::vector<T> src)
{
    exec->copy_from(exec->get_master().get(), src.size(), src.data(), dst);
}
template <typename T>
static std::vector<T> download(std::shared_ptr<const Executor> exec, const T* src, size_type n)
{
    std::vector<T> out(n);
    if (n) exec->get_master()->copy_from(exec.get(), n, src, out.data());
    return out;
}
static std::vector<double> host_of(const Vec* v)
{
    auto h = v->clone(v->get_executor()->get_master());
    std::vector<double> out;
    for (size_type i = 0; i < v->get_size()[0]; ++i)
        for (size_type j = 0; j < v->get_size()[1]; ++j) out.push_back(h->at(i, j));
    return out;
}

int main()
{
    auto hip = HipExecutor::create(0, ReferenceExecutor::create());
    // block rows: 0: (col 2: [1 3; 2 4]), (col 0: [5 7; 6 8]);  1: none;  2: (col 2: [9 11; 10 12]); blocks column-major
    auto a = Fb::create(hip, dim<2>(6, 8), 12, 2);
    upload<int32>(hip, a->get_row_ptrs(), {0, 2, 2, 3});
    upload<int32>(hip, a->get_col_idxs(), {2, 0, 2});
    upload<double>(hip, a->get_values(), {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12});
    auto b = Vec::create(hip, dim<2>(8, 1));
    b->fill(1.0);
    {
        auto c = Vec::create(hip, dim<2>(6, 1));
        c->fill(-1.0);
        k::fbcsr::spmv(hip, a.get(), b.get(), c.get());
        ran("fbcsr::spmv", same(host_of(c.get()), {16.0, 20.0, 0.0, 0.0, 20.0, 22.0}));
        auto alpha = initialize<Vec>({2.0}, hip), beta = initialize<Vec>({-1.0}, hip);
        c->fill(1.0);
        k::fbcsr::advanced_spmv(hip, alpha.get(), a.get(), b.get(), beta.get(), c.get());
        ran("fbcsr::advanced_spmv", same(host_of(c.get()), {31.0, 39.0, -1.0, -1.0, 39.0, 43.0}));
    }
    {
        auto d = Vec::create(hip, dim<2>(6, 8));
        d->fill(0.0);
        k::fbcsr::fill_in_dense(hip, a.get(), d.get());
        const auto h = host_of(d.get());
        ran("fbcsr::fill_in_dense", h[0 * 8 + 4] == 1.0 && h[0 * 8 + 5] == 3.0 && h[1 * 8 + 4] == 2.0 && h[1 * 8 + 0] == 6.0 && h[5 * 8 + 5] == 12.0 && h[2 * 8 + 4] == 0.0);
    }
    auto csr = matrix::Csr<double, int32>::create(hip, dim<2>(6, 8), 12);
    {
        k::fbcsr::convert_to_csr(hip, a.get(), csr.get());
        ran("fbcsr::convert_to_csr", same(download(hip, csr->get_const_row_ptrs(), 7), {0, 4, 8, 8, 8, 10, 12}) &&
                                         same(download(hip, csr->get_const_col_idxs(), 12), {4, 5, 0, 1, 4, 5, 0, 1, 4, 5, 4, 5}) &&
                                         same(download(hip, csr->get_const_values(), 12), {1.0, 3.0, 5.0, 7.0, 2.0, 4.0, 6.0, 8.0, 9.0, 11.0, 10.0, 12.0}));
    }
    {
        // csr -> fbcsr sorts the block columns: (col 0), (col 2) in block row 0
        array<int32> rp(hip), ci(hip);
        array<double> v(hip);
        k::csr::convert_to_fbcsr(hip, csr.get(), 2, rp, ci, v);
        const bool ok = same(rp.to_host(), {0, 2, 2, 3}) && same(ci.to_host(), {0, 2, 2}) &&
                        same(v.to_host(), {5.0, 6.0, 7.0, 8.0, 1.0, 2.0, 3.0, 4.0, 9.0, 10.0, 11.0, 12.0});
        ran("csr::convert_to_fbcsr", ok);
        // the same entries as sorted triplets, one of them left out: an explicit zero in its block
        matrix_data<double, int32> md;
        md.size = dim<2>(6, 8);
        md.nonzeros = {{0, 0, 5.0}, {0, 1, 7.0}, {0, 4, 1.0}, {0, 5, 3.0}, {1, 0, 6.0}, {1, 4, 2.0}, {1, 5, 4.0}, {4, 4, 9.0}, {4, 5, 11.0}, {5, 4, 10.0}, {5, 5, 12.0}};
        auto dmd = device_matrix_data<double, int32>::create_from_host(hip, md);
        array<int32> rp2(hip), ci2(hip);
        array<double> v2(hip);
        k::fbcsr::fill_in_matrix_data(hip, dmd, 2, rp2, ci2, v2);
        ran("fbcsr::fill_in_matrix_data", same(rp2.to_host(), {0, 2, 2, 3}) && same(ci2.to_host(), {0, 2, 2}) &&
                                              same(v2.to_host(), {5.0, 6.0, 7.0, 0.0, 1.0, 2.0, 3.0, 4.0, 9.0, 10.0, 11.0, 12.0}));
    }
    {
        // block column 0 <- (row 0), block column 2 <- (row 0), (row 2), every block transposed
        auto t = Fb::create(hip, dim<2>(8, 6), 12, 2);
        k::fbcsr::transpose(hip, a.get(), t.get());
        const bool ok = same(download(hip, t->get_const_row_ptrs(), 5), {0, 1, 1, 3, 3}) && same(download(hip, t->get_const_col_idxs(), 3), {0, 0, 2}) &&
                        same(download(hip, t->get_const_values(), 12), {5.0, 7.0, 6.0, 8.0, 1.0, 3.0, 2.0, 4.0, 9.0, 11.0, 10.0, 12.0});
        ran("fbcsr::transpose", ok);
        auto t2 = Fb::create(hip, dim<2>(8, 6), 12, 2);
        k::fbcsr::conj_transpose(hip, a.get(), t2.get());
        ran("fbcsr::conj_transpose", download(hip, t2->get_const_values(), 12) == download(hip, t->get_const_values(), 12) &&
                                         download(hip, t2->get_const_col_idxs(), 3) == download(hip, t->get_const_col_idxs(), 3));
    }
    {
        auto d = matrix::Diagonal<double>::create(hip, 6);
        upload<double>(hip, d->get_values(), {-1, -1, -1, -1, -1, -1});
        k::fbcsr::extract_diagonal(hip, a.get(), d.get());
        // stored diagonal blocks: (0, 0) and (2, 2); block row 1 is not written
        ran("fbcsr::extract_diagonal", same(download(hip, d->get_const_values(), 6), {5.0, 8.0, -1.0, -1.0, 9.0, 12.0}));
    }
    {
        bool before = true, after = false;
        k::fbcsr::is_sorted_by_column_index(hip, a.get(), &before);
        k::fbcsr::sort_by_column_index(hip, a.get());
        k::fbcsr::is_sorted_by_column_index(hip, a.get(), &after);
        ran("fbcsr::is_sorted_by_column_index", !before && after);
        ran("fbcsr::sort_by_column_index", same(download(hip, a->get_const_col_idxs(), 3), {0, 2, 2}) &&
                                               same(download(hip, a->get_const_values(), 12), {5.0, 6.0, 7.0, 8.0, 1.0, 2.0, 3.0, 4.0, 9.0, 10.0, 11.0, 12.0}));
    }
    return wrong;
}
