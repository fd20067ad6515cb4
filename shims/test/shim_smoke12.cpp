// Runs the CB-GMRES shims (shims/hip/solver/cb_gmres_kernels.hip.cpp) on the device for each of the six
// <double, storage> accessor instantiations: one GMRES(3) cycle on the 3 x 3 system of the reference's own test
// (reference/test/solver/cb_gmres_kernels.cpp, SolvesStencilSystem: A = [1 2 3; 3 2 -1; 0 -1 2], b = (13, 7, 1),
// x = (1, 3, 2)) from x0 = 0: initialize, restart, three times next = A next and arnoldi, then solve_krylov, whose
// before_preconditioner is x.  initialize and restart are compared exactly (3 rows: every sum order gives the same
// bits), x with that test's precision per storage type (1e-14, 1e-6, 1e-2) times 10, as there.
// Prints one "ran <kernel><storage> ok|WRONG" line per kernel like shim_smoke2.cpp and returns the number of wrong ones.
#include "prelude_cb_gmres.hpp"
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

namespace gko { namespace kernels { namespace hip { namespace cb_gmres {
// the declarations of core/solver/cb_gmres_kernels.hpp:128-169 (a template's name carries its dependent parameter types)
template <typename T> using Vec = matrix::Dense<T>;
template <typename T> using Norms = matrix::Dense<remove_complex<T>>;
template <typename T>
void initialize(std::shared_ptr<const HipExecutor>, const Vec<T>*, Vec<T>*, Vec<T>*, Vec<T>*, array<stopping_status>*, size_type);
template <typename T, typename Accessor3d>
void restart(std::shared_ptr<const HipExecutor>, const Vec<T>*, Norms<T>*, Vec<T>*, Norms<T>*, Accessor3d, Vec<T>*, array<size_type>*, array<char>&,
             size_type);
template <typename T, typename Accessor3d>
void arnoldi(std::shared_ptr<const HipExecutor>, Vec<T>*, Vec<T>*, Vec<T>*, Norms<T>*, Vec<T>*, Accessor3d, Vec<T>*, Vec<T>*, Norms<T>*, size_type,
             array<size_type>*, const array<stopping_status>*, array<stopping_status>*, array<size_type>*);
template <typename T, typename ConstAccessor3d>
void solve_krylov(std::shared_ptr<const HipExecutor>, const Vec<T>*, ConstAccessor3d, const Vec<T>*, Vec<T>*, Vec<T>*, const array<size_type>*);
}}}}

using namespace gko;
namespace k = gko::kernels::hip::cb_gmres;
using Vec = matrix::Dense<double>;

static int wrong = 0;
static void ran(const std::string& name, bool ok)
{
    std::printf("ran %s %s\n", name.c_str(), ok ? "ok" : "WRONG");
    if (!ok) ++wrong;
}
static std::vector<double> buffer_of(const Vec* v)
{
    std::vector<double> out(v->get_num_stored_elements());
    auto exec = v->get_executor();
    exec->get_master()->copy_from(exec.get(), out.size(), v->get_const_values(), out.data());
    return out;
}

constexpr size_type n = 3, krylov_dim = 3;
using dim3d = std::array<size_type, 3>;

template <typename S>
struct reduced {
    using range = acc::range<acc::reduced_row_major<3, double, S>>;
    using const_range = acc::range<acc::reduced_row_major<3, double, const S>>;
    static range make(S* data, double*) { return range(dim3d{{krylov_dim + 1, n, 1}}, data); }
    static const_range make_const(const S* data, const double*) { return const_range(dim3d{{krylov_dim + 1, n, 1}}, data); }
};
template <typename S>
struct scaled {
    using range = acc::range<acc::scaled_reduced_row_major<3, double, S, 0b101>>;
    using const_range = acc::range<acc::scaled_reduced_row_major<3, double, const S, 0b101>>;
    static range make(S* data, double* scalar) { return range(dim3d{{krylov_dim + 1, n, 1}}, data, scalar); }
    static const_range make_const(const S* data, const double* scalar) { return const_range(dim3d{{krylov_dim + 1, n, 1}}, data, scalar); }
};

template <typename S, typename Kind>
static void cycle(std::shared_ptr<const HipExecutor> hip, const std::string& tag, double precision)
{
    auto A = initialize<Vec>({{1.0, 2.0, 3.0}, {3.0, 2.0, -1.0}, {0.0, -1.0, 2.0}}, hip);
    auto b = initialize<Vec>({13.0, 7.0, 1.0}, hip);
    auto residual = Vec::create(hip, dim<2>(n, 1)), next = Vec::create(hip, dim<2>(n, 1)), image = Vec::create(hip, dim<2>(n, 1));
    auto before = Vec::create(hip, dim<2>(n, 1));
    auto hessenberg = Vec::create(hip, dim<2>(krylov_dim + 1, krylov_dim)), buffer = Vec::create(hip, dim<2>(krylov_dim + 1, 1));
    auto givens_sin = Vec::create(hip, dim<2>(krylov_dim, 1)), givens_cos = Vec::create(hip, dim<2>(krylov_dim, 1));
    auto collection = Vec::create(hip, dim<2>(krylov_dim + 1, 1)), residual_norm = Vec::create(hip, dim<2>(1, 1));
    auto arnoldi_norm = Vec::create(hip, dim<2>(3, 1)), y = Vec::create(hip, dim<2>(krylov_dim, 1));
    hessenberg->fill(0.0);
    givens_sin->fill(-1.0);
    array<S> basis(hip, (krylov_dim + 1) * n);
    array<double> scalars(hip, krylov_dim + 1);
    scalars.fill(1.0);
    array<size_type> final_iter_nums(hip, 1), num_reorth(hip, 1);
    array<stopping_status> stop_status(hip, 1), reorth_status(hip, 1);
    array<char> reduction_tmp(hip);
    auto bases = Kind::make(basis.get_data(), scalars.get_data());

    k::initialize<double>(hip, b.get(), residual.get(), givens_sin.get(), givens_cos.get(), &stop_status, krylov_dim);
    ran("cb_gmres::initialize" + tag, buffer_of(residual.get()) == std::vector<double>{13.0, 7.0, 1.0} &&
                                          buffer_of(givens_sin.get()) == std::vector<double>(krylov_dim, 0.0) &&
                                          buffer_of(givens_cos.get()) == std::vector<double>(krylov_dim, 0.0) &&
                                          stop_status.to_host()[0].data_ == 0);

    k::restart<double>(hip, residual.get(), residual_norm.get(), collection.get(), arnoldi_norm.get(), bases, next.get(), &final_iter_nums,
                       reduction_tmp, krylov_dim);
    const double norm = std::sqrt(219.0);
    ran("cb_gmres::restart" + tag, buffer_of(residual_norm.get()) == std::vector<double>{norm} &&
                                       buffer_of(collection.get()) == std::vector<double>{norm, 0.0, 0.0, 0.0} &&
                                       buffer_of(next.get()) == std::vector<double>{13.0 / norm, 7.0 / norm, 1.0 / norm} &&
                                       final_iter_nums.to_host()[0] == 0);

    for (size_type iter = 0; iter < krylov_dim; ++iter) {
        A->apply(next.get(), image.get());
        next->copy_from(image.get());
        // rows 0..iter+1 of column iter of hessenberg, with hessenberg's stride
        auto h_iter = Vec::create(hip, dim<2>(iter + 2, 1),
                                  array<double>::view(hip, (iter + 1) * krylov_dim + 1, hessenberg->get_values() + iter), krylov_dim);
        auto buffer_iter = Vec::create(hip, dim<2>(iter + 2, 1), array<double>::view(hip, iter + 2, buffer->get_values()), 1);
        k::arnoldi<double>(hip, next.get(), givens_sin.get(), givens_cos.get(), residual_norm.get(), collection.get(), bases, h_iter.get(),
                           buffer_iter.get(), arnoldi_norm.get(), iter, &final_iter_nums, &stop_status, &reorth_status, &num_reorth);
    }
    // the implicit residual norm after a full cycle on a 3 x 3 system, and the iteration count of the column
    const double left = std::abs(buffer_of(residual_norm.get())[0]);
    ran("cb_gmres::arnoldi" + tag, final_iter_nums.to_host()[0] == krylov_dim && left <= 10 * precision * norm);

    k::solve_krylov<double>(hip, collection.get(), Kind::make_const(basis.get_const_data(), scalars.get_const_data()), hessenberg.get(), y.get(),
                            before.get(), &final_iter_nums);
    const auto x = buffer_of(before.get());
    const double want[3] = {1.0, 3.0, 2.0};
    double err = 0.0;
    for (size_type i = 0; i < n; ++i) err += (x[i] - want[i]) * (x[i] - want[i]);
    ran("cb_gmres::solve_krylov" + tag, std::sqrt(err) <= 10 * precision * std::sqrt(14.0));
}

int main()
{
    auto hip = HipExecutor::create(0, ReferenceExecutor::create());
    cycle<double, reduced<double>>(hip, "<double>", 1e-14);
    cycle<float, reduced<float>>(hip, "<float>", 1e-6);
    cycle<half, reduced<half>>(hip, "<half>", 1e-2);
    cycle<int64, scaled<int64>>(hip, "<int64>", 1e-14);
    cycle<int32, scaled<int32>>(hip, "<int32>", 1e-6);
    cycle<int16, scaled<int16>>(hip, "<int16>", 1e-2);
    return wrong;
}
