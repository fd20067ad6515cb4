// Records what the reference executor computes for solver::CbGmres and for its four kernels: the source of
// tests/golden/cb_gmres_ref.json (tests/test_cb_gmres_reference.py turns the output into that fixture and, where the
// reference's objects are present, runs this program again and compares).  Our own program over the reference's public
// API and core/solver/cb_gmres_kernels.hpp, like tools/isai_ref_record.cpp; it is built against the objects that
// oracle/ref.mk leaves in oracle/_ref/obj, with that file's flags:
//
//   g++ -std=c++14 -O1 -fPIC -ffp-contract=off -pthread -w -Ioracle/_ref/include -I$GINKGO_REF/include
//       -I$GINKGO_REF tools/cb_gmres_ref_record.cpp $(find oracle/_ref/obj -name '*.o') -o cb_gmres_ref_record -lm
//
// Input (stdin), any number of times, numbers as decimal integers or hexadecimal floats:
//   solve <name> <storage 0..5> <krylov_dim> <max_iters> <reduction> <baseline 0 rhs_norm | 1 initial_resnorm>
//         <jacobi max_block_size, 0: no preconditioner> <n> <nrhs> <nnz>, then n + 1 row pointers, nnz column indices,
//         nnz values and the n x nrhs right-hand side (row-major); x starts at 0
//   kernels <name> <storage> <krylov_dim> <steps> <stop_col> <stop_step> <n> <nrhs> <nnz>, then the same arrays:
//         initialize, restart, `steps` times { next = A next; arnoldi } with column stop_col stopped before step
//         stop_step (-1: never), then solve_krylov
// Output (stdout): one line per array, "<name> <what> <count> <items...>", doubles as hexadecimal floats, the Krylov
// basis as the raw stored integers.
#include <ginkgo/ginkgo.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "core/solver/cb_gmres_accessor.hpp"
#include "core/solver/cb_gmres_kernels.hpp"

using csr = gko::matrix::Csr<double, gko::int32>;
using dense = gko::matrix::Dense<double>;
namespace kernels = gko::kernels::reference::cb_gmres;
using gko::solver::cb_gmres::storage_precision;

static void put_vals(const std::string& tag, const std::string& what, const double* p, size_t count)
{
    std::printf("%s %s %zu", tag.c_str(), what.c_str(), count);
    for (size_t i = 0; i < count; ++i) std::printf(" %a", p[i]);
    std::printf("\n");
}

static void put_dense(const std::string& tag, const std::string& what, const dense* m)
{
    std::vector<double> v;
    for (size_t i = 0; i < m->get_size()[0]; ++i) {
        for (size_t j = 0; j < m->get_size()[1]; ++j) v.push_back(m->at(i, j));
    }
    put_vals(tag, what, v.data(), v.size());
}

template <class T>
static void put_ints(const std::string& tag, const std::string& what, const T* p, size_t count)
{
    std::printf("%s %s %zu", tag.c_str(), what.c_str(), count);
    for (size_t i = 0; i < count; ++i) std::printf(" %lld", static_cast<long long>(p[i]));
    std::printf("\n");
}

template <class Raw, class Stored>
static void put_raw(const std::string& tag, const std::string& what, const Stored* p, size_t count)
{
    static_assert(sizeof(Raw) == sizeof(Stored), "the raw view has the storage's width");
    std::vector<Raw> raw(count);
    std::memcpy(raw.data(), p, count * sizeof(Raw));
    put_ints(tag, what, raw.data(), count);
}

static double number(std::istream& in)
{
    std::string word;
    in >> word;
    return std::strtod(word.c_str(), nullptr);
}

struct iteration_logger : gko::log::Logger {
    mutable long last = -1;
    mutable std::vector<double> tau;
    void on_iteration_complete(const gko::LinOp*, const gko::size_type& it, const gko::LinOp*, const gko::LinOp*,
                               const gko::LinOp* t) const override
    {
        last = static_cast<long>(it);
        if (t != nullptr) {
            auto d = gko::as<dense>(t);
            tau.assign(d->get_const_values(), d->get_const_values() + d->get_size()[1]);
        }
    }
    iteration_logger() : gko::log::Logger(gko::log::Logger::iteration_complete_mask) {}
};

struct problem {
    long n = 0, nrhs = 0, nnz = 0;
    std::shared_ptr<csr> a;
    std::shared_ptr<dense> b;
};

static problem read_problem(std::shared_ptr<const gko::Executor> ref, long n, long nrhs, long nnz)
{
    problem p;
    p.n = n, p.nrhs = nrhs, p.nnz = nnz;
    gko::array<gko::int32> rp(ref, n + 1), ci(ref, nnz);
    gko::array<double> v(ref, nnz);
    for (long i = 0; i <= n; ++i) std::cin >> rp.get_data()[i];
    for (long i = 0; i < nnz; ++i) std::cin >> ci.get_data()[i];
    for (long i = 0; i < nnz; ++i) v.get_data()[i] = number(std::cin);
    p.a = gko::share(csr::create(ref, gko::dim<2>(n, n), std::move(v), std::move(ci), std::move(rp)));
    p.b = gko::share(dense::create(ref, gko::dim<2>(n, nrhs)));
    for (long i = 0; i < n; ++i) {
        for (long j = 0; j < nrhs; ++j) p.b->at(i, j) = number(std::cin);
    }
    return p;
}

// the scalars of an integer basis, (krylov_dim + 1) x nrhs; nothing for the floating storages
template <class Range>
static void put_scalars(const std::string& name, const std::string& what, Range range, size_t count, std::true_type)
{
    put_vals(name, what, range.get_accessor().get_const_scalar(), count);
}

template <class Range>
static void put_scalars(const std::string&, const std::string&, Range, size_t, std::false_type)
{}

template <class Storage, class Raw>
static void run_kernels(std::shared_ptr<const gko::ReferenceExecutor> ref, const std::string& name, const problem& p,
                        long krylov_dim, long steps, long stop_col, long stop_step)
{
    using helper = gko::cb_gmres::Range3dHelper<double, Storage>;
    const gko::size_type n = p.n, nrhs = p.nrhs, kd = krylov_dim;
    helper h(ref, gko::dim<3>{kd + 1, n, nrhs});
    auto range = h.get_range();
    auto residual = dense::create(ref, gko::dim<2>{n, nrhs});
    auto next = dense::create(ref, gko::dim<2>{n, nrhs});
    auto pv = dense::create(ref, gko::dim<2>{n, nrhs});
    auto hessenberg = dense::create(ref, gko::dim<2>{kd + 1, kd * nrhs});
    auto buffer = dense::create(ref, gko::dim<2>{kd + 1, nrhs});
    auto gsin = dense::create(ref, gko::dim<2>{kd, nrhs});
    auto gcos = dense::create(ref, gko::dim<2>{kd, nrhs});
    auto rnc = dense::create(ref, gko::dim<2>{kd + 1, nrhs});
    auto residual_norm = dense::create(ref, gko::dim<2>{1, nrhs});
    auto arnoldi_norm = dense::create(ref, gko::dim<2>{3, nrhs});
    auto y = dense::create(ref, gko::dim<2>{kd, nrhs});
    auto before = dense::create(ref, gko::dim<2>{n, nrhs});
    hessenberg->fill(0.0);
    buffer->fill(0.0);
    arnoldi_norm->fill(0.0);
    y->fill(0.0);
    gko::array<gko::size_type> final_iter_nums(ref, nrhs), num_reorth(ref, 1);
    gko::array<gko::stopping_status> stop_status(ref, nrhs), reorth_status(ref, nrhs);
    gko::array<char> tmp(ref);

    kernels::initialize(ref, p.b.get(), residual.get(), gsin.get(), gcos.get(), &stop_status, kd);
    put_dense(name, "initialize/residual", residual.get());
    kernels::restart(ref, residual.get(), residual_norm.get(), rnc.get(), arnoldi_norm.get(), range, next.get(),
                     &final_iter_nums, tmp, kd);
    put_dense(name, "restart/residual_norm", residual_norm.get());
    put_dense(name, "restart/residual_norm_collection", rnc.get());
    put_dense(name, "restart/next", next.get());
    put_raw<Raw>(name, "restart/basis", h.get_bases().get_const_data(), (kd + 1) * n * nrhs);
    for (long s = 0; s < steps; ++s) {
        if (s == stop_step) stop_status.get_data()[stop_col].stop(1);
        pv->copy_from(next.get());
        p.a->apply(pv.get(), next.get());
        auto hessenberg_iter =
            hessenberg->create_submatrix(gko::span{0, s + 2}, gko::span{nrhs * s, nrhs * (s + 1)});
        auto buffer_iter = buffer->create_submatrix(gko::span{0, s + 2}, gko::span{0, nrhs});
        kernels::arnoldi(ref, next.get(), gsin.get(), gcos.get(), residual_norm.get(), rnc.get(), range,
                         hessenberg_iter.get(), buffer_iter.get(), arnoldi_norm.get(), s, &final_iter_nums,
                         &stop_status, &reorth_status, &num_reorth);
        const std::string at = "arnoldi/" + std::to_string(s) + "/";
        put_dense(name, at + "next", next.get());
        put_dense(name, at + "hessenberg_iter", hessenberg_iter.get());
        put_dense(name, at + "arnoldi_norm", arnoldi_norm.get());
        put_dense(name, at + "residual_norm", residual_norm.get());
        put_dense(name, at + "residual_norm_collection", rnc.get());
        put_ints(name, at + "final_iter_nums", final_iter_nums.get_const_data(), nrhs);
    }
    put_dense(name, "givens_sin", gsin.get());
    put_dense(name, "givens_cos", gcos.get());
    auto hessenberg_view = hessenberg->create_submatrix(gko::span{0, steps}, gko::span{0, nrhs * steps});
    kernels::solve_krylov(ref, rnc.get(), range.get_accessor().to_const(), hessenberg_view.get(), y.get(),
                          before.get(), &final_iter_nums);
    put_dense(name, "solve_krylov/y", y.get());
    put_dense(name, "solve_krylov/before_preconditioner", before.get());
    put_raw<Raw>(name, "basis", h.get_bases().get_const_data(), (kd + 1) * n * nrhs);
    put_scalars(name, "scalars", range, (kd + 1) * nrhs,
                gko::cb_gmres::detail::has_3d_scaled_accessor<decltype(range)>{});
}

int main()
{
    auto ref = gko::ReferenceExecutor::create();
    std::string word, name;
    while (std::cin >> word) {
        long storage = 0, krylov_dim = 0, n = 0, nrhs = 0, nnz = 0;
        if (word == "solve") {
            long max_iters = 0, baseline = 0, jacobi = 0;
            std::cin >> name >> storage >> krylov_dim >> max_iters;
            const double reduction = number(std::cin);
            std::cin >> baseline >> jacobi >> n >> nrhs >> nnz;
            const problem p = read_problem(ref, n, nrhs, nnz);
            if (!std::cin) return 3;
            auto builder = gko::solver::CbGmres<double>::build()
                               .with_krylov_dim(static_cast<gko::size_type>(krylov_dim))
                               .with_storage_precision(static_cast<storage_precision>(storage))
                               .with_criteria(gko::stop::Iteration::build()
                                                  .with_max_iters(static_cast<gko::size_type>(max_iters))
                                                  .on(ref),
                                              gko::stop::ResidualNorm<double>::build()
                                                  .with_baseline(baseline == 0 ? gko::stop::mode::rhs_norm
                                                                               : gko::stop::mode::initial_resnorm)
                                                  .with_reduction_factor(reduction)
                                                  .on(ref));
            std::shared_ptr<gko::LinOp> solver;
            if (jacobi > 0) {
                solver = builder
                             .with_preconditioner(gko::preconditioner::Jacobi<double, gko::int32>::build()
                                                      .with_max_block_size(static_cast<gko::uint32>(jacobi))
                                                      .on(ref))
                             .on(ref)
                             ->generate(p.a);
            } else {
                solver = builder.on(ref)->generate(p.a);
            }
            auto logger = std::make_shared<iteration_logger>();
            solver->add_logger(logger);
            auto x = dense::create(ref, gko::dim<2>(n, nrhs));
            x->fill(0.0);
            solver->apply(p.b.get(), x.get());
            put_dense(name, "x", x.get());
            const long long its[1] = {logger->last};
            put_ints(name, "iterations", its, 1);
            put_vals(name, "residual_norm", logger->tau.data(), logger->tau.size());
        } else if (word == "kernels") {
            long steps = 0, stop_col = 0, stop_step = -1;
            std::cin >> name >> storage >> krylov_dim >> steps >> stop_col >> stop_step >> n >> nrhs >> nnz;
            const problem p = read_problem(ref, n, nrhs, nnz);
            if (!std::cin) return 3;
            switch (storage) {
            case 0: run_kernels<double, gko::int64>(ref, name, p, krylov_dim, steps, stop_col, stop_step); break;
            case 1: run_kernels<float, gko::int32>(ref, name, p, krylov_dim, steps, stop_col, stop_step); break;
            case 2: run_kernels<gko::half, gko::int16>(ref, name, p, krylov_dim, steps, stop_col, stop_step); break;
            case 3: run_kernels<gko::int64, gko::int64>(ref, name, p, krylov_dim, steps, stop_col, stop_step); break;
            case 4: run_kernels<gko::int32, gko::int32>(ref, name, p, krylov_dim, steps, stop_col, stop_step); break;
            case 5: run_kernels<gko::int16, gko::int16>(ref, name, p, krylov_dim, steps, stop_col, stop_step); break;
            default: return 4;
            }
        } else {
            return 2;
        }
    }
    return 0;
}
