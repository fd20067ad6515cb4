// The solver part of the reference's examples/multigrid-preconditioned-solver with multigrid::FixedCoarsening in place
// of Pgm: Cg preconditioned by one V-cycle of a three-level hierarchy (every second row, twice) on the 5-point Poisson
// matrix of a g x g grid.  The smoother is the reference's default -- Ir over scalar Jacobi, one sweep, relaxation 0.9,
// built by build_smoother -- and runs as the fused sweep of the library; the coarsest level is solved by Cg.
// Injection coarsening is a weak hierarchy: the example shows the classes, not a fast solver.
//
//   multigrid_preconditioned_solver [g = 64]
#include <ginkgo/ginkgo.hpp>

#include <cstdio>
#include <cstdlib>
#include <vector>

using csr = gko::matrix::Csr<double, gko::int32>;
using dense = gko::matrix::Dense<double>;
using cg = gko::solver::Cg<double>;
using ir = gko::solver::Ir<double>;
using mg = gko::solver::Multigrid;
using jacobi = gko::preconditioner::Jacobi<double, gko::int32>;
using coarsening = gko::multigrid::FixedCoarsening<double, gko::int32>;

// an mg_level entry: FixedCoarsening on every second row of the matrix it is handed
struct every_second_row : gko::LinOpFactory {
    explicit every_second_row(std::shared_ptr<const gko::Executor> exec) : gko::LinOpFactory(std::move(exec)) {}
    std::unique_ptr<gko::LinOp> generate_impl(std::shared_ptr<const gko::LinOp> m) const override
    {
        const gko::size_type rows = (m->get_size()[0] + 1) / 2;
        gko::array<gko::int32> coarse(exec_->get_master(), rows);
        for (gko::size_type i = 0; i < rows; ++i) coarse.get_data()[i] = static_cast<gko::int32>(2 * i);
        return coarsening::build().with_coarse_rows(coarse).on(exec_)->generate(m);
    }
};

int main(int argc, char** argv)
{
    const int g = argc > 1 ? std::atoi(argv[1]) : 64;
    auto exec = gko::HipExecutor::create(0, gko::ReferenceExecutor::create());
    gko::matrix_data<double, gko::int32> data(gko::dim<2>(g * g, g * g));
    for (int i = 0; i < g; ++i) {
        for (int j = 0; j < g; ++j) {
            const int row = i * g + j;
            if (i > 0) data.nonzeros.emplace_back(row, row - g, -1.0);
            if (j > 0) data.nonzeros.emplace_back(row, row - 1, -1.0);
            data.nonzeros.emplace_back(row, row, 4.0);
            if (j + 1 < g) data.nonzeros.emplace_back(row, row + 1, -1.0);
            if (i + 1 < g) data.nonzeros.emplace_back(row, row + g, -1.0);
        }
    }
    auto A = gko::share(csr::create(exec));
    A->read(data);
    const gko::size_type n = g * g;
    auto b = dense::create(exec, gko::dim<2>(n, 1)), x = dense::create(exec, gko::dim<2>(n, 1));
    b->fill(1.0);
    x->fill(0.0);

    auto smoother = gko::share(gko::solver::build_smoother<double>(
        std::shared_ptr<const gko::LinOpFactory>(jacobi::build().with_max_block_size(1u).on(exec)), 1u, 0.9));
    auto coarsest = gko::share(cg::build().with_criteria(gko::stop::Iteration::build().with_max_iters(50u).on(exec),
                                                         gko::stop::ResidualNorm<double>::build().with_reduction_factor(1e-8).on(exec)).on(exec));
    auto multigrid = gko::share(mg::build()
                                    .with_mg_level(gko::share(std::make_shared<every_second_row>(exec)))
                                    .with_pre_smoother(smoother)
                                    .with_post_uses_pre(true)
                                    .with_max_levels(2u)
                                    .with_coarsest_solver(coarsest)
                                    .with_cycle(gko::solver::multigrid::cycle::v)
                                    .with_default_initial_guess(gko::solver::initial_guess_mode::zero)
                                    .with_criteria(gko::stop::Iteration::build().with_max_iters(1u).on(exec))
                                    .on(exec));
    auto solver = cg::build()
                      .with_preconditioner(multigrid)
                      .with_criteria(gko::stop::Iteration::build().with_max_iters(2000u).on(exec),
                                     gko::stop::ResidualNorm<double>::build().with_reduction_factor(1e-8).on(exec))
                      .on(exec)
                      ->generate(A);
    solver->apply(b.get(), x.get());

    auto one = gko::initialize<dense>({1.0}, exec), neg_one = gko::initialize<dense>({-1.0}, exec);
    auto r = b->clone();
    A->apply(neg_one.get(), x.get(), one.get(), r.get());
    auto res = dense::create(exec, gko::dim<2>(1, 1)), rhs = dense::create(exec, gko::dim<2>(1, 1));
    r->compute_norm2(res.get());
    b->compute_norm2(rhs.get());
    auto levels = gko::as<const mg>(solver->get_preconditioner().get())->get_mg_level_list();
    std::printf("levels:");
    for (const auto& lvl : levels) std::printf(" %zu -> %zu", static_cast<size_t>(lvl->get_fine_op()->get_size()[0]), static_cast<size_t>(lvl->get_coarse_op()->get_size()[0]));
    std::printf("\niterations: %lld converged: %s\nrelative residual: %.3e\n", static_cast<long long>(solver->get_last_iteration_count()),
                solver->has_converged() ? "yes" : "no", res->clone(exec->get_master())->at(0) / rhs->clone(exec->get_master())->at(0));
    return solver->has_converged() ? 0 : 1;
}
