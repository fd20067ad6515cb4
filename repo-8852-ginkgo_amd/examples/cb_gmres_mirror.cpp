// gko::solver::CbGmres<double> of the host mirror: its factory parameters on the host (no device needed), and with
// "solve" as argument one solve per storage precision on the device.
//   cb_gmres_mirror         -> "cb_gmres factory ok"
//   cb_gmres_mirror solve   -> per storage "<name>: iterations <n> converged <yes|no> forced resets <k> relative residual <r>"
#include <ginkgo/ginkgo.hpp>

#include <cmath>
#include <iostream>
#include <string>

int main(int argc, char** argv)
{
    using cb = gko::solver::CbGmres<double>;
    using sp = gko::solver::cb_gmres::storage_precision;
    using dense = gko::matrix::Dense<double>;
    using csr = gko::matrix::Csr<double, int>;
    try {
        auto host = gko::ReferenceExecutor::create();
        gko::matrix_data<double, int> data;
        const gko::size_type n = 1000;
        data.size = {n, n};
        for (gko::size_type i = 0; i < n; ++i) {
            if (i > 0) data.nonzeros.emplace_back(i, i - 1, -1.5);
            data.nonzeros.emplace_back(i, i, 4.0);
            if (i + 1 < n) data.nonzeros.emplace_back(i, i + 1, -0.5);
        }
        const bool solve = argc > 1 && std::string(argv[1]) == "solve";
        std::shared_ptr<gko::Executor> exec = host;
        if (solve) exec = gko::HipExecutor::create(0, host);
        auto A = gko::share(csr::create(exec));
        A->read(data);
        auto defaults = cb::build().on(exec)->generate(A);
        auto set = cb::build().with_krylov_dim(7u).with_storage_precision(sp::ireduce2).on(exec)->generate(A);
        const bool getters = defaults->get_krylov_dim() == 100 && defaults->get_storage_precision() == sp::reduce1 &&
                             set->get_krylov_dim() == 7 && set->get_storage_precision() == sp::ireduce2 &&
                             static_cast<int>(sp::keep) == 0 && static_cast<int>(sp::ireduce2) == 5;
        if (!solve) {
            std::cout << (getters ? "cb_gmres factory ok" : "cb_gmres factory WRONG") << std::endl;
            return getters ? 0 : 1;
        }
        const char* names[] = {"keep", "reduce1", "reduce2", "integer", "ireduce1", "ireduce2"};
        auto plus = gko::initialize<dense>({1.0}, exec), minus = gko::initialize<dense>({-1.0}, exec);
        for (int s = 0; s < 6; ++s) {
            auto solver = cb::build()
                              .with_krylov_dim(20u)
                              .with_storage_precision(static_cast<sp>(s))
                              .with_criteria(gko::stop::Iteration::build().with_max_iters(500u).on(exec),
                                             gko::stop::ResidualNorm<double>::build().with_reduction_factor(1e-10).on(exec))
                              .on(exec)
                              ->generate(A);
            auto b = dense::create(exec, gko::dim<2>(n, 1)), x = dense::create(exec, gko::dim<2>(n, 1));
            b->fill(1.0);
            x->fill(0.0);
            solver->apply(gko::lend(b), gko::lend(x));
            auto r = b->clone();
            A->apply(gko::lend(minus), gko::lend(x), gko::lend(plus), gko::lend(r));
            auto norm = gko::initialize<dense>({0.0}, exec);
            r->compute_norm2(gko::lend(norm));
            std::cout << names[s] << ": iterations " << solver->get_last_iteration_count() << " converged "
                      << (solver->has_converged() ? "yes" : "no") << " forced resets " << solver->get_last_forced_resets()
                      << " relative residual " << exec->copy_val_to_host(norm->get_const_values()) / std::sqrt(double(n))
                      << std::endl;
        }
        return 0;
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
