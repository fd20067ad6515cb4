// gko::solver::Idr<double> of the host mirror: its factory parameters on the host (no device needed), and with
// "solve" as argument one solve on the device with a subspace seeded from std::random_device.
//   idr_mirror         -> "idr factory ok"
//   idr_mirror solve   -> "iterations: <n>\nrelative residual: <r>"
#include <ginkgo/ginkgo.hpp>

#include <cmath>
#include <iostream>
#include <string>

int main(int argc, char** argv)
{
    using idr = gko::solver::Idr<double>;
    using dense = gko::matrix::Dense<double>;
    using csr = gko::matrix::Csr<double, int>;
    try {
        bool thrown = false;
        try {
            idr::build().with_complex_subspace(true);
        } catch (const gko::NotSupported&) {
            thrown = true;
        }
        idr::build().with_complex_subspace(false);
        auto host = gko::ReferenceExecutor::create();
        gko::matrix_data<double, int> data;
        const gko::size_type n = 500;
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
        auto solver = idr::build()
                          .with_subspace_dim(3u)
                          .with_kappa(0.6)
                          .with_deterministic(false)
                          .with_criteria(gko::stop::Iteration::build().with_max_iters(300u).on(exec),
                                         gko::stop::ResidualNorm<double>::build().with_reduction_factor(1e-10).on(exec))
                          .on(exec)
                          ->generate(A);
        const bool getters = solver->get_subspace_dim() == 3 && solver->get_kappa() == 0.6 && !solver->get_deterministic() &&
                             !solver->get_complex_subspace() && idr::build().on(exec)->generate(A)->get_subspace_dim() == 2;
        if (!solve) {
            std::cout << (thrown && getters ? "idr factory ok" : "idr factory WRONG") << std::endl;
            return thrown && getters ? 0 : 1;
        }
        auto b = dense::create(exec, gko::dim<2>(n, 1)), x = dense::create(exec, gko::dim<2>(n, 1));
        b->fill(1.0);
        x->fill(0.0);
        solver->apply(gko::lend(b), gko::lend(x));
        auto r = b->clone();
        auto plus = gko::initialize<dense>({1.0}, exec), minus = gko::initialize<dense>({-1.0}, exec);
        A->apply(gko::lend(minus), gko::lend(x), gko::lend(plus), gko::lend(r));
        auto norm = gko::initialize<dense>({0.0}, exec);
        r->compute_norm2(gko::lend(norm));
        std::cout << "iterations: " << solver->get_last_iteration_count() << "\nconverged: " << (solver->has_converged() ? "yes" : "no")
                  << "\nrelative residual: " << exec->copy_val_to_host(norm->get_const_values()) / std::sqrt(double(n)) << std::endl;
        return 0;
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
