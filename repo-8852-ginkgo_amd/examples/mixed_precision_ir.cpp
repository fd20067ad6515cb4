// mixed_precision_ir: mixed-precision iterative refinement through the gko:: host mirror over libgkomi.so.  The
// outer residual and the solution stay in double; each correction comes from a Cg<float>.
//
//   mixed_precision_ir [executor] [outer reduction] [inner reduction]
//
// reads data/A.mtx, b = A * 1 (so x = 1 solves the system), x0 = 0, and solves A x = b two ways:
//   loop : the hand-written refinement -- r = b - A x, convert r to float, Cg<float> with (float) r as its initial
//          guess, convert the correction back, x += d -- on Csr<float> / Dense<float> converted on the device;
//   ir   : solver::Ir<double> with the generated Cg<float> as its inner solver, which the mirror runs as one native
//          driver.
// Prints for each the outer and inner iterations and the TRUE double residual ||b - A x|| / ||b||; exit code 0 only if
// both reach the outer goal, 3 on a host executor (gko::NotCompiled).
#include <ginkgo/ginkgo.hpp>

#include <cmath>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>

namespace {

using vec = gko::matrix::Dense<double>;
using solver_vec = gko::matrix::Dense<float>;
using mtx = gko::matrix::Csr<double, int>;
using solver_mtx = gko::matrix::Csr<float, int>;
using cg = gko::solver::Cg<float>;
using ir = gko::solver::Ir<double>;

constexpr gko::size_type max_outer_iters = 100;
constexpr gko::size_type max_inner_iters = 500;

double norm(const vec* v)
{
    auto res = gko::initialize<vec>({0.0}, v->get_executor());
    v->compute_norm2(res.get());
    return v->get_executor()->copy_val_to_host(res->get_const_values());
}

// ||b - A x|| / ||b|| in double
double true_rel_residual(const mtx* A, const vec* b, const vec* x)
{
    auto exec = b->get_executor();
    auto one = gko::initialize<vec>({1.0}, exec);
    auto neg_one = gko::initialize<vec>({-1.0}, exec);
    auto r = b->clone();
    A->apply(neg_one.get(), x, one.get(), r.get());
    return norm(r.get()) / norm(b);
}

}  // namespace

int main(int argc, char* argv[])
{
    const std::string executor = argc >= 2 ? argv[1] : "hip";
    const double outer_reduction = argc >= 3 ? std::strtod(argv[2], nullptr) : 1e-12;
    const float inner_reduction = argc >= 4 ? static_cast<float>(std::strtod(argv[3], nullptr)) : 1e-2f;
    try {
        std::shared_ptr<gko::Executor> exec;
        if (executor == "hip") {
            exec = gko::HipExecutor::create(0, gko::OmpExecutor::create(), true);
        } else if (executor == "reference") {
            exec = gko::ReferenceExecutor::create();
        } else {
            std::cerr << "unknown executor " << executor << "\n";
            return 2;
        }
        std::ifstream in("data/A.mtx");
        if (!in) {
            std::cerr << "data/A.mtx not found\n";
            return 2;
        }
        auto A = gko::share(gko::read<mtx>(in, exec));
        const auto n = A->get_size()[0];
        auto host_ones = vec::create(exec->get_master(), gko::dim<2>(n, 1));
        for (gko::size_type i = 0; i < n; ++i) host_ones->at(i, 0) = 1.0;
        auto ones = gko::clone(exec, host_ones);
        auto b = vec::create(exec, gko::dim<2>(n, 1));
        A->apply(ones.get(), b.get());
        auto one = gko::initialize<vec>({1.0}, exec);
        auto neg_one = gko::initialize<vec>({-1.0}, exec);

        auto A_float = gko::share(solver_mtx::create(exec));
        A->convert_to(A_float.get());
        auto inner_factory = cg::build()
                                 .with_criteria(gko::stop::ResidualNorm<float>::build().with_reduction_factor(inner_reduction).on(exec),
                                                gko::stop::Iteration::build().with_max_iters(max_inner_iters).on(exec))
                                 .on(exec);
        auto inner_solver = gko::share(inner_factory->generate(A_float));

        // 1. the hand-written loop (ir.cpp:188-277 spelled out)
        auto x = vec::create(exec, gko::dim<2>(n, 1));
        x->fill(0.0);
        auto residual = b->clone();
        auto inner_residual = solver_vec::create(exec);
        auto inner_solution = solver_vec::create(exec);
        auto delta = vec::create(exec);
        const double goal = outer_reduction * norm(b.get());
        long long loop_iters = -1, loop_inner = 0;
        while (true) {
            ++loop_iters;
            if (loop_iters >= static_cast<long long>(max_outer_iters) || norm(residual.get()) < goal) break;
            residual->convert_to(inner_residual.get());
            inner_solution->copy_from(inner_residual.get());
            inner_solver->apply(inner_residual.get(), inner_solution.get());
            loop_inner += inner_solver->get_last_iteration_count();
            inner_solution->convert_to(delta.get());
            x->add_scaled(one.get(), delta.get());
            residual->copy_from(b.get());
            A->apply(neg_one.get(), x.get(), one.get(), residual.get());
        }
        const double loop_res = true_rel_residual(A.get(), b.get(), x.get());
        std::cout << "loop: outer iterations " << loop_iters << ", inner iterations " << loop_inner << ", true residual "
                  << loop_res << "\n";

        // 2. Ir<double> over the generated Cg<float>
        auto solver = ir::build()
                          .with_criteria(gko::stop::ResidualNorm<double>::build().with_reduction_factor(outer_reduction).on(exec),
                                         gko::stop::Iteration::build().with_max_iters(max_outer_iters).on(exec))
                          .with_generated_solver(inner_solver)
                          .on(exec)
                          ->generate(A);
        auto x2 = vec::create(exec, gko::dim<2>(n, 1));
        x2->fill(0.0);
        solver->apply(b.get(), x2.get());
        const double ir_res = true_rel_residual(A.get(), b.get(), x2.get());
        std::cout << "ir: outer iterations " << solver->get_last_iteration_count() << ", inner iterations "
                  << solver->get_last_inner_iteration_count() << ", true residual " << ir_res << "\n";
        const bool ok = loop_res <= outer_reduction && ir_res <= outer_reduction && solver->has_converged();
        std::cout << (ok ? "both reached the goal" : "goal NOT reached") << "\n";
        return ok ? 0 : 1;
    } catch (const gko::NotCompiled& e) {
        std::cerr << "NotCompiled: " << e.what() << "\n";
        return 3;
    } catch (const std::exception& e) {
        std::cerr << e.what() << "\n";
        return 2;
    }
}
