// ISAI through the host mirror: solver::Gmres(30) on a MatrixMarket matrix with preconditioner::Ilu (the exact
// ILU(0)) whose two triangular solves are replaced by LowerIsai and UpperIsai, i.e. by two CSR SpMVs per apply,
// against the same preconditioner with its triangular solves and against no preconditioner.
//   isai_preconditioned_solver <matrix.mtx> [sparsity_power = 1]
// Prints one "check <what>: ok|FAILED" line per check and
//   isai_preconditioned_solver: rows=<n> nnz=<n> power=<p> l_inv_nnz=<n> u_inv_nnz=<n> isai_iterations=<n>
//   trs_iterations=<n> plain_iterations=<n>
#include <ginkgo/ginkgo.hpp>

#include <cmath>
#include <cstdlib>
#include <fstream>
#include <iostream>

using dense = gko::matrix::Dense<double>;
using csr = gko::matrix::Csr<double, gko::int32>;
using ilu = gko::preconditioner::Ilu<double, gko::int32>;
using lower_isai = gko::preconditioner::LowerIsai<double, gko::int32>;
using upper_isai = gko::preconditioner::UpperIsai<double, gko::int32>;

static bool check(const char* what, bool ok)
{
    std::cout << "check " << what << ": " << (ok ? "ok" : "FAILED") << std::endl;
    return ok;
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::cerr << "usage: isai_preconditioned_solver <matrix.mtx> [sparsity_power]" << std::endl;
        return 2;
    }
    try {
        const int power = argc > 2 ? std::atoi(argv[2]) : 1;
        auto exec = gko::HipExecutor::create(0, gko::ReferenceExecutor::create());
        auto A = gko::share(gko::read<csr>(std::ifstream(argv[1]), exec));
        const gko::size_type n = A->get_size()[0];
        auto hb = dense::create(exec->get_master(), gko::dim<2>(n, 1));
        double bb = 0.0;
        for (gko::size_type i = 0; i < n; ++i) {
            hb->at(i, 0) = std::cos(0.3 * static_cast<double>(i));
            bb += hb->at(i, 0) * hb->at(i, 0);
        }
        const double bnorm = std::sqrt(bb);
        auto b = hb->clone(exec);
        auto x = dense::create(exec, gko::dim<2>(n, 1));
        auto one = gko::initialize<dense>({1.0}, exec), minus = gko::initialize<dense>({-1.0}, exec);

        auto solve = [&](std::shared_ptr<const gko::LinOp> precond, double* relres) {
            auto f = gko::solver::Gmres<double>::build();
            f.with_krylov_dim(30u).with_criteria(gko::stop::Iteration::build().with_max_iters(5000u).on(exec),
                                                 gko::stop::ResidualNorm<double>::build().with_reduction_factor(1e-10).on(exec));
            if (precond) f.with_generated_preconditioner(precond);
            auto s = f.on(exec)->generate(A);
            x->fill(0.0);
            s->apply(gko::lend(b), gko::lend(x));
            auto r = b->clone();
            A->apply(gko::lend(minus), gko::lend(x), gko::lend(one), gko::lend(r));
            auto rnorm = gko::initialize<dense>({0.0}, exec);
            r->compute_norm2(rnorm.get());
            *relres = rnorm->clone(exec->get_master())->at(0, 0) / bnorm;
            return static_cast<long>(s->get_last_iteration_count());
        };

        auto exact = gko::factorization::Ilu<double, gko::int32>::build().on(exec);
        auto with_isai = gko::share(ilu::build()
                                        .with_factorization_factory(exact)
                                        .with_l_solver_factory(lower_isai::build().with_sparsity_power(power).on(exec))
                                        .with_u_solver_factory(upper_isai::build().with_sparsity_power(power).on(exec))
                                        .on(exec)
                                        ->generate(A));
        auto with_trs = gko::share(ilu::build().with_factorization_factory(exact).on(exec)->generate(A));
        auto l_inv = dynamic_cast<const lower_isai*>(with_isai->get_l_solver().get());
        auto u_inv = dynamic_cast<const upper_isai*>(with_isai->get_u_solver().get());
        bool ok = check("solvers_are_isai", l_inv != nullptr && u_inv != nullptr);
        if (!ok) return 1;

        double res_isai = 0.0, res_trs = 0.0, res_plain = 0.0;
        const long it_isai = solve(with_isai, &res_isai);
        const long it_trs = solve(with_trs, &res_trs);
        const long it_plain = solve(nullptr, &res_plain);
        ok &= check("isai_converged", it_isai > 0 && it_isai < 5000 && res_isai <= 2e-9);
        ok &= check("trs_converged", it_trs > 0 && it_trs < 5000 && res_trs <= 2e-9);
        ok &= check("isai_saves_iterations", it_isai < it_plain);

        std::cout << "isai_preconditioned_solver: rows=" << n << " nnz=" << A->get_num_stored_elements() << " power=" << power
                  << " l_inv_nnz=" << l_inv->get_approximate_inverse()->get_num_stored_elements()
                  << " u_inv_nnz=" << u_inv->get_approximate_inverse()->get_num_stored_elements() << " isai_iterations=" << it_isai
                  << " trs_iterations=" << it_trs << " plain_iterations=" << it_plain << std::endl;
        return ok ? 0 : 1;
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
