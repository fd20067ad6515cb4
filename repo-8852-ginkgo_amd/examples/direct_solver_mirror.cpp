// The sparse direct solver through the host mirror: experimental::solver::Direct over experimental::factorization::Lu
// (symmetric sparsity: symbolic Cholesky) on a MatrixMarket file.  The right-hand side is A times a known vector.
// Usage: direct_solver_mirror <matrix.mtx> [num_rhs]
// Prints one "check <what>: ok|FAILED" line per check and
//   direct_solver_mirror: rows=<n> factor_nnz=<n> residual_norm=<r> rhs_norm=<r>
#include <ginkgo/ginkgo.hpp>

#include <cmath>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

using dense = gko::matrix::Dense<double>;
using csr = gko::matrix::Csr<double, gko::int32>;
using lu_type = gko::experimental::factorization::Lu<double, gko::int32>;
using factorization_type = gko::experimental::factorization::Factorization<double, gko::int32>;
using direct_type = gko::experimental::solver::Direct<double, gko::int32>;

static int failures = 0;

static void check(const char* what, bool ok)
{
    std::cout << "check " << what << ": " << (ok ? "ok" : "FAILED") << "\n";
    failures += ok ? 0 : 1;
}

// the largest column norm of a dense matrix
static double norm_of(std::shared_ptr<const gko::Executor> exec, const dense* m)
{
    auto norm = dense::create(exec, gko::dim<2>(1, m->get_size()[1]));
    m->compute_norm2(gko::lend(norm));
    auto host = dense::create(exec->get_master(), norm->get_size());
    host->copy_from(gko::lend(norm));
    double largest = 0.0;
    for (gko::size_type j = 0; j < m->get_size()[1]; ++j) largest = std::max(largest, host->at(0, j));
    return largest;
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::cerr << "usage: direct_solver_mirror <matrix.mtx> [num_rhs]\n";
        return 2;
    }
    try {
        const gko::size_type nrhs = argc > 2 ? std::stoul(argv[2]) : 1;
        auto exec = gko::HipExecutor::create(0, gko::ReferenceExecutor::create());
        std::ifstream file(argv[1]);
        if (!file.good()) throw std::runtime_error(std::string("cannot read ") + argv[1]);
        auto A = gko::share(gko::read<csr>(std::move(file), exec));
        const gko::size_type n = A->get_size()[0];
        // x_ref(i, j) = 1 + sin(0.37 i + j), b = A x_ref
        auto x_host = dense::create(exec->get_master(), gko::dim<2>(n, nrhs));
        for (gko::size_type i = 0; i < n; ++i) {
            for (gko::size_type j = 0; j < nrhs; ++j) x_host->at(i, j) = 1.0 + std::sin(0.37 * static_cast<double>(i) + static_cast<double>(j));
        }
        auto x_ref = dense::create(exec, x_host->get_size());
        x_ref->copy_from(gko::lend(x_host));
        auto b = dense::create(exec, x_ref->get_size());
        A->apply(gko::lend(x_ref), gko::lend(b));
        auto x = dense::create(exec, x_ref->get_size());
        x->fill(0.0);

        auto lu_factory = gko::share(lu_type::build().with_symmetric_sparsity(true).on(exec));
        auto solver = direct_type::build().with_factorization(lu_factory).with_num_rhs(nrhs).on(exec)->generate(A);
        solver->apply(gko::lend(b), gko::lend(x));
        auto factors = solver->get_system_matrix();
        check("the factorization is a combined L + U", factors->get_storage_type() == gko::experimental::factorization::storage_type::combined_lu);

        auto plus = gko::initialize<dense>({1.0}, exec), minus = gko::initialize<dense>({-1.0}, exec);
        auto r = b->clone();
        A->apply(gko::lend(minus), gko::lend(x), gko::lend(plus), gko::lend(r));
        const double rnorm = norm_of(exec, gko::lend(r)), bnorm = norm_of(exec, gko::lend(b));
        check("residual below 1e-10 of the right-hand side", rnorm <= 1e-10 * bnorm);

        // a Factorization as the system matrix is taken as it is; so is its unpacked composition
        auto x2 = dense::create(exec, x_ref->get_size());
        x2->fill(0.0);
        direct_type::build().with_num_rhs(nrhs).on(exec)->generate(factors)->apply(gko::lend(b), gko::lend(x2));
        auto x3 = dense::create(exec, x_ref->get_size());
        x3->fill(0.0);
        std::shared_ptr<const factorization_type> unpacked = factors->unpack();
        check("unpack gives a composition", unpacked->get_storage_type() == gko::experimental::factorization::storage_type::composition);
        direct_type::build().with_num_rhs(nrhs).on(exec)->generate(unpacked)->apply(gko::lend(b), gko::lend(x3));
        auto hx = dense::create(exec->get_master(), x->get_size()), hx2 = hx->clone(), hx3 = hx->clone();
        hx->copy_from(gko::lend(x));
        hx2->copy_from(gko::lend(x2));
        hx3->copy_from(gko::lend(x3));
        bool same = true;
        for (gko::size_type i = 0; i < n; ++i) {
            for (gko::size_type j = 0; j < nrhs; ++j) same = same && hx->at(i, j) == hx2->at(i, j) && hx->at(i, j) == hx3->at(i, j);
        }
        check("the same solution from the factorization handed over and from its composition", same);

        // x4 = 0.5 A^-1 b - 2 x4 against scale + add_scaled on the plain result
        auto alpha = gko::initialize<dense>({0.5}, exec), beta = gko::initialize<dense>({-2.0}, exec);
        auto x4 = x_ref->clone(), want = x_ref->clone();
        solver->apply(gko::lend(alpha), gko::lend(b), gko::lend(beta), gko::lend(x4));
        want->scale(gko::lend(beta));
        want->add_scaled(gko::lend(alpha), gko::lend(x));
        auto h4 = hx->clone(), hw = hx->clone();
        h4->copy_from(gko::lend(x4));
        hw->copy_from(gko::lend(want));
        same = true;
        for (gko::size_type i = 0; i < n; ++i) {
            for (gko::size_type j = 0; j < nrhs; ++j) same = same && h4->at(i, j) == hw->at(i, j);
        }
        check("advanced apply = scale + add_scaled of the plain result", same);

        bool thrown = false;
        try {
            solver->transpose();
        } catch (const gko::NotImplemented&) {
            thrown = true;
        }
        check("transpose is not implemented", thrown);
        thrown = false;
        try {
            lu_type::build().on(exec)->generate(A);
        } catch (const gko::NotSupported&) {
            thrown = true;
        }
        check("Lu without symbolic factorization and without symmetric sparsity is not supported", thrown);

        std::cout << "direct_solver_mirror: rows=" << n << " factor_nnz=" << factors->get_combined()->get_num_stored_elements() << " residual_norm=" << rnorm
                  << " rhs_norm=" << bnorm << "\n";
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
    return failures == 0 ? 0 : 1;
}
