// ParILUT through the host mirror: factorization::ParIlut of a 2-D 5-point matrix on a g x g grid with an upwind
// convection term, with its defaults (5 iterations, fill_in_limit 2.0, approximate selection), with the exact
// selection and with a fill-in budget below the pattern of A; then solver::Gmres with preconditioner::Ilu over the
// ParIlut factory against the same solver without a preconditioner.  The factors are deterministic (a level
// schedule reproduces the reference executor's sequential sweep), which the example checks by generating twice.
// Prints one "check <what>: ok|FAILED" line per check and
//   par_ilut_preconditioned_solver: rows=<n> a_nnz=<n> l_nnz=<n> u_nnz=<n> gmres_ilut_iterations=<n> gmres_plain_iterations=<n>
#include <ginkgo/ginkgo.hpp>

#include <cmath>
#include <cstring>
#include <iostream>
#include <vector>

using dense = gko::matrix::Dense<double>;
using csr = gko::matrix::Csr<double, gko::int32>;
using mdata = gko::matrix_data<double, gko::int32>;
using par_ilut = gko::factorization::ParIlut<double, gko::int32>;

struct host_csr {
    gko::size_type n;
    std::vector<int> rp, ci;
    std::vector<double> v;
};

static host_csr to_host(const csr* m)
{
    mdata d;
    m->write(d);
    host_csr h{m->get_size()[0], std::vector<int>(m->get_size()[0] + 1, 0), {}, {}};
    for (const auto& e : d.nonzeros) {
        h.rp[e.row + 1]++;
        h.ci.push_back(e.column);
        h.v.push_back(e.value);
    }
    for (gko::size_type r = 0; r < h.n; ++r) h.rp[r + 1] += h.rp[r];
    return h;
}

static bool same(const host_csr& x, const host_csr& y)
{
    return x.n == y.n && x.rp == y.rp && x.ci == y.ci && x.v.size() == y.v.size() &&
           (x.v.empty() || std::memcmp(x.v.data(), y.v.data(), sizeof(double) * x.v.size()) == 0);
}

// rows strictly ascending; lower: they end in a unit diagonal; upper: they start with their diagonal
static bool triangular(const host_csr& m, bool lower)
{
    for (int row = 0; row < static_cast<int>(m.n); ++row) {
        const int b = m.rp[row], e = m.rp[row + 1];
        if (e <= b) return false;
        for (int z = b + 1; z < e; ++z) {
            if (m.ci[z] <= m.ci[z - 1]) return false;
        }
        if (lower ? (m.ci[e - 1] != row || m.v[e - 1] != 1.0) : m.ci[b] != row) return false;
    }
    return true;
}

static bool check(const char* what, bool ok)
{
    std::cout << "check " << what << ": " << (ok ? "ok" : "FAILED") << std::endl;
    return ok;
}

static double residual(const host_csr& a, const dense* hx, double rhs)
{
    double rr = 0.0;
    for (int row = 0; row < static_cast<int>(a.n); ++row) {
        double r = rhs;
        for (int z = a.rp[row]; z < a.rp[row + 1]; ++z) r -= a.v[z] * hx->at(a.ci[z], 0);
        rr += r * r;
    }
    return std::sqrt(rr);
}

int main()
{
    try {
        auto exec = gko::HipExecutor::create(0, gko::ReferenceExecutor::create());
        const int g = 24;
        const gko::size_type n = static_cast<gko::size_type>(g) * g;
        mdata conv_data;
        conv_data.size = {n, n};
        for (int p = 0; p < g * g; ++p) {
            const int px = p % g, py = p / g;
            const int nb[5] = {py > 0 ? p - g : -1, px > 0 ? p - 1 : -1, p, px + 1 < g ? p + 1 : -1, py + 1 < g ? p + g : -1};
            for (int q : nb) {
                if (q < 0) continue;
                conv_data.nonzeros.emplace_back(p, q, q == p ? 4.5 : (q < p ? -1.5 : -1.0));
            }
        }
        auto C = gko::share(csr::create(exec));
        C->read(conv_data);
        const host_csr hc = to_host(C.get());
        const long a_nnz = static_cast<long>(hc.v.size());
        bool ok = true;

        auto fact = par_ilut::build().on(exec)->generate(C);
        const host_csr hl = to_host(fact->get_l_factor().get()), hu = to_host(fact->get_u_factor().get());
        ok &= check("factors_are_triangular", triangular(hl, true) && triangular(hu, false));
        // the entries of a triangle of A with its diagonal; the budget is fill_in_limit times that (the approximate
        // threshold, ties and diagonals below the threshold keep a few entries more)
        const long l0 = (a_nnz - static_cast<long>(n)) / 2 + static_cast<long>(n);
        ok &= check("factors_take_fill", static_cast<long>(hl.v.size()) > l0 && static_cast<long>(hu.v.size()) > l0);
        auto again = par_ilut::build().on(exec)->generate(C);
        ok &= check("generate_is_deterministic", same(to_host(again->get_l_factor().get()), hl) && same(to_host(again->get_u_factor().get()), hu));

        auto exact = par_ilut::build().with_approximate_select(false).with_fill_in_limit(1.2).with_iterations(3u).on(exec)->generate(C);
        ok &= check("exact_selection", triangular(to_host(exact->get_l_factor().get()), true) && triangular(to_host(exact->get_u_factor().get()), false));
        auto lean = par_ilut::build().with_fill_in_limit(0.75).on(exec)->generate(C);
        ok &= check("budget_below_the_pattern_of_a", static_cast<long>(lean->get_l_factor()->get_num_stored_elements()) < l0 &&
                                                      triangular(to_host(lean->get_l_factor().get()), true));

        bool refused = false;
        try {
            par_ilut::build().with_fill_in_limit(0.0).on(exec)->generate(C);
        } catch (const gko::ValueMismatch&) {
            refused = true;
        }
        ok &= check("fill_in_limit_zero_is_refused", refused);

        auto criteria = [&] {
            return std::make_pair(gko::stop::Iteration::build().with_max_iters(500u).on(exec),
                                  gko::stop::ResidualNorm<double>::build().with_reduction_factor(1e-10).on(exec));
        };
        auto b = dense::create(exec, gko::dim<2>(n, 1)), x = dense::create(exec, gko::dim<2>(n, 1));
        b->fill(1.0);
        const double bnorm = std::sqrt(static_cast<double>(n));

        x->fill(0.0);
        auto plain = gko::solver::Gmres<double>::build().with_criteria(criteria().first, criteria().second).with_krylov_dim(30u).on(exec)->generate(C);
        plain->apply(gko::lend(b), gko::lend(x));
        const long plain_iters = static_cast<long>(plain->get_last_iteration_count());

        x->fill(0.0);
        auto gmres = gko::solver::Gmres<double>::build()
                         .with_criteria(criteria().first, criteria().second)
                         .with_krylov_dim(30u)
                         .with_preconditioner(gko::preconditioner::Ilu<double, gko::int32>::build()
                                                  .with_factorization_factory(par_ilut::build().on(exec))
                                                  .on(exec))
                         .on(exec)
                         ->generate(C);
        gmres->apply(gko::lend(b), gko::lend(x));
        const long gmres_iters = static_cast<long>(gmres->get_last_iteration_count());
        ok &= check("gmres_ilut_converged", gmres_iters < plain_iters && residual(hc, x->clone(exec->get_master()).get(), 1.0) <= 1e-8 * bnorm);

        std::cout << "par_ilut_preconditioned_solver: rows=" << n << " a_nnz=" << a_nnz << " l_nnz=" << hl.v.size() << " u_nnz=" << hu.v.size()
                  << " gmres_ilut_iterations=" << gmres_iters << " gmres_plain_iterations=" << plain_iters << std::endl;
        return ok ? 0 : 1;
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
