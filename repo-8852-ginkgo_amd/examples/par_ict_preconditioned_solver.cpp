// ParICT through the host mirror: factorization::ParIct of the 2-D 5-point Laplacian on a 24 x 20 grid, with its
// defaults (5 iterations, fill_in_limit 2.0, approximate selection), with the exact selection and with a fill-in
// budget below the pattern of A; then solver::Cg with preconditioner::Ic over the ParIct factory against the same
// solver without a preconditioner.  The factor is deterministic (a level schedule reproduces the reference
// executor's sequential sweep), which the example checks by generating twice.
// Prints one "check <what>: ok|FAILED" line per check and
//   par_ict_preconditioned_solver: rows=<n> a_nnz=<n> l_nnz=<n> cg_ict_iterations=<n> cg_plain_iterations=<n>
#include <ginkgo/ginkgo.hpp>

#include <cmath>
#include <cstring>
#include <iostream>
#include <vector>

using dense = gko::matrix::Dense<double>;
using csr = gko::matrix::Csr<double, gko::int32>;
using mdata = gko::matrix_data<double, gko::int32>;
using par_ict = gko::factorization::ParIct<double, gko::int32>;

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

// rows strictly ascending and ending in a positive diagonal, every value finite
static bool lower_factor(const host_csr& m)
{
    for (int row = 0; row < static_cast<int>(m.n); ++row) {
        const int b = m.rp[row], e = m.rp[row + 1];
        if (e <= b) return false;
        for (int z = b + 1; z < e; ++z) {
            if (m.ci[z] <= m.ci[z - 1]) return false;
        }
        for (int z = b; z < e; ++z) {
            if (!std::isfinite(m.v[z])) return false;
        }
        if (m.ci[e - 1] != row || !(m.v[e - 1] > 0.0)) return false;
    }
    return true;
}

// y is the transpose of x, entry for entry
static bool transposed(const host_csr& x, const host_csr& y)
{
    if (x.n != y.n || x.v.size() != y.v.size()) return false;
    std::vector<int> at(y.rp.begin(), y.rp.end() - 1);
    for (int row = 0; row < static_cast<int>(x.n); ++row) {
        for (int z = x.rp[row]; z < x.rp[row + 1]; ++z) {
            const int q = at[x.ci[z]]++;
            if (q >= y.rp[x.ci[z] + 1] || y.ci[q] != row || std::memcmp(&y.v[q], &x.v[z], sizeof(double)) != 0) return false;
        }
    }
    return true;
}

static bool check(const char* what, bool ok)
{
    std::cout << "check " << what << ": " << (ok ? "ok" : "FAILED") << std::endl;
    return ok;
}

static double residual(const host_csr& a, const dense* hx, const dense* hb)
{
    double rr = 0.0;
    for (int row = 0; row < static_cast<int>(a.n); ++row) {
        double r = hb->at(row, 0);
        for (int z = a.rp[row]; z < a.rp[row + 1]; ++z) r -= a.v[z] * hx->at(a.ci[z], 0);
        rr += r * r;
    }
    return std::sqrt(rr);
}

int main()
{
    try {
        auto exec = gko::HipExecutor::create(0, gko::ReferenceExecutor::create());
        const int gx = 24, gy = 20;  // 20 rows of 24 points
        const gko::size_type n = static_cast<gko::size_type>(gx) * gy;
        mdata grid;
        grid.size = {n, n};
        for (int p = 0; p < gx * gy; ++p) {
            const int px = p % gx, py = p / gx;
            const int nb[5] = {py > 0 ? p - gx : -1, px > 0 ? p - 1 : -1, p, px + 1 < gx ? p + 1 : -1, py + 1 < gy ? p + gx : -1};
            for (int q : nb) {
                if (q < 0) continue;
                grid.nonzeros.emplace_back(p, q, q == p ? 4.0 : -1.0);
            }
        }
        auto A = gko::share(csr::create(exec));
        A->read(grid);
        const host_csr ha = to_host(A.get());
        const long a_nnz = static_cast<long>(ha.v.size());
        bool ok = true;

        auto fact = par_ict::build().on(exec)->generate(A);
        const host_csr hl = to_host(fact->get_l_factor().get()), hlt = to_host(fact->get_lt_factor().get());
        ok &= check("factor_is_lower_triangular", lower_factor(hl));
        ok &= check("lt_is_its_transpose", transposed(hl, hlt));
        // the entries of the lower triangle of A with its diagonal; the budget is fill_in_limit times that (the
        // approximate threshold, ties and diagonals below the threshold keep a few entries more)
        const long l0 = (a_nnz - static_cast<long>(n)) / 2 + static_cast<long>(n);
        ok &= check("factor_takes_fill", static_cast<long>(hl.v.size()) > l0);
        auto again = par_ict::build().on(exec)->generate(A);
        ok &= check("generate_is_deterministic", same(to_host(again->get_l_factor().get()), hl) && same(to_host(again->get_lt_factor().get()), hlt));

        auto exact = par_ict::build().with_approximate_select(false).with_fill_in_limit(1.2).with_iterations(3u).on(exec)->generate(A);
        ok &= check("exact_selection", lower_factor(to_host(exact->get_l_factor().get())));
        auto lean = par_ict::build().with_fill_in_limit(0.75).on(exec)->generate(A);
        ok &= check("budget_below_the_pattern_of_a", static_cast<long>(lean->get_l_factor()->get_num_stored_elements()) < l0 &&
                                                      lower_factor(to_host(lean->get_l_factor().get())));

        bool refused = false;
        try {
            par_ict::build().with_fill_in_limit(0.0).on(exec)->generate(A);
        } catch (const gko::ValueMismatch&) {
            refused = true;
        }
        ok &= check("fill_in_limit_zero_is_refused", refused);
        refused = false;
        try {
            auto wide = gko::share(csr::create(exec));
            mdata w;
            w.size = {2, 3};
            w.nonzeros.emplace_back(0, 0, 1.0);
            w.nonzeros.emplace_back(1, 2, 1.0);
            wide->read(w);
            par_ict::build().on(exec)->generate(wide);
        } catch (const gko::DimensionMismatch&) {
            refused = true;
        }
        ok &= check("non_square_is_refused", refused);

        auto criteria = [&] {
            return std::make_pair(gko::stop::Iteration::build().with_max_iters(500u).on(exec),
                                  gko::stop::ResidualNorm<double>::build().with_reduction_factor(1e-10).on(exec));
        };
        auto hb = dense::create(exec->get_master(), gko::dim<2>(n, 1));
        double bb = 0.0;
        for (gko::size_type i = 0; i < n; ++i) {
            hb->at(i, 0) = std::cos(0.3 * static_cast<double>(i));
            bb += hb->at(i, 0) * hb->at(i, 0);
        }
        const double bnorm = std::sqrt(bb);
        auto b = hb->clone(exec);
        auto x = dense::create(exec, gko::dim<2>(n, 1));

        x->fill(0.0);
        auto plain = gko::solver::Cg<double>::build().with_criteria(criteria().first, criteria().second).on(exec)->generate(A);
        plain->apply(gko::lend(b), gko::lend(x));
        const long plain_iters = static_cast<long>(plain->get_last_iteration_count());

        x->fill(0.0);
        auto cg = gko::solver::Cg<double>::build()
                      .with_criteria(criteria().first, criteria().second)
                      .with_preconditioner(gko::preconditioner::Ic<double, gko::int32>::build()
                                               .with_factorization_factory(par_ict::build().on(exec))
                                               .on(exec))
                      .on(exec)
                      ->generate(A);
        cg->apply(gko::lend(b), gko::lend(x));
        const long cg_iters = static_cast<long>(cg->get_last_iteration_count());
        ok &= check("cg_ict_converged", cg_iters > 0 && cg_iters < plain_iters && residual(ha, x->clone(exec->get_master()).get(), hb.get()) <= 1e-8 * bnorm);

        std::cout << "par_ict_preconditioned_solver: rows=" << n << " a_nnz=" << a_nnz << " l_nnz=" << hl.v.size() << " cg_ict_iterations=" << cg_iters
                  << " cg_plain_iterations=" << plain_iters << std::endl;
        return ok ? 0 : 1;
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
