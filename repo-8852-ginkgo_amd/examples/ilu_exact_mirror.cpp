// The exact ILU(0) / IC(0) through the host mirror: factorization::Ilu and factorization::Ic of a 2-D 5-point
// matrix on a g x g grid (an upwind convection term makes the ILU input unsymmetric), compared value bit for value
// bit with the reference's loops run on the host (reference/factorization/ilu_kernels.cpp:56-97,
// ic_kernels.cpp:53-100), then solver::Cg with preconditioner::Ic and solver::Gmres with preconditioner::Ilu, both
// through with_factorization_factory.  Prints one "check <what>: ok|FAILED" line per check and
//   ilu_exact_mirror: rows=<n> cg_ic_iterations=<n> gmres_ilu_iterations=<n> cg_plain_iterations=<n>
#include <ginkgo/ginkgo.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <iostream>
#include <vector>

using dense = gko::matrix::Dense<double>;
using csr = gko::matrix::Csr<double, gko::int32>;
using mdata = gko::matrix_data<double, gko::int32>;

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

static int find(const host_csr& m, int row, int col)
{
    const auto b = m.ci.begin() + m.rp[row], e = m.ci.begin() + m.rp[row + 1];
    const auto it = std::lower_bound(b, e, col);
    return it != e && *it == col ? static_cast<int>(it - m.ci.begin()) : -1;
}

static void host_compute_lu(host_csr& m)
{
    for (int row = 0; row < static_cast<int>(m.n); ++row) {
        for (int nz = m.rp[row]; nz < m.rp[row + 1]; ++nz) {
            const int col = m.ci[nz];
            double value = m.v[nz];
            for (int l = m.rp[row]; l < m.rp[row + 1]; ++l) {
                const int k = m.ci[l];
                if (k >= std::min(row, col)) continue;
                const int u = find(m, k, col);
                if (u >= 0) value -= m.v[l] * m.v[u];
            }
            m.v[nz] = row <= col ? value : value / m.v[find(m, col, col)];
        }
    }
}

static void host_ic_compute(host_csr& m)
{
    for (int row = 0; row < static_cast<int>(m.n); ++row) {
        for (int nz = m.rp[row]; nz < m.rp[row + 1]; ++nz) {
            const int col = m.ci[nz];
            if (col > row) continue;
            double sum = 0.0;
            for (int l = m.rp[row]; l < m.rp[row + 1] && m.ci[l] < col; ++l) {
                const int h = find(m, col, m.ci[l]);
                if (h >= 0) sum += m.v[l] * m.v[h];
            }
            m.v[nz] = row == col ? std::sqrt(m.v[nz] - sum) : (m.v[nz] - sum) / m.v[find(m, col, col)];
        }
    }
}

// the part of m with col < row (strict), col == row (diag: 1.0 when unit) and col > row as asked
static host_csr part(const host_csr& m, bool lower, bool unit)
{
    host_csr p{m.n, {0}, {}, {}};
    for (int row = 0; row < static_cast<int>(m.n); ++row) {
        for (int nz = m.rp[row]; nz < m.rp[row + 1]; ++nz) {
            const int col = m.ci[nz];
            if (lower ? col > row : col < row) continue;
            p.ci.push_back(col);
            p.v.push_back(col == row && unit ? 1.0 : m.v[nz]);
        }
        p.rp.push_back(static_cast<int>(p.ci.size()));
    }
    return p;
}

static bool same(const host_csr& x, const host_csr& y)
{
    return x.n == y.n && x.rp == y.rp && x.ci == y.ci && x.v.size() == y.v.size() &&
           (x.v.empty() || std::memcmp(x.v.data(), y.v.data(), sizeof(double) * x.v.size()) == 0);
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
        mdata spd_data, conv_data;
        spd_data.size = {n, n};
        conv_data.size = {n, n};
        for (int p = 0; p < g * g; ++p) {
            const int px = p % g, py = p / g;
            const int nb[5] = {py > 0 ? p - g : -1, px > 0 ? p - 1 : -1, p, px + 1 < g ? p + 1 : -1, py + 1 < g ? p + g : -1};
            for (int q : nb) {
                if (q < 0) continue;
                spd_data.nonzeros.emplace_back(p, q, q == p ? 4.0 : -1.0);
                conv_data.nonzeros.emplace_back(p, q, q == p ? 4.5 : (q < p ? -1.5 : -1.0));
            }
        }
        auto S = gko::share(csr::create(exec)), C = gko::share(csr::create(exec));
        S->read(spd_data);
        C->read(conv_data);
        bool ok = true;

        auto ilu = gko::factorization::Ilu<double, gko::int32>::build().on(exec)->generate(C);
        host_csr hc = to_host(C.get());
        host_compute_lu(hc);
        ok &= check("ilu_l_factor_bits", same(to_host(ilu->get_l_factor().get()), part(hc, true, true)));
        ok &= check("ilu_u_factor_bits", same(to_host(ilu->get_u_factor().get()), part(hc, false, false)));

        auto ic = gko::factorization::Ic<double, gko::int32>::build().with_both_factors(true).on(exec)->generate(S);
        host_csr hs = to_host(S.get());
        host_ic_compute(hs);
        const host_csr hl = part(hs, true, false);
        ok &= check("ic_l_factor_bits", same(to_host(ic->get_l_factor().get()), hl));
        ok &= check("ic_lt_factor_is_transpose", same(to_host(ic->get_lt_factor()->transpose().get()), hl));
        auto ic_l_only = gko::factorization::Ic<double, gko::int32>::build().with_both_factors(false).on(exec)->generate(S);
        ok &= check("ic_without_lt_factor", ic_l_only->get_lt_factor() == nullptr && same(to_host(ic_l_only->get_l_factor().get()), hl));

        auto criteria = [&] {
            return std::make_pair(gko::stop::Iteration::build().with_max_iters(500u).on(exec),
                                  gko::stop::ResidualNorm<double>::build().with_reduction_factor(1e-10).on(exec));
        };
        auto b = dense::create(exec, gko::dim<2>(n, 1)), x = dense::create(exec, gko::dim<2>(n, 1));
        b->fill(1.0);
        const double bnorm = std::sqrt(static_cast<double>(n));

        x->fill(0.0);
        auto plain = gko::solver::Cg<double>::build().with_criteria(criteria().first, criteria().second).on(exec)->generate(S);
        plain->apply(gko::lend(b), gko::lend(x));
        const long plain_iters = static_cast<long>(plain->get_last_iteration_count());

        x->fill(0.0);
        auto cg = gko::solver::Cg<double>::build()
                      .with_criteria(criteria().first, criteria().second)
                      .with_preconditioner(gko::preconditioner::Ic<double, gko::int32>::build()
                                               .with_factorization_factory(gko::factorization::Ic<double, gko::int32>::build().on(exec))
                                               .on(exec))
                      .on(exec)
                      ->generate(S);
        cg->apply(gko::lend(b), gko::lend(x));
        const long cg_iters = static_cast<long>(cg->get_last_iteration_count());
        ok &= check("cg_ic_converged", cg_iters < plain_iters && residual(to_host(S.get()), x->clone(exec->get_master()).get(), 1.0) <= 1e-8 * bnorm);

        x->fill(0.0);
        auto gmres = gko::solver::Gmres<double>::build()
                         .with_criteria(criteria().first, criteria().second)
                         .with_krylov_dim(30u)
                         .with_preconditioner(gko::preconditioner::Ilu<double, gko::int32>::build()
                                                  .with_factorization_factory(gko::factorization::Ilu<double, gko::int32>::build().on(exec))
                                                  .on(exec))
                         .on(exec)
                         ->generate(C);
        gmres->apply(gko::lend(b), gko::lend(x));
        const long gmres_iters = static_cast<long>(gmres->get_last_iteration_count());
        ok &= check("gmres_ilu_converged", gmres_iters < 500 && residual(to_host(C.get()), x->clone(exec->get_master()).get(), 1.0) <= 1e-8 * bnorm);

        std::cout << "ilu_exact_mirror: rows=" << n << " cg_ic_iterations=" << cg_iters << " gmres_ilu_iterations=" << gmres_iters
                  << " cg_plain_iterations=" << plain_iters << std::endl;
        return ok ? 0 : 1;
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
