// A Galerkin coarse operator through the host mirror: A is the 2-D 5-point Poisson matrix on a g x g grid, P the
// piecewise-constant prolongation over 2 x 2 aggregates, R = P^T by transpose(), and A_c = R (A P) by two
// Csr::apply calls with Csr operands (csr::spgemm, core/matrix/csr.cpp:184-200).  A_c is compared entry for entry,
// value bits included, with the reference's loops run on the host, then solver::Cg solves A_c x = 1.  The alpha /
// beta forms follow: 2 A_c A_c - A_c (advanced_spgemm) and 2 A_c + 3 A_c through an Identity operand (spgeam).
// Prints one line:
//   spgemm_mirror: coarse_rows=<n> coarse_nnz=<n> exact_match=<0|1> advanced_match=<0|1> cg_iterations=<n> converged=<0|1>
#include <ginkgo/ginkgo.hpp>

#include <cmath>
#include <cstring>
#include <iostream>
#include <map>
#include <vector>

using dense = gko::matrix::Dense<double>;
using csr = gko::matrix::Csr<double, gko::int32>;
using mdata = gko::matrix_data<double, gko::int32>;

struct host_csr {
    gko::size_type nrows, ncols;
    std::vector<int> rp, ci;
    std::vector<double> v;
};

static host_csr to_host(const csr* m)
{
    mdata d;
    m->write(d);
    host_csr h{m->get_size()[0], m->get_size()[1], std::vector<int>(m->get_size()[0] + 1, 0), {}, {}};
    for (const auto& e : d.nonzeros) {
        h.rp[e.row + 1]++;
        h.ci.push_back(e.column);
        h.v.push_back(e.value);
    }
    for (gko::size_type r = 0; r < h.nrows; ++r) h.rp[r + 1] += h.rp[r];
    return h;
}

// reference/matrix/csr_kernels.cpp:257-307 (alpha = 1 and no D: :209-252)
static host_csr host_spgemm(const host_csr& a, const host_csr& b, double alpha = 1.0, double beta = 0.0, const host_csr* d = nullptr)
{
    host_csr c{a.nrows, b.ncols, {0}, {}, {}};
    for (gko::size_type row = 0; row < a.nrows; ++row) {
        std::map<int, double> acc;
        if (d) for (int z = d->rp[row]; z < d->rp[row + 1]; ++z) acc[d->ci[z]] += beta * d->v[z];
        for (int k = a.rp[row]; k < a.rp[row + 1]; ++k) {
            for (int z = b.rp[a.ci[k]]; z < b.rp[a.ci[k] + 1]; ++z) acc[b.ci[z]] += alpha * a.v[k] * b.v[z];
        }
        for (const auto& e : acc) {
            c.ci.push_back(e.first);
            c.v.push_back(e.second);
        }
        c.rp.push_back(static_cast<int>(c.ci.size()));
    }
    return c;
}

static bool same(const host_csr& x, const host_csr& y)
{
    return x.nrows == y.nrows && x.ncols == y.ncols && x.rp == y.rp && x.ci == y.ci && x.v.size() == y.v.size() &&
           (x.v.empty() || std::memcmp(x.v.data(), y.v.data(), sizeof(double) * x.v.size()) == 0);
}

int main()
{
    try {
        auto exec = gko::HipExecutor::create(0, gko::ReferenceExecutor::create());
        const int g = 32, gc = g / 2;
        const gko::size_type n = static_cast<gko::size_type>(g) * g, nc = static_cast<gko::size_type>(gc) * gc;
        mdata a_data, p_data;
        a_data.size = {n, n};
        p_data.size = {n, nc};
        for (int p = 0; p < g * g; ++p) {
            const int px = p % g, py = p / g;
            const int nb[5] = {py > 0 ? p - g : -1, px > 0 ? p - 1 : -1, p, px + 1 < g ? p + 1 : -1, py + 1 < g ? p + g : -1};
            for (int q : nb) if (q >= 0) a_data.nonzeros.emplace_back(p, q, q == p ? 4.0 : -1.0);
            p_data.nonzeros.emplace_back(p, (py / 2) * gc + px / 2, 1.0);
        }
        auto A = csr::create(exec), P = csr::create(exec);
        A->read(a_data);
        P->read(p_data);
        auto R = P->transpose();
        auto AP = csr::create(exec, gko::dim<2>(n, nc));
        A->apply(gko::lend(P), gko::lend(AP));
        auto Ac = gko::share(csr::create(exec, gko::dim<2>(nc, nc)));
        R->apply(gko::lend(AP), gko::lend(Ac));

        const host_csr hA = to_host(A.get()), hP = to_host(P.get()), hR = to_host(R.get());
        const host_csr hAc = host_spgemm(hR, host_spgemm(hA, hP));
        const bool exact = same(to_host(Ac.get()), hAc);

        // alpha A_c A_c + beta A_c into a copy of A_c, then alpha A_c + beta (that) through the Identity operand
        auto alpha = gko::initialize<dense>({2.0}, exec), beta = gko::initialize<dense>({-1.0}, exec), three = gko::initialize<dense>({3.0}, exec);
        auto X = csr::create(exec);
        {
            mdata d;
            Ac->write(d);
            X->read(d);
        }
        Ac->apply(gko::lend(alpha), gko::lend(Ac), gko::lend(beta), gko::lend(X));
        const host_csr hX = host_spgemm(hAc, hAc, 2.0, -1.0, &hAc);
        bool advanced = same(to_host(X.get()), hX);
        auto id = gko::matrix::Identity<double>::create(exec, nc);
        Ac->apply(gko::lend(alpha), gko::lend(id), gko::lend(three), gko::lend(X));
        {
            // A_c's pattern lies inside X's: every entry of X is 2 a + 3 x with a literal 0.0 where A_c has none
            const host_csr got = to_host(X.get());
            advanced = advanced && got.rp == hX.rp && got.ci == hX.ci;
            for (gko::size_type row = 0; row < nc && advanced; ++row) {
                for (int z = hX.rp[row]; z < hX.rp[row + 1]; ++z) {
                    double a = 0.0;
                    for (int k = hAc.rp[row]; k < hAc.rp[row + 1]; ++k) if (hAc.ci[k] == hX.ci[z]) a = hAc.v[k];
                    const double want = 2.0 * a + 3.0 * hX.v[z];
                    advanced = advanced && std::memcmp(&want, &got.v[z], sizeof(double)) == 0;
                }
            }
        }

        auto b = dense::create(exec, gko::dim<2>(nc, 1)), x = dense::create(exec, gko::dim<2>(nc, 1));
        b->fill(1.0);
        x->fill(0.0);
        auto solver = gko::solver::Cg<double>::build()
                          .with_criteria(gko::stop::Iteration::build().with_max_iters(500u).on(exec),
                                         gko::stop::ResidualNorm<double>::build().with_reduction_factor(1e-10).on(exec))
                          .on(exec)
                          ->generate(Ac);
        solver->apply(gko::lend(b), gko::lend(x));
        const long iters = static_cast<long>(solver->get_last_iteration_count());
        auto hx = x->clone(exec->get_master());
        double rr = 0.0;
        for (gko::size_type row = 0; row < nc; ++row) {
            double r = 1.0;
            for (int z = hAc.rp[row]; z < hAc.rp[row + 1]; ++z) r -= hAc.v[z] * hx->at(hAc.ci[z], 0);
            rr += r * r;
        }
        const bool converged = iters < 500 && std::sqrt(rr) <= 1e-8 * std::sqrt(static_cast<double>(nc));
        std::cout << "spgemm_mirror: coarse_rows=" << nc << " coarse_nnz=" << Ac->get_num_stored_elements() << " exact_match=" << exact
                  << " advanced_match=" << advanced << " cg_iterations=" << iters << " converged=" << converged << std::endl;
        return exact && advanced && converged ? 0 : 1;
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
