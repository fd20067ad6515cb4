// gko::matrix::Dense<double> of the host mirror as an operator: Dense::apply (both forms) on the values of the
// reference's own tests (reference/test/matrix/dense_kernels.cpp, AppliesToDense :206-221 and
// AppliesLinearCombinationToDense :244-263, including the untouched stride slot values[3]), Dense::transpose
// (NonSquareMatrixIsTransposable :2149-2156 and a round trip), and solver::Cg and solver::Bicg on a small dense SPD matrix
// (Bicg takes the transpose through Transposable).  Prints one "<what> ok" line per check:
//   dense_operator_mirror: apply ok
//   dense_operator_mirror: advanced_apply ok
//   dense_operator_mirror: transpose ok
//   dense_operator_mirror: cg ok
//   dense_operator_mirror: bicg ok
#include <ginkgo/ginkgo.hpp>

#include <cmath>
#include <iostream>
#include <vector>

using dense = gko::matrix::Dense<double>;

// a rows x cols matrix on `exec` whose buffer (rows x stride) holds `buffer`
static std::unique_ptr<dense> with_buffer(std::shared_ptr<const gko::Executor> exec, gko::dim<2> size, gko::size_type stride,
                                          const std::vector<double>& buffer)
{
    auto h = dense::create(exec->get_master(), size, stride);
    for (gko::size_type i = 0; i < buffer.size(); ++i) h->get_values()[i] = buffer[i];
    return h->clone(exec);
}

static std::vector<double> buffer_of(const dense* d)
{
    auto h = d->clone(d->get_executor()->get_master());
    return std::vector<double>(h->get_const_values(), h->get_const_values() + h->get_num_stored_elements());
}

static int failures = 0;
static void report(const char* what, bool ok)
{
    std::cout << "dense_operator_mirror: " << what << (ok ? " ok" : " WRONG") << std::endl;
    if (!ok) ++failures;
}

template <typename Solver>
static bool solves(std::shared_ptr<const gko::Executor> exec, std::shared_ptr<const dense> A, const dense* b, const std::vector<double>& want)
{
    auto solver = Solver::build()
                      .with_criteria(gko::stop::Iteration::build().with_max_iters(200u).on(exec),
                                     gko::stop::ResidualNorm<double>::build().with_reduction_factor(1e-12).on(exec))
                      .on(exec)
                      ->generate(A);
    auto x = dense::create(exec, b->get_size());
    x->fill(0.0);
    solver->apply(b, gko::lend(x));
    const auto got = buffer_of(x.get());
    double err = 0.0, norm = 0.0;
    for (std::size_t i = 0; i < want.size(); ++i) {
        err += (got[i] - want[i]) * (got[i] - want[i]);
        norm += want[i] * want[i];
    }
    return solver->get_last_iteration_count() > 0 && std::sqrt(err) <= 1e-9 * std::sqrt(norm);
}

int main()
{
    try {
        auto exec = gko::HipExecutor::create(0, gko::ReferenceExecutor::create());
        auto mtx1 = with_buffer(exec, gko::dim<2>(2, 3), 4, {1.0, 2.0, 3.0, 0.0, 1.5, 2.5, 3.5, 0.0});
        auto mtx2 = with_buffer(exec, gko::dim<2>(2, 2), 2, {1.0, -1.0, -2.0, 2.0});
        const std::vector<double> mtx3{1.0, 2.0, 3.0, -1.0, 0.5, 1.5, 2.5, 0.0};
        {
            auto c = with_buffer(exec, gko::dim<2>(2, 3), 4, mtx3);
            mtx2->apply(gko::lend(mtx1), gko::lend(c));
            report("apply", buffer_of(c.get()) == std::vector<double>{-0.5, -0.5, -0.5, -1.0, 1.0, 1.0, 1.0, 0.0});
        }
        {
            auto c = with_buffer(exec, gko::dim<2>(2, 3), 4, mtx3);
            auto alpha = gko::initialize<dense>({-1.0}, exec), beta = gko::initialize<dense>({2.0}, exec);
            mtx2->apply(gko::lend(alpha), gko::lend(mtx1), gko::lend(beta), gko::lend(c));
            report("advanced_apply", buffer_of(c.get()) == std::vector<double>{2.5, 4.5, 6.5, -1.0, 0.0, 2.0, 4.0, 0.0});
        }
        {
            auto mtx4 = with_buffer(exec, gko::dim<2>(2, 3), 4, {1.0, 3.0, 2.0, 9.0, 0.0, 5.0, 0.0, 9.0});
            auto transposed = mtx4->transpose();
            auto t = gko::as<dense>(transposed.get());
            bool ok = t->get_size() == gko::dim<2>(3, 2) && buffer_of(t) == std::vector<double>{1.0, 0.0, 3.0, 5.0, 2.0, 0.0};
            auto back = with_buffer(exec, gko::dim<2>(2, 3), 4, std::vector<double>(8, -7.0));
            t->transpose(back.get());
            ok = ok && buffer_of(back.get()) == std::vector<double>{1.0, 3.0, 2.0, -7.0, 0.0, 5.0, 0.0, -7.0};
            bool threw = false;
            try {
                mtx4->transpose(back.get());
            } catch (const gko::DimensionMismatch&) {
                threw = true;
            }
            report("transpose", ok && threw);
        }
        {
            // SPD: A = M^T M / n + 2 I with M(i,j) = sin(i + 2 j + 1); b = A x for a known x
            const gko::size_type n = 40;
            std::vector<double> m(n * n), a(n * n, 0.0), want(n), rhs(n, 0.0);
            for (gko::size_type i = 0; i < n; ++i) for (gko::size_type j = 0; j < n; ++j) m[i * n + j] = std::sin(static_cast<double>(i + 2 * j + 1));
            for (gko::size_type i = 0; i < n; ++i) {
                for (gko::size_type j = 0; j < n; ++j) {
                    for (gko::size_type l = 0; l < n; ++l) a[i * n + j] += m[l * n + i] * m[l * n + j] / static_cast<double>(n);
                }
                a[i * n + i] += 2.0;
                want[i] = std::cos(0.3 * static_cast<double>(i));
            }
            for (gko::size_type i = 0; i < n; ++i) for (gko::size_type j = 0; j < n; ++j) rhs[i] += a[i * n + j] * want[j];
            std::shared_ptr<const dense> A = with_buffer(exec, gko::dim<2>(n, n), n, a);
            auto b = with_buffer(exec, gko::dim<2>(n, 1), 1, rhs);
            report("cg", solves<gko::solver::Cg<double>>(exec, A, b.get(), want));
            report("bicg", solves<gko::solver::Bicg<double>>(exec, A, b.get(), want));
        }
        return failures;
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
