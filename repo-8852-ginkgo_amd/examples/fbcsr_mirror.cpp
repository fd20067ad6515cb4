// gko::matrix::Fbcsr<double, int32> of the host mirror on a block system: kron(2-D 5-point Poisson on a g x g grid,
// SPD 3 x 3), i.e. three unknowns per grid point.  The matrix is read as Csr, converted to Fbcsr (block size 3), both are
// applied (plain and alpha/beta form) and solver::Cg solves two right-hand sides on each; both formats add a row's terms in the same order,
// so everything is compared bit for bit.  Prints one line:
//   fbcsr_mirror: apply_bits_equal=<0|1> advanced_bits_equal=<0|1> cg_iterations_fbcsr=<n> cg_iterations_csr=<n> x_bits_equal=<0|1>
#include <ginkgo/ginkgo.hpp>

#include <cmath>
#include <cstring>
#include <iostream>
#include <vector>

using dense = gko::matrix::Dense<double>;
using csr = gko::matrix::Csr<double, gko::int32>;
using fbcsr = gko::matrix::Fbcsr<double, gko::int32>;

static bool same_bits(const dense* a, const dense* b)
{
    auto ha = a->clone(a->get_executor()->get_master()), hb = b->clone(b->get_executor()->get_master());
    for (gko::size_type i = 0; i < a->get_size()[0]; ++i) {
        for (gko::size_type j = 0; j < a->get_size()[1]; ++j) {
            const double x = ha->at(i, j), y = hb->at(i, j);
            if (std::memcmp(&x, &y, sizeof(double)) != 0) return false;
        }
    }
    return true;
}

int main()
{
    try {
        auto exec = gko::HipExecutor::create(0, gko::ReferenceExecutor::create());
        const int g = 8, bs = 3;
        const double spd[3][3] = {{4.0, 1.0, 0.5}, {1.0, 3.0, 0.25}, {0.5, 0.25, 2.0}};
        const gko::size_type n = static_cast<gko::size_type>(g) * g * bs;
        gko::matrix_data<double, gko::int32> data;
        data.size = {n, n};
        for (int p = 0; p < g * g; ++p) {
            const int px = p % g, py = p / g;
            for (int ib = 0; ib < bs; ++ib) {
                // neighbours in ascending order of their index: the row comes out sorted
                const int nb[5] = {py > 0 ? p - g : -1, px > 0 ? p - 1 : -1, p, px + 1 < g ? p + 1 : -1, py + 1 < g ? p + g : -1};
                for (int q : nb) {
                    if (q < 0) continue;
                    for (int jb = 0; jb < bs; ++jb) data.nonzeros.emplace_back(p * bs + ib, q * bs + jb, (q == p ? 4.0 : -1.0) * spd[ib][jb]);
                }
            }
        }
        auto A = gko::share(csr::create(exec));
        A->read(data);
        auto B = gko::share(fbcsr::create(exec, bs));
        A->convert_to(B.get());
        auto Bread = fbcsr::create(exec, bs);
        Bread->read(data);
        const bool shape = B->get_block_size() == bs && B->get_num_block_rows() == g * g && B->get_num_block_cols() == g * g &&
                           B->get_num_stored_elements() == A->get_num_stored_elements() && B->get_num_stored_blocks() * bs * bs == B->get_num_stored_elements() &&
                           Bread->get_num_stored_blocks() == B->get_num_stored_blocks() && B->is_sorted_by_column_index();

        auto b = dense::create(exec->get_master(), gko::dim<2>(n, 2));
        for (gko::size_type i = 0; i < n; ++i) {
            b->at(i, 0) = std::sin(0.1 * static_cast<double>(i));
            b->at(i, 1) = 1.0 / (1.0 + static_cast<double>(i));
        }
        auto db = b->clone(exec);
        auto ya = dense::create(exec, gko::dim<2>(n, 2)), yb = dense::create(exec, gko::dim<2>(n, 2));
        A->apply(gko::lend(db), gko::lend(ya));
        B->apply(gko::lend(db), gko::lend(yb));
        const bool apply_equal = same_bits(ya.get(), yb.get());
        auto alpha = gko::initialize<dense>({2.0}, exec), beta = gko::initialize<dense>({-1.0}, exec);
        A->apply(gko::lend(alpha), gko::lend(db), gko::lend(beta), gko::lend(ya));
        B->apply(gko::lend(alpha), gko::lend(db), gko::lend(beta), gko::lend(yb));
        const bool advanced_equal = same_bits(ya.get(), yb.get());
        // round trip and transpose keep the entries
        auto back = csr::create(exec);
        B->convert_to(back.get());
        auto tt = B->transpose()->transpose();
        tt->apply(gko::lend(db), gko::lend(ya));
        B->apply(gko::lend(db), gko::lend(yb));
        const bool round_trip = back->get_num_stored_elements() == A->get_num_stored_elements() && same_bits(ya.get(), yb.get());

        // two right-hand sides: Cg then runs the reference's kernel sequence for both formats (with one, a Csr system
        // carries the dot products inside its SpMV launch, which partitions their sums differently from any other operator)
        auto rhs = db->clone();
        long iters[2];
        std::unique_ptr<dense> x[2];
        const std::shared_ptr<const gko::LinOp> systems[2] = {B, A};
        for (int k = 0; k < 2; ++k) {
            auto solver = gko::solver::Cg<double>::build()
                              .with_criteria(gko::stop::Iteration::build().with_max_iters(400u).on(exec),
                                             gko::stop::ResidualNorm<double>::build().with_reduction_factor(1e-10).on(exec))
                              .on(exec)
                              ->generate(systems[k]);
            x[k] = dense::create(exec, gko::dim<2>(n, 2));
            x[k]->fill(0.0);
            solver->apply(gko::lend(rhs), gko::lend(x[k]));
            iters[k] = static_cast<long>(solver->get_last_iteration_count());
        }
        const bool x_equal = same_bits(x[0].get(), x[1].get());
        std::cout << "fbcsr_mirror: apply_bits_equal=" << (apply_equal && shape) << " advanced_bits_equal=" << (advanced_equal && round_trip)
                  << " cg_iterations_fbcsr=" << iters[0] << " cg_iterations_csr=" << iters[1] << " x_bits_equal=" << x_equal << std::endl;
        return apply_equal && advanced_equal && shape && round_trip && x_equal && iters[0] == iters[1] ? 0 : 1;
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
