// Records what the reference executor computes for multigrid::Pgm -- the aggregates, the restriction, the coarse
// matrix, the fine operator's column order -- and for whole solver::Multigrid applies over a Pgm hierarchy: the source
// of tests/golden/pgm_ref.json (tests/test_pgm_reference.py turns the output into that fixture and, where the
// reference's objects are present, runs this program again and compares).  Our own program over the reference's public
// API, like tools/multigrid_ref_record.cpp, and built the same way:
//
//   g++ -std=c++14 -O1 -fPIC -ffp-contract=off -pthread -w -Ioracle/_ref/include -I$GINKGO_REF/include
//       -I$GINKGO_REF tools/pgm_ref_record.cpp $(find oracle/_ref/obj -name '*.o') -o pgm_ref_record -lm
//
// Input (stdin), one case per line as tests/pgm_util.recorder_input() writes them; numbers are decimal integers or
// hexadecimal floats, a matrix is "<n> <nnz> row_ptrs col_idxs vals":
//   generate <name> <max_iterations> <max_unassigned_ratio> <deterministic> <skip_sorting> matrix
//   solve    <name> <max_iterations> <max_unassigned_ratio> <deterministic> and then what the solve line of
//            tools/multigrid_ref_record.cpp carries; every mg_level word stands for that Pgm factory
// Output (stdout): one line per array, "<name> <what> <count> <items...>", doubles as hexadecimal floats.
#include <ginkgo/ginkgo.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

using csr = gko::matrix::Csr<double, gko::int32>;
using dense = gko::matrix::Dense<double>;
using pgm = gko::multigrid::Pgm<double, gko::int32>;
using jacobi = gko::preconditioner::Jacobi<double, gko::int32>;

static void put_vals(const std::string& tag, const std::string& what, const double* p, size_t count)
{
    std::printf("%s %s %zu", tag.c_str(), what.c_str(), count);
    for (size_t i = 0; i < count; ++i) std::printf(" %a", p[i]);
    std::printf("\n");
}

static void put_dense(const std::string& tag, const std::string& what, const dense* m)
{
    std::vector<double> v;
    for (size_t i = 0; i < m->get_size()[0]; ++i) {
        for (size_t j = 0; j < m->get_size()[1]; ++j) v.push_back(m->at(i, j));
    }
    put_vals(tag, what, v.data(), v.size());
}

template <class T>
static void put_ints(const std::string& tag, const std::string& what, const T* p, size_t count)
{
    std::printf("%s %s %zu", tag.c_str(), what.c_str(), count);
    for (size_t i = 0; i < count; ++i) std::printf(" %lld", static_cast<long long>(p[i]));
    std::printf("\n");
}

static void put_csr(const std::string& tag, const std::string& what, const gko::LinOp* op)
{
    auto m = gko::as<csr>(op);
    put_ints(tag, what + "/row_ptrs", m->get_const_row_ptrs(), m->get_size()[0] + 1);
    put_ints(tag, what + "/col_idxs", m->get_const_col_idxs(), m->get_num_stored_elements());
    put_vals(tag, what + "/vals", m->get_const_values(), m->get_num_stored_elements());
}

static double number(std::istream& in)
{
    std::string word;
    in >> word;
    return std::strtod(word.c_str(), nullptr);
}

static std::shared_ptr<dense> read_dense(std::shared_ptr<const gko::Executor> ref, long rows, long cols)
{
    auto m = gko::share(dense::create(ref, gko::dim<2>(rows, cols)));
    for (long i = 0; i < rows; ++i) {
        for (long j = 0; j < cols; ++j) m->at(i, j) = number(std::cin);
    }
    return m;
}

static std::shared_ptr<csr> read_csr(std::shared_ptr<const gko::Executor> ref)
{
    long n = 0, nnz = 0;
    std::cin >> n >> nnz;
    gko::array<gko::int32> rp(ref, n + 1), ci(ref, nnz);
    gko::array<double> v(ref, nnz);
    for (long i = 0; i <= n; ++i) std::cin >> rp.get_data()[i];
    for (long i = 0; i < nnz; ++i) std::cin >> ci.get_data()[i];
    for (long i = 0; i < nnz; ++i) v.get_data()[i] = number(std::cin);
    return gko::share(csr::create(ref, gko::dim<2>(n, n), std::move(v), std::move(ci), std::move(rp)));
}

static std::vector<std::string> read_words()
{
    long count = 0;
    std::cin >> count;
    std::vector<std::string> words(count);
    for (auto& w : words) std::cin >> w;
    return words;
}

struct iteration_logger : gko::log::Logger {
    mutable long last = -1;
    void on_iteration_complete(const gko::LinOp*, const gko::size_type& it, const gko::LinOp*, const gko::LinOp*,
                               const gko::LinOp*) const override
    {
        last = static_cast<long>(it);
    }
    iteration_logger() : gko::log::Logger(gko::log::Logger::iteration_complete_mask) {}
};

int main()
{
    auto ref = gko::ReferenceExecutor::create();
    std::string word, name;
    while (std::cin >> word) {
        long pgm_iterations = 0, pgm_deterministic = 0;
        std::cin >> name >> pgm_iterations;
        const double pgm_ratio = number(std::cin);
        std::cin >> pgm_deterministic;
        if (word == "generate") {
            long skip = 0;
            std::cin >> skip;
            auto a = read_csr(ref);
            if (!std::cin) return 3;
            auto level = pgm::build()
                             .with_max_iterations(static_cast<unsigned>(pgm_iterations))
                             .with_max_unassigned_ratio(pgm_ratio)
                             .with_deterministic(pgm_deterministic != 0)
                             .with_skip_sorting(skip != 0)
                             .on(ref)
                             ->generate(a);
            const size_t n = a->get_size()[0];
            put_ints(name, "agg", level->get_const_agg(), n);
            auto restriction = gko::as<gko::matrix::SparsityCsr<double, gko::int32>>(level->get_restrict_op());
            const long long num_agg[1] = {static_cast<long long>(restriction->get_size()[0])};
            put_ints(name, "num_agg", num_agg, 1);
            put_ints(name, "restrict/row_ptrs", restriction->get_const_row_ptrs(), restriction->get_size()[0] + 1);
            put_ints(name, "restrict/col_idxs", restriction->get_const_col_idxs(), n);
            auto fine = gko::as<csr>(level->get_fine_op());
            put_ints(name, "fine/col_idxs", fine->get_const_col_idxs(), fine->get_num_stored_elements());
            put_csr(name, "coarse", level->get_coarse_op().get());
        } else if (word == "solve") {
            std::string cycle, mid_case, coarsest, guess;
            long post_uses_pre = 0, max_levels = 0, min_coarse_rows = 0, iters = 0, max_iters = 0;
            std::cin >> cycle >> mid_case >> post_uses_pre >> max_levels >> min_coarse_rows >> coarsest;
            const double relax = number(std::cin);
            std::cin >> iters >> guess >> max_iters;
            const double reduction = number(std::cin);
            const auto level_words = read_words(), pre_words = read_words(), mid_words = read_words(),
                       post_words = read_words();
            auto a = read_csr(ref);
            const long n = static_cast<long>(a->get_size()[0]);
            auto b = read_dense(ref, n, 1), x = read_dense(ref, n, 1);
            if (!std::cin) return 3;
            using factories = std::vector<std::shared_ptr<const gko::LinOpFactory>>;
            factories levels, pre, mid, post, coarsest_list;
            for (const auto& w : level_words) {
                (void)w;
                levels.push_back(gko::share(pgm::build()
                                                .with_max_iterations(static_cast<unsigned>(pgm_iterations))
                                                .with_max_unassigned_ratio(pgm_ratio)
                                                .with_deterministic(pgm_deterministic != 0)
                                                .on(ref)));
            }
            auto smoothers = [&](const std::vector<std::string>& words, factories& out) {
                for (const auto& w : words) {
                    if (w == "null") {
                        out.push_back(nullptr);
                    } else if (w == "eye") {
                        out.push_back(gko::share(gko::matrix::IdentityFactory<double>::create(ref)));
                    } else {
                        out.push_back(gko::share(jacobi::build().with_max_block_size(1u).on(ref)));
                    }
                }
            };
            smoothers(pre_words, pre);
            smoothers(mid_words, mid);
            smoothers(post_words, post);
            if (coarsest == "direct") {
                coarsest_list.push_back(gko::share(
                    gko::experimental::solver::Direct<double, gko::int32>::build()
                        .with_factorization(gko::experimental::factorization::Lu<double, gko::int32>::build()
                                                .with_symmetric_sparsity(true)
                                                .on(ref))
                        .on(ref)));
            }
            if (coarsest == "cg") {
                coarsest_list.push_back(gko::share(
                    gko::solver::Cg<double>::build().with_criteria(gko::stop::Iteration::build().with_max_iters(10u).on(ref)).on(ref)));
            }
            namespace mg = gko::solver::multigrid;
            std::vector<std::shared_ptr<const gko::stop::CriterionFactory>> criteria;
            criteria.push_back(
                gko::share(gko::stop::Iteration::build().with_max_iters(static_cast<gko::size_type>(max_iters)).on(ref)));
            if (reduction != 0.0) {
                criteria.push_back(gko::share(gko::stop::ResidualNorm<double>::build()
                                                  .with_baseline(gko::stop::mode::rhs_norm)
                                                  .with_reduction_factor(reduction)
                                                  .on(ref)));
            }
            auto solver =
                gko::solver::Multigrid::build()
                    .with_mg_level(levels)
                    .with_pre_smoother(pre)
                    .with_mid_smoother(mid)
                    .with_post_smoother(post)
                    .with_post_uses_pre(post_uses_pre != 0)
                    .with_mid_case(mid_case == "both"            ? mg::mid_smooth_type::both
                                   : mid_case == "post_smoother" ? mg::mid_smooth_type::post_smoother
                                   : mid_case == "pre_smoother"  ? mg::mid_smooth_type::pre_smoother
                                                                 : mg::mid_smooth_type::standalone)
                    .with_max_levels(static_cast<gko::size_type>(max_levels))
                    .with_min_coarse_rows(static_cast<gko::size_type>(min_coarse_rows))
                    .with_coarsest_solver(coarsest_list)
                    .with_cycle(cycle == "v" ? mg::cycle::v : cycle == "f" ? mg::cycle::f : mg::cycle::w)
                    .with_smoother_relax(relax)
                    .with_smoother_iters(static_cast<gko::size_type>(iters))
                    .with_default_initial_guess(guess == "zero"  ? gko::solver::initial_guess_mode::zero
                                                : guess == "rhs" ? gko::solver::initial_guess_mode::rhs
                                                                 : gko::solver::initial_guess_mode::provided)
                    .with_criteria(criteria)
                    .on(ref)
                    ->generate(a);
            auto logger = std::make_shared<iteration_logger>();
            solver->add_logger(logger);
            solver->apply(b.get(), x.get());
            put_dense(name, "x", x.get());
            const long long its[1] = {logger->last};
            put_ints(name, "iterations", its, 1);
            std::vector<long long> rows;
            for (const auto& level : solver->get_mg_level_list()) {
                rows.push_back(static_cast<long long>(level->get_coarse_op()->get_size()[0]));
            }
            put_ints(name, "levels", rows.data(), rows.size());
        } else {
            return 2;
        }
    }
    return 0;
}
