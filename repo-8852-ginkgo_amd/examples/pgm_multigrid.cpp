// Algebraic multigrid with gko::multigrid::Pgm of the host mirror, and the driver of tests/test_cpp_pgm.py.
//   pgm_multigrid            on the device: one Pgm level of the reference's 5 x 5 test matrix (agg and the coarse
//                            matrix printed), then Cg preconditioned by one V-cycle of a Pgm hierarchy on a 2-D Poisson
//                            problem against plain Cg
//   pgm_multigrid check      host only: the factory's parameters and defaults; prints "pgm factory ok"
//   pgm_multigrid run        on the device, one case per line of stdin as tests/pgm_util.recorder_input() writes them
//                            (numbers as decimals or hexadecimal floats, a matrix is "<n> <nnz> row_ptrs col_idxs vals"):
//     generate <name> <max_iterations> <max_unassigned_ratio> <deterministic> <skip_sorting> matrix
//         prints agg, num_agg, restrict/row_ptrs, restrict/col_idxs, fine/col_idxs and the coarse Csr, one array per line
//         as "<name> <what> <count> <items...>", "<name> fine_is_given 1 <0|1>", and "<name> fbcsr_same 1 <0|1>": whether the
//         matrix as an Fbcsr with block size 1 gives the same level with the converted Csr as its fine operator
//     solve <name> <max_iterations> <max_unassigned_ratio> <deterministic> <v|f|w> <mid_case> <post_uses_pre> <max_levels>
//           <min_coarse_rows> <direct> <relax> <smoother_iters> <zero|rhs|provided> <max_iters> <reduction, 0: none>
//           1 pgm 1 jacobi 0 0 matrix b x
//         a solver::Multigrid over Pgm levels with a scalar Jacobi smoother and Direct on the coarsest level; prints x,
//         iterations and levels
#include <ginkgo/ginkgo.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

using csr = gko::matrix::Csr<double, gko::int32>;
using dense = gko::matrix::Dense<double>;
using mg = gko::solver::Multigrid;
using pgm = gko::multigrid::Pgm<double, gko::int32>;
using jacobi = gko::preconditioner::Jacobi<double, gko::int32>;
namespace mgns = gko::solver::multigrid;

static double number(std::istream& in)
{
    std::string word;
    in >> word;
    return std::strtod(word.c_str(), nullptr);
}

static std::shared_ptr<csr> upload(std::shared_ptr<const gko::Executor> exec, long n, const std::vector<gko::int32>& rp,
                                   const std::vector<gko::int32>& ci, const std::vector<double>& v)
{
    auto A = gko::share(csr::create(exec, gko::dim<2>(n, n), ci.size(), std::make_shared<csr::merge_path>()));
    auto host = exec->get_master();
    exec->copy_from(host.get(), n + 1, rp.data(), A->get_row_ptrs());
    exec->copy_from(host.get(), ci.size(), ci.data(), A->get_col_idxs());
    exec->copy_from(host.get(), v.size(), v.data(), A->get_values());
    return A;
}

static std::shared_ptr<csr> read_csr(std::shared_ptr<const gko::Executor> exec)
{
    long n = 0, nnz = 0;
    std::cin >> n >> nnz;
    std::vector<gko::int32> rp(n + 1), ci(nnz);
    std::vector<double> v(nnz);
    for (auto& t : rp) std::cin >> t;
    for (auto& t : ci) std::cin >> t;
    for (auto& t : v) t = number(std::cin);
    return upload(exec, n, rp, ci, v);
}

static std::shared_ptr<dense> read_vector(std::shared_ptr<const gko::Executor> exec, long n)
{
    std::vector<double> h(n);
    for (auto& t : h) t = number(std::cin);
    auto d = gko::share(dense::create(exec, gko::dim<2>(n, 1)));
    exec->copy_from(exec->get_master().get(), n, h.data(), d->get_values());
    return d;
}

template <typename T>
static std::vector<T> to_host(const gko::Executor* exec, const T* data, gko::size_type n)
{
    std::vector<T> out(n);
    exec->get_master()->copy_from(exec, n, data, out.data());
    return out;
}

static void put_ints(const std::string& tag, const std::string& what, const gko::Executor* exec, const gko::int32* data, gko::size_type n)
{
    std::printf("%s %s %zu", tag.c_str(), what.c_str(), static_cast<size_t>(n));
    for (auto t : to_host(exec, data, n)) std::printf(" %d", t);
    std::printf("\n");
}

static void put_vals(const std::string& tag, const std::string& what, const gko::Executor* exec, const double* data, gko::size_type n)
{
    std::printf("%s %s %zu", tag.c_str(), what.c_str(), static_cast<size_t>(n));
    for (auto t : to_host(exec, data, n)) std::printf(" %a", t);
    std::printf("\n");
}

static void put_level(const std::string& name, const pgm* level, const gko::LinOp* given)
{
    const auto exec = level->get_executor().get();
    const auto n = level->get_size()[0];
    auto restriction = dynamic_cast<const csr*>(level->get_restrict_op().get());
    auto coarse = dynamic_cast<const csr*>(level->get_coarse_op().get());
    auto fine = dynamic_cast<const csr*>(level->get_fine_op().get());
    put_ints(name, "agg", exec, level->get_const_agg(), n);
    std::printf("%s num_agg 1 %zu\n", name.c_str(), static_cast<size_t>(restriction->get_size()[0]));
    put_ints(name, "restrict/row_ptrs", exec, restriction->get_const_row_ptrs(), restriction->get_size()[0] + 1);
    put_ints(name, "restrict/col_idxs", exec, restriction->get_const_col_idxs(), n);
    put_ints(name, "fine/col_idxs", exec, fine->get_const_col_idxs(), fine->get_num_stored_elements());
    put_ints(name, "coarse/row_ptrs", exec, coarse->get_const_row_ptrs(), coarse->get_size()[0] + 1);
    put_ints(name, "coarse/col_idxs", exec, coarse->get_const_col_idxs(), coarse->get_num_stored_elements());
    put_vals(name, "coarse/vals", exec, coarse->get_const_values(), coarse->get_num_stored_elements());
    std::printf("%s fine_is_given 1 %d\n", name.c_str(), static_cast<int>(level->get_fine_op().get() == given));
}

static int check()
{
    auto ref = gko::ReferenceExecutor::create();
    auto defaults = pgm::build().on(ref);
    auto set = pgm::build().with_max_iterations(2u).with_max_unassigned_ratio(0.1).with_deterministic(true).with_skip_sorting(true).on(ref);
    int wrong = 0;
    wrong += defaults->max_iterations_ != 15u || defaults->max_unassigned_ratio_ != 0.05 || defaults->deterministic_ || defaults->skip_sorting_;
    wrong += set->max_iterations_ != 2u || set->max_unassigned_ratio_ != 0.1 || !set->deterministic_ || !set->skip_sorting_;
    // an empty matrix generates nothing and touches no device
    auto empty = set->generate(gko::share(csr::create(ref, gko::dim<2>(0, 0))));
    wrong += empty->get_coarse_op() != nullptr || empty->get_system_matrix()->get_size()[0] != 0;
    std::printf(wrong ? "pgm factory WRONG (%d)\n" : "pgm factory ok\n", wrong);
    return wrong;
}

static std::shared_ptr<csr> poisson_2d(std::shared_ptr<const gko::Executor> exec, long g)
{
    std::vector<gko::int32> rp(g * g + 1, 0), ci;
    std::vector<double> v;
    for (long i = 0; i < g; ++i) {
        for (long j = 0; j < g; ++j) {
            const long row = i * g + j;
            if (i > 0) ci.push_back(row - g), v.push_back(-1.0);
            if (j > 0) ci.push_back(row - 1), v.push_back(-1.0);
            ci.push_back(row), v.push_back(4.0);
            if (j + 1 < g) ci.push_back(row + 1), v.push_back(-1.0);
            if (i + 1 < g) ci.push_back(row + g), v.push_back(-1.0);
            rp[row + 1] = static_cast<gko::int32>(ci.size());
        }
    }
    return upload(exec, g * g, rp, ci, v);
}

static int tour(std::shared_ptr<const gko::Executor> exec)
{
    // the matrix of reference/test/multigrid/pgm_kernels.cpp and its level: agg {0, 1, 0, 1, 0}, A_c = {6, -5, -4, 5}
    auto A5 = upload(exec, 5, {0, 3, 7, 10, 12, 15}, {0, 1, 2, 0, 1, 3, 4, 0, 2, 4, 1, 3, 1, 2, 4},
                     {5, -3, -3, -3, 5, -2, -1, -3, 5, -1, -3, 5, -2, -2, 5});
    auto level = pgm::build().with_max_iterations(2u).with_max_unassigned_ratio(0.1).with_skip_sorting(true).on(exec)->generate(A5);
    std::printf("agg:");
    for (auto a : to_host(exec.get(), level->get_const_agg(), 5)) std::printf(" %d", a);
    auto coarse = dynamic_cast<const csr*>(level->get_coarse_op().get());
    std::printf("\ncoarse matrix (%zu x %zu):", static_cast<size_t>(coarse->get_size()[0]), static_cast<size_t>(coarse->get_size()[1]));
    for (auto c : to_host(exec.get(), coarse->get_const_values(), coarse->get_num_stored_elements())) std::printf(" %g", c);
    std::printf("\n");

    // Cg on a 2-D Poisson problem, plain and preconditioned by one V-cycle over a deterministic Pgm hierarchy
    const long g = 96, n = g * g;
    auto A = poisson_2d(exec, g);
    auto b = dense::create(exec, gko::dim<2>(n, 1));
    b->fill(1.0);
    auto multigrid = gko::share(
        mg::build()
            .with_mg_level(gko::share(pgm::build().with_deterministic(true).on(exec)))
            .with_pre_smoother(gko::share(jacobi::build().with_max_block_size(1u).on(exec)))
            .with_smoother_iters(2u)
            .with_max_levels(8u)
            .with_min_coarse_rows(32u)
            .with_default_initial_guess(gko::solver::initial_guess_mode::zero)
            .with_criteria(gko::stop::Iteration::build().with_max_iters(1u).on(exec))
            .on(exec));
    for (int with_mg = 0; with_mg < 2; ++with_mg) {
        auto builder = gko::solver::Cg<double>::build();
        builder.with_criteria(gko::share(gko::stop::Iteration::build().with_max_iters(2000u).on(exec)),
                              gko::share(gko::stop::ResidualNorm<double>::build().with_reduction_factor(1e-10).on(exec)));
        if (with_mg) builder.with_preconditioner(multigrid);
        auto solver = builder.on(exec)->generate(A);
        auto x = dense::create(exec, gko::dim<2>(n, 1));
        x->fill(0.0);
        solver->apply(b.get(), x.get());
        exec->synchronize();
        std::printf("%s: %lld iterations\n", with_mg ? "cg + pgm v-cycle" : "cg", static_cast<long long>(solver->get_last_iteration_count()));
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::string(argv[1]) == "check") return check();
    auto exec = gko::HipExecutor::create(0, gko::ReferenceExecutor::create());
    if (argc < 2) return tour(exec);
    std::string word, name;
    while (std::cin >> word) {
        long pgm_iterations = 0, pgm_deterministic = 0;
        std::cin >> name >> pgm_iterations;
        const double pgm_ratio = number(std::cin);
        std::cin >> pgm_deterministic;
        auto factory = [&](bool skip) {
            return gko::share(pgm::build()
                                  .with_max_iterations(static_cast<unsigned>(pgm_iterations))
                                  .with_max_unassigned_ratio(pgm_ratio)
                                  .with_deterministic(pgm_deterministic != 0)
                                  .with_skip_sorting(skip)
                                  .on(exec));
        };
        if (word == "generate") {
            long skip = 0;
            std::cin >> skip;
            auto A = read_csr(exec);
            if (!std::cin) return 3;
            auto level = factory(skip != 0)->generate(A);
            put_level(name, level.get(), A.get());
            // the same matrix as an Fbcsr with block size 1: it comes in through Fbcsr::convert_to(Csr*), the converted
            // Csr (not the Fbcsr) is the fine operator, and the level is the Csr's
            auto blocks = gko::share(gko::matrix::Fbcsr<double, gko::int32>::create(exec, 1));
            A->convert_to(blocks.get());
            auto from_blocks = factory(skip != 0)->generate(blocks);
            const auto n = A->get_size()[0];
            auto c1 = dynamic_cast<const csr*>(level->get_coarse_op().get()), c2 = dynamic_cast<const csr*>(from_blocks->get_coarse_op().get());
            bool same = dynamic_cast<const csr*>(from_blocks->get_fine_op().get()) != nullptr && from_blocks->get_system_matrix().get() == blocks.get();
            same = same && to_host(exec.get(), level->get_const_agg(), n) == to_host(exec.get(), from_blocks->get_const_agg(), n);
            same = same && c1->get_num_stored_elements() == c2->get_num_stored_elements();
            if (same) {
                const auto nnz = c1->get_num_stored_elements();
                const auto v1 = to_host(exec.get(), c1->get_const_values(), nnz), v2 = to_host(exec.get(), c2->get_const_values(), nnz);
                same = to_host(exec.get(), c1->get_const_col_idxs(), nnz) == to_host(exec.get(), c2->get_const_col_idxs(), nnz) &&
                       (nnz == 0 || std::memcmp(v1.data(), v2.data(), nnz * sizeof(double)) == 0);
            }
            std::printf("%s fbcsr_same 1 %d\n", name.c_str(), static_cast<int>(same));
        } else if (word == "solve") {
            std::string cycle, mid_case, coarsest, guess, skip_word;
            long post_uses_pre = 0, max_levels = 0, min_coarse_rows = 0, iters = 0, max_iters = 0;
            std::cin >> cycle >> mid_case >> post_uses_pre >> max_levels >> min_coarse_rows >> coarsest;
            const double relax = number(std::cin);
            std::cin >> iters >> guess >> max_iters;
            const double reduction = number(std::cin);
            for (int i = 0; i < 6; ++i) std::cin >> skip_word;   // "1 pgm 1 jacobi 0 0": the lists this driver serves
            auto A = read_csr(exec);
            const long n = static_cast<long>(A->get_size()[0]);
            auto b = read_vector(exec, n), x = read_vector(exec, n);
            if (!std::cin || coarsest != "direct" || skip_word != "0") return 3;
            using lu = gko::experimental::factorization::Lu<double, gko::int32>;
            using direct = gko::experimental::solver::Direct<double, gko::int32>;
            auto cycles = gko::share(gko::stop::Iteration::build().with_max_iters(static_cast<gko::size_type>(max_iters)).on(exec));
            auto builder = mg::build();
            if (reduction != 0.0) {
                builder.with_criteria(cycles, gko::share(gko::stop::ResidualNorm<double>::build().with_reduction_factor(reduction).on(exec)));
            } else {
                builder.with_criteria(cycles);
            }
            auto solver = builder
                              .with_mg_level(factory(false))
                              .with_pre_smoother(gko::share(jacobi::build().with_max_block_size(1u).on(exec)))
                              .with_post_uses_pre(post_uses_pre != 0)
                              .with_mid_case(mid_case == "both" ? mgns::mid_smooth_type::both : mid_case == "post_smoother" ? mgns::mid_smooth_type::post_smoother
                                             : mid_case == "pre_smoother" ? mgns::mid_smooth_type::pre_smoother : mgns::mid_smooth_type::standalone)
                              .with_smoother_relax(relax)
                              .with_smoother_iters(static_cast<gko::size_type>(iters))
                              .with_max_levels(static_cast<gko::size_type>(max_levels))
                              .with_min_coarse_rows(static_cast<gko::size_type>(min_coarse_rows))
                              .with_coarsest_solver(gko::share(direct::build().with_factorization(gko::share(lu::build().with_symmetric_sparsity(true).on(exec))).on(exec)))
                              .with_cycle(cycle == "v" ? mgns::cycle::v : cycle == "f" ? mgns::cycle::f : mgns::cycle::w)
                              .with_default_initial_guess(guess == "zero" ? gko::solver::initial_guess_mode::zero
                                                          : guess == "rhs" ? gko::solver::initial_guess_mode::rhs : gko::solver::initial_guess_mode::provided)
                              .on(exec)
                              ->generate(A);
            solver->apply(b.get(), x.get());
            exec->synchronize();
            put_vals(name, "x", exec.get(), x->get_const_values(), n);
            std::printf("%s iterations 1 %lld\n%s levels %zu", name.c_str(), static_cast<long long>(solver->get_last_iteration_count()), name.c_str(),
                        solver->get_mg_level_list().size());
            for (const auto& lvl : solver->get_mg_level_list()) std::printf(" %zu", static_cast<size_t>(lvl->get_coarse_op()->get_size()[0]));
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
