// gko::solver::Multigrid and gko::multigrid::FixedCoarsening of the host mirror, driven for tests/test_cpp_multigrid.py.
//   multigrid_mirror            host only: validate() throws for an empty mg_level list, a null entry and the list
//                               lengths the 0 / 1 / n rule forbids; prints "multigrid validate ok"
//   multigrid_mirror time       on the device: the time of one smoother apply through the fused sweep and through the
//                               three-call sequence on 2-D Poisson matrices, as a table (profiles/multigrid_probe_reading.md)
//   multigrid_mirror run        on the device, one case per line of stdin:
//     sequence <name> <individual|same> <v|f|w> <max_levels> <both|post_smoother|pre_smoother|standalone> <rows> [<f>]
//         the dummy hierarchy of the reference's cycle tests (reference/test/solver/multigrid_kernels.cpp): operators that
//         only take a step number.  Prints "<name> trace <what>:<level> ..." in call order; with a trailing cycle letter
//         the solver is generated with the first cycle and switched with set_cycle before the apply.
//     solve <name> <v|f|w> <n> <nnz> row_ptrs col_idxs vals b x      (numbers as decimals or hexadecimal floats)
//         three cycles of the three-level hierarchy (FixedCoarsening on every second row, twice), 2 Jacobi sweeps wrapped
//         by build_smoother, Direct on the coarsest level, zero initial guess.  Prints "<name> x <n> <hex floats>" and
//         "<name> levels <count> <coarse rows...>".  GKOMI_MG_FUSED=0 / 1 in the environment picks the smoother's path.
//     fbcsr <name> <n> <nnz> row_ptrs col_idxs vals
//         FixedCoarsening of the matrix as a Csr and as an Fbcsr with block size 1, and of a Coo.  Prints
//         "<name> fbcsr same coo refused" when the Fbcsr comes in through its conversion with the Csr's R, P and A_c bit
//         for bit, and the Coo, which has no conversion to a Csr, throws NotSupported.
#include <ginkgo/ginkgo.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

using csr = gko::matrix::Csr<double, gko::int32>;
using dense = gko::matrix::Dense<double>;
using mg = gko::solver::Multigrid;
using coarsening = gko::multigrid::FixedCoarsening<double, gko::int32>;
namespace mgns = gko::solver::multigrid;

static std::vector<std::string> trace;

// takes a step number on the plain apply (a smoother, a restriction, a coarsest solver) or on the advanced one (a
// prolongation); an empty tag records nothing (system and coarse matrices)
struct counting_op : gko::LinOp {
    counting_op(std::shared_ptr<const gko::Executor> exec, gko::dim<2> size, std::string tag, bool on_advanced)
        : gko::LinOp(std::move(exec), size), tag_(std::move(tag)), on_advanced_(on_advanced)
    {}
    bool apply_uses_initial_guess() const override { return true; }
protected:
    void apply_impl(const gko::LinOp*, gko::LinOp*) const override
    {
        if (!tag_.empty() && !on_advanced_) trace.push_back(tag_);
    }
    void apply_impl(const gko::LinOp*, const gko::LinOp*, const gko::LinOp*, gko::LinOp*) const override
    {
        if (!tag_.empty() && on_advanced_) trace.push_back(tag_);
    }
    std::string tag_;
    bool on_advanced_;
};

static gko::size_type top_rows = 0;
static std::string level_of(const gko::LinOp* m) { return std::to_string(top_rows - m->get_size()[0]); }

struct counting_factory : gko::LinOpFactory {
    counting_factory(std::shared_ptr<const gko::Executor> exec, std::string what) : gko::LinOpFactory(std::move(exec)), what_(std::move(what)) {}
    std::unique_ptr<gko::LinOp> generate_impl(std::shared_ptr<const gko::LinOp> m) const override
    {
        return std::unique_ptr<gko::LinOp>(new counting_op(exec_, m->get_size(), what_ + ":" + level_of(m.get()), false));
    }
    std::string what_;
};

// a level whose coarse operator has one row less
struct counting_level : gko::LinOp, gko::multigrid::EnableMultigridLevel<double> {
    counting_level(std::shared_ptr<const gko::Executor> exec, std::shared_ptr<const gko::LinOp> fine)
        : gko::LinOp(exec, fine->get_size()), gko::multigrid::EnableMultigridLevel<double>(fine)
    {
        const auto n = fine->get_size()[0];
        const auto lvl = level_of(fine.get());
        this->set_multigrid_level(std::make_shared<counting_op>(exec, gko::dim<2>(n, n - 1), "prolong:" + lvl, true),
                                  std::make_shared<counting_op>(exec, gko::dim<2>(n - 1, n - 1), "", false),
                                  std::make_shared<counting_op>(exec, gko::dim<2>(n - 1, n), "restrict:" + lvl, false));
    }
protected:
    void apply_impl(const gko::LinOp*, gko::LinOp*) const override {}
    void apply_impl(const gko::LinOp*, const gko::LinOp*, const gko::LinOp*, gko::LinOp*) const override {}
};
struct counting_level_factory : gko::LinOpFactory {
    explicit counting_level_factory(std::shared_ptr<const gko::Executor> exec) : gko::LinOpFactory(std::move(exec)) {}
    std::unique_ptr<gko::LinOp> generate_impl(std::shared_ptr<const gko::LinOp> m) const override
    {
        return std::unique_ptr<gko::LinOp>(new counting_level(exec_, m));
    }
};

static mgns::cycle cycle_of(const std::string& c) { return c == "v" ? mgns::cycle::v : c == "f" ? mgns::cycle::f : mgns::cycle::w; }

// FixedCoarsening on every second row of whatever matrix it is handed
struct every_second_row : gko::LinOpFactory {
    explicit every_second_row(std::shared_ptr<const gko::Executor> exec) : gko::LinOpFactory(std::move(exec)) {}
    std::unique_ptr<gko::LinOp> generate_impl(std::shared_ptr<const gko::LinOp> m) const override
    {
        const gko::size_type n = m->get_size()[0], rows = (n + 1) / 2;
        gko::array<gko::int32> coarse(exec_->get_master(), rows);
        for (gko::size_type i = 0; i < rows; ++i) coarse.get_data()[i] = static_cast<gko::int32>(2 * i);
        return coarsening::build().with_coarse_rows(coarse).on(exec_)->generate(m);
    }
};

template <typename Build>
static bool throws(Build build)
{
    try {
        build();
    } catch (const gko::NotSupported&) {
        return true;
    }
    return false;
}

static int validate()
{
    auto ref = gko::ReferenceExecutor::create();
    std::shared_ptr<const gko::LinOp> A = csr::create(ref, gko::dim<2>(100, 100));
    std::shared_ptr<const gko::LinOpFactory> level = std::make_shared<counting_level_factory>(ref);
    std::shared_ptr<const gko::LinOpFactory> smoother = std::make_shared<counting_factory>(ref, "pre");
    const auto one_cycle = [&] { return gko::stop::Iteration::build().with_max_iters(1u).on(ref); };
    int wrong = 0;
    wrong += !throws([&] { mg::build().with_criteria(one_cycle()).on(ref)->generate(A); });
    wrong += !throws([&] { mg::build().with_mg_level(level, nullptr).with_criteria(one_cycle()).on(ref)->generate(A); });
    wrong += !throws([&] { mg::build().with_mg_level(level, level, level).with_pre_smoother(smoother, smoother).with_criteria(one_cycle()).on(ref)->generate(A); });
    wrong += !throws([&] {
        mg::build().with_mg_level(level, level, level).with_post_uses_pre(false).with_post_smoother(smoother, smoother).with_criteria(one_cycle()).on(ref)->generate(A);
    });
    wrong += !throws([&] { mg::build().with_mg_level(level, level, level).with_mid_smoother(smoother, smoother).with_criteria(one_cycle()).on(ref)->generate(A); });
    // an unused list is not checked; a vector is taken as the list
    std::vector<std::shared_ptr<const gko::LinOpFactory>> three{level, level, level};
    top_rows = 100;
    auto ok = mg::build().with_mg_level(three).with_mid_case(mgns::mid_smooth_type::both).with_mid_smoother(smoother, smoother).with_max_levels(3u)
                  .with_min_coarse_rows(1u).with_criteria(one_cycle()).on(ref)->generate(A);
    wrong += ok->get_mg_level_list().size() != 3 || ok->get_cycle() != mgns::cycle::v || !ok->apply_uses_initial_guess();
    wrong += gko::solver::build_smoother<double>(smoother, 2u, 0.5)->generate(A)->get_relaxation_factor() != 0.5;
    std::printf(wrong ? "multigrid validate WRONG (%d)\n" : "multigrid validate ok\n", wrong);
    return wrong;
}

static double number(std::istream& in)
{
    std::string word;
    in >> word;
    return std::strtod(word.c_str(), nullptr);
}

template <typename T>
static std::vector<T> to_host(const gko::Executor* exec, const T* data, gko::size_type n)
{
    std::vector<T> out(n);
    exec->get_master()->copy_from(exec, n, data, out.data());
    return out;
}

// two Csr operators with the same size, row_ptrs, col_idxs and bits of the values
static bool same_csr(const gko::LinOp* a, const gko::LinOp* b)
{
    auto ca = dynamic_cast<const csr*>(a), cb = dynamic_cast<const csr*>(b);
    if (!ca || !cb || ca->get_size() != cb->get_size() || ca->get_num_stored_elements() != cb->get_num_stored_elements()) return false;
    const auto exec = ca->get_executor().get();
    const auto rows = ca->get_size()[0] + 1, nnz = ca->get_num_stored_elements();
    const auto va = to_host(exec, ca->get_const_values(), nnz), vb = to_host(exec, cb->get_const_values(), nnz);
    return to_host(exec, ca->get_const_row_ptrs(), rows) == to_host(exec, cb->get_const_row_ptrs(), rows) &&
           to_host(exec, ca->get_const_col_idxs(), nnz) == to_host(exec, cb->get_const_col_idxs(), nnz) &&
           (nnz == 0 || std::memcmp(va.data(), vb.data(), nnz * sizeof(double)) == 0);
}

// One apply of the smoother build_smoother makes (Ir over scalar Jacobi, one sweep, relaxation 0.9, provided guess) on the
// 5-point Poisson matrix of a g x g grid, through the fused sweep and through copy + SpMV + scalar_apply: a host clock
// around `reps` applies that end in a device synchronise, after a warm-up of both, 7 batches of each taking turns.
static void time_smoother(std::shared_ptr<const gko::Executor> exec, long g, int reps)
{
    const long n = g * g;
    std::vector<gko::int32> rp(n + 1, 0), ci;
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
    const long nnz = static_cast<long>(ci.size());
    auto A = gko::share(csr::create(exec, gko::dim<2>(n, n), nnz, std::make_shared<csr::merge_path>()));
    auto host = exec->get_master();
    exec->copy_from(host.get(), n + 1, rp.data(), A->get_row_ptrs());
    exec->copy_from(host.get(), nnz, ci.data(), A->get_col_idxs());
    exec->copy_from(host.get(), nnz, v.data(), A->get_values());
    auto jacobi = gko::share(gko::preconditioner::Jacobi<double, gko::int32>::build().with_max_block_size(1u).on(exec));
    auto smoother = gko::solver::build_smoother<double>(std::shared_ptr<const gko::LinOpFactory>(jacobi))->generate(A);
    auto b = dense::create(exec, gko::dim<2>(n, 1)), x = dense::create(exec, gko::dim<2>(n, 1));
    b->fill(1.0), x->fill(0.5);
    const char* paths[2] = {"1", "0"};
    std::vector<double> us[2];
    for (int batch = -1; batch < 7; ++batch) {   // batch -1 warms both paths up
        for (int p = 0; p < 2; ++p) {
            setenv("GKOMI_MG_FUSED", paths[p], 1);
            exec->synchronize();
            const auto t0 = std::chrono::steady_clock::now();
            for (int r = 0; r < reps; ++r) smoother->apply_with_initial_guess(b.get(), x.get(), gko::solver::initial_guess_mode::provided);
            exec->synchronize();
            const double t = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
            if (batch >= 0) us[p].push_back(t);
        }
    }
    unsetenv("GKOMI_MG_FUSED");
    std::sort(us[0].begin(), us[0].end()), std::sort(us[1].begin(), us[1].end());
    std::printf("| %ld | %ld | %.1f (%.1f .. %.1f) | %.1f (%.1f .. %.1f) | %.2f |\n", n, nnz, us[0][3], us[0].front(), us[0].back(), us[1][3],
                us[1].front(), us[1].back(), us[1][3] / us[0][3]);
    std::fflush(stdout);
}

int main(int argc, char** argv)
{
    if (argc < 2) return validate();
    auto exec = gko::HipExecutor::create(0, gko::ReferenceExecutor::create());
    if (std::string(argv[1]) == "time") {
        std::printf("| rows | nonzeros | fused sweep, us: median (min .. max) | copy + SpMV + scalar_apply, us | sequence / fused |\n|---|---|---|---|---|\n");
        for (long g : {16L, 64L, 256L, 512L, 640L, 768L, 896L, 1024L}) time_smoother(exec, g, 500);
        return 0;
    }
    std::string word, name;
    while (std::cin >> word) {
        if (word == "sequence") {
            std::string factory, cycle, mid, rest;
            gko::size_type max_levels = 0, rows = 0;
            std::cin >> name >> factory >> cycle >> max_levels >> mid >> rows;
            std::getline(std::cin, rest);
            const bool individual = factory == "individual";
            top_rows = rows;
            trace.clear();
            std::shared_ptr<const gko::LinOp> A = std::make_shared<counting_op>(exec, gko::dim<2>(rows, rows), "", false);
            std::shared_ptr<const gko::LinOpFactory> level = std::make_shared<counting_level_factory>(exec);
            std::shared_ptr<const gko::LinOpFactory> pre = std::make_shared<counting_factory>(exec, "pre");
            std::shared_ptr<const gko::LinOpFactory> mids = std::make_shared<counting_factory>(exec, "mid");
            std::shared_ptr<const gko::LinOpFactory> post = std::make_shared<counting_factory>(exec, "post");
            std::shared_ptr<const gko::LinOpFactory> coarsest = std::make_shared<counting_factory>(exec, "coarsest");
            auto builder = mg::build();
            builder.with_max_levels(max_levels).with_mg_level(level, level, level).with_pre_smoother(nullptr, pre, pre).with_post_uses_pre(!individual)
                .with_mid_case(mid == "both" ? mgns::mid_smooth_type::both : mid == "post_smoother" ? mgns::mid_smooth_type::post_smoother
                               : mid == "pre_smoother" ? mgns::mid_smooth_type::pre_smoother : mgns::mid_smooth_type::standalone)
                .with_cycle(cycle_of(cycle)).with_min_coarse_rows(1u).with_criteria(gko::stop::Iteration::build().with_max_iters(1u).on(exec));
            if (individual) {
                builder.with_mid_smoother(nullptr, nullptr, mids).with_post_smoother(post, nullptr, post);
            } else {
                builder.with_coarsest_solver(coarsest);
            }
            auto solver = builder.on(exec)->generate(A);
            if (rest.find_first_not_of(' ') != std::string::npos) solver->set_cycle(cycle_of(rest.substr(rest.find_first_not_of(' '), 1)));
            auto b = dense::create(exec, gko::dim<2>(rows, 1)), x = dense::create(exec, gko::dim<2>(rows, 1));
            b->fill(0.0), x->fill(0.0);
            solver->apply(b.get(), x.get());
            std::printf("%s trace", name.c_str());
            for (auto t : trace) {
                // the coarsest solver's level is the number of levels
                std::printf(" %s", t.c_str());
            }
            std::printf("\n");
        } else if (word == "solve") {
            std::string cycle;
            long n = 0, nnz = 0;
            std::cin >> name >> cycle >> n >> nnz;
            std::vector<gko::int32> rp(n + 1), ci(nnz);
            std::vector<double> v(nnz), hb(n), hx(n);
            for (auto& t : rp) std::cin >> t;
            for (auto& t : ci) std::cin >> t;
            for (auto& t : v) t = number(std::cin);
            for (auto& t : hb) t = number(std::cin);
            for (auto& t : hx) t = number(std::cin);
            if (!std::cin) return 3;
            auto A = gko::share(csr::create(exec, gko::dim<2>(n, n), nnz, std::make_shared<csr::merge_path>()));
            auto host = exec->get_master();
            exec->copy_from(host.get(), n + 1, rp.data(), A->get_row_ptrs());
            exec->copy_from(host.get(), nnz, ci.data(), A->get_col_idxs());
            exec->copy_from(host.get(), nnz, v.data(), A->get_values());
            auto b = dense::create(exec, gko::dim<2>(n, 1)), x = dense::create(exec, gko::dim<2>(n, 1));
            exec->copy_from(host.get(), n, hb.data(), b->get_values());
            exec->copy_from(host.get(), n, hx.data(), x->get_values());
            using lu = gko::experimental::factorization::Lu<double, gko::int32>;
            using direct = gko::experimental::solver::Direct<double, gko::int32>;
            auto solver = mg::build()
                              .with_mg_level(gko::share(std::make_shared<every_second_row>(exec)))
                              .with_pre_smoother(gko::share(gko::preconditioner::Jacobi<double, gko::int32>::build().with_max_block_size(1u).on(exec)))
                              .with_smoother_iters(2u)
                              .with_max_levels(2u)
                              .with_coarsest_solver(gko::share(direct::build().with_factorization(gko::share(lu::build().with_symmetric_sparsity(true).on(exec))).on(exec)))
                              .with_cycle(cycle_of(cycle))
                              .with_default_initial_guess(gko::solver::initial_guess_mode::zero)
                              .with_criteria(gko::stop::Iteration::build().with_max_iters(3u).on(exec))
                              .on(exec)
                              ->generate(A);
            solver->apply(b.get(), x.get());
            exec->synchronize();
            host->copy_from(exec.get(), n, x->get_const_values(), hx.data());
            std::printf("%s x %ld", name.c_str(), n);
            for (auto t : hx) std::printf(" %a", t);
            std::printf("\n%s levels %zu", name.c_str(), solver->get_mg_level_list().size());
            for (const auto& lvl : solver->get_mg_level_list()) std::printf(" %zu", static_cast<size_t>(lvl->get_coarse_op()->get_size()[0]));
            std::printf("\n%s iterations 1 %lld\n", name.c_str(), static_cast<long long>(solver->get_last_iteration_count()));
        } else if (word == "fbcsr") {
            long n = 0, nnz = 0;
            std::cin >> name >> n >> nnz;
            std::vector<gko::int32> rp(n + 1), ci(nnz);
            std::vector<double> v(nnz);
            for (auto& t : rp) std::cin >> t;
            for (auto& t : ci) std::cin >> t;
            for (auto& t : v) t = number(std::cin);
            if (!std::cin) return 3;
            auto A = gko::share(csr::create(exec, gko::dim<2>(n, n), nnz));
            auto host = exec->get_master();
            exec->copy_from(host.get(), n + 1, rp.data(), A->get_row_ptrs());
            exec->copy_from(host.get(), nnz, ci.data(), A->get_col_idxs());
            exec->copy_from(host.get(), nnz, v.data(), A->get_values());
            auto blocks = gko::share(gko::matrix::Fbcsr<double, gko::int32>::create(exec, 1));
            A->convert_to(blocks.get());
            every_second_row factory(exec);
            auto from_csr = factory.generate_impl(A), from_fbcsr = factory.generate_impl(blocks);
            auto a = dynamic_cast<const coarsening*>(from_csr.get()), f = dynamic_cast<const coarsening*>(from_fbcsr.get());
            // the converted Csr is the fine operator (fixed_coarsening.cpp:87); R, P and A_c are those of the Csr
            bool same = dynamic_cast<const csr*>(f->get_fine_op().get()) != nullptr && f->get_fine_op().get() != blocks.get();
            same = same && same_csr(a->get_fine_op().get(), f->get_fine_op().get()) && same_csr(a->get_restrict_op().get(), f->get_restrict_op().get()) &&
                   same_csr(a->get_prolong_op().get(), f->get_prolong_op().get()) && same_csr(a->get_coarse_op().get(), f->get_coarse_op().get());
            auto coo = gko::share(gko::matrix::Coo<double, gko::int32>::create(exec));
            A->convert_to(coo.get());
            const bool refused = throws([&] { factory.generate_impl(coo); });
            std::printf("%s fbcsr %s coo %s\n", name.c_str(), same ? "same" : "DIFFERENT", refused ? "refused" : "TAKEN");
        } else {
            return 2;
        }
    }
    return 0;
}
