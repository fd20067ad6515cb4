// Records what the reference executor computes for factorization::ParIct and for each kernel of one iteration:
// the source of tests/golden/par_ict_ref.json (tests/test_par_ict_reference.py turns the output into that
// fixture and, where the reference's objects are present, runs this program again and compares).  Our own
// program over the reference's public API and its kernel headers, like tools/par_ilut_ref_record.cpp; it is
// built against the objects that oracle/ref.mk leaves in oracle/_ref/obj, with that file's flags:
//
//   g++ -std=c++14 -O1 -fPIC -ffp-contract=off -pthread -w -Ioracle/_ref/include -I$GINKGO_REF/include
//       -I$GINKGO_REF tools/par_ict_ref_record.cpp $(find oracle/_ref/obj -name '*.o') -o par_ict_ref_record -lm
//
// Input (stdin), any number of times:   matrix <name> <n> <nnz>, then n + 1 row pointers, nnz column indices and
// nnz values (hexadecimal floats).  Output (stdout): one line per array, "<case> <what> <count> <items...>",
// values as hexadecimal floats:
//   generate  for approximate_select 0 / 1, fill_in_limit 0.75 / 1.2 / 2.0, iterations 1 ... 5: the number of
//             entries of L, and for 1 and 5 iterations the factor;
//   kernels   each kernel alone on the intermediate matrices of the first iteration at fill_in_limit 1.2.
#include <ginkgo/ginkgo.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "core/factorization/factorization_kernels.hpp"
#include "core/factorization/par_ict_kernels.hpp"
#include "core/factorization/par_ilut_kernels.hpp"

using csr = gko::matrix::Csr<double, gko::int32>;
using coo = gko::matrix::Coo<double, gko::int32>;
namespace ict = gko::kernels::reference::par_ict_factorization;
namespace ilut = gko::kernels::reference::par_ilut_factorization;

static void put_ints(const std::string& tag, const char* what, const gko::int32* p, size_t count)
{
    std::printf("%s %s %zu", tag.c_str(), what, count);
    for (size_t i = 0; i < count; ++i) std::printf(" %d", p[i]);
    std::printf("\n");
}

static void put_vals(const std::string& tag, const char* what, const double* p, size_t count)
{
    std::printf("%s %s %zu", tag.c_str(), what, count);
    for (size_t i = 0; i < count; ++i) std::printf(" %a", p[i]);
    std::printf("\n");
}

static void put_csr(const std::string& tag, const std::string& name, const csr* m)
{
    put_ints(tag, (name + ".row_ptrs").c_str(), m->get_const_row_ptrs(), m->get_size()[0] + 1);
    put_ints(tag, (name + ".col_idxs").c_str(), m->get_const_col_idxs(), m->get_num_stored_elements());
    put_vals(tag, (name + ".vals").c_str(), m->get_const_values(), m->get_num_stored_elements());
}

int main()
{
    auto ref = gko::ReferenceExecutor::create();
    std::string word, name;
    while (std::cin >> word) {
        if (word != "matrix") return 2;
        long n = 0, nnz = 0;
        std::cin >> name >> n >> nnz;
        gko::array<gko::int32> rp(ref, n + 1), ci(ref, nnz);
        gko::array<double> v(ref, nnz);
        for (long i = 0; i <= n; ++i) std::cin >> rp.get_data()[i];
        for (long i = 0; i < nnz; ++i) std::cin >> ci.get_data()[i];
        for (long i = 0; i < nnz; ++i) {
            std::cin >> word;
            v.get_data()[i] = std::strtod(word.c_str(), nullptr);
        }
        if (!std::cin) return 3;
        const gko::dim<2> size(n, n);
        auto a = gko::share(csr::create(ref, size, std::move(v), std::move(ci), std::move(rp)));

        for (int approx = 0; approx < 2; ++approx) {
            for (double limit : {0.75, 1.2, 2.0}) {
                for (unsigned iterations = 1; iterations <= 5; ++iterations) {
                    auto fact = gko::factorization::ParIct<double, gko::int32>::build()
                                    .with_iterations(iterations)
                                    .with_fill_in_limit(limit)
                                    .with_approximate_select(approx != 0)
                                    .on(ref)
                                    ->generate(a);
                    char tag[256];
                    std::snprintf(tag, sizeof(tag), "%s generate/%s/%g/%u", name.c_str(), approx ? "approx" : "exact", limit,
                                  iterations);
                    const gko::int32 count = static_cast<gko::int32>(fact->get_l_factor()->get_num_stored_elements());
                    put_ints(tag, "nnz", &count, 1);
                    if (iterations != 1 && iterations != 5) continue;
                    put_csr(tag, "l", fact->get_l_factor().get());
                }
            }
        }

        // the first iteration of core/factorization/par_ict.cpp:228-292, kernel by kernel
        const std::string tag = name + " kernels";
        gko::array<gko::int32> l_rp(ref, n + 1);
        gko::kernels::reference::factorization::initialize_row_ptrs_l(ref, a.get(), l_rp.get_data());
        const size_t l_nnz = l_rp.get_data()[n];
        auto l = csr::create(ref, size, gko::array<double>(ref, l_nnz), gko::array<gko::int32>(ref, l_nnz), std::move(l_rp));
        gko::kernels::reference::factorization::initialize_l(ref, a.get(), l.get(), true);
        put_csr(tag, "initialize_l", l.get());
        const gko::int32 l_limit = static_cast<gko::int32>(l_nnz * 1.2);
        auto lh = gko::as<csr>(l->conj_transpose());
        auto llh = csr::create(ref, size);
        l->apply(lh.get(), llh.get());
        put_csr(tag, "llh", llh.get());
        auto l_new = csr::create(ref, size);
        ict::add_candidates(ref, llh.get(), a.get(), l.get(), l_new.get());
        put_csr(tag, "add_candidates", l_new.get());
        const coo* no_coo = nullptr;
        ict::compute_factor(ref, a.get(), l_new.get(), no_coo);
        put_csr(tag, "sweep", l_new.get());
        const gko::int32 ln = static_cast<gko::int32>(l_new->get_num_stored_elements());
        const gko::int32 rank = std::max<gko::int32>(0, ln - l_limit - 1);
        put_ints(tag, "ranks", &rank, 1);
        gko::array<double> tmp(ref), tmp2(ref);
        double select = 0.0, approx = 0.0;
        ilut::threshold_select(ref, l_new.get(), rank, tmp, tmp2, select);
        put_vals(tag, "select", &select, 1);
        coo* null_coo = nullptr;
        auto l_f = csr::create(ref, size);
        ilut::threshold_filter(ref, l_new.get(), select, l_f.get(), null_coo, true);
        put_csr(tag, "filter", l_f.get());
        auto l_a = csr::create(ref, size);
        ilut::threshold_filter_approx(ref, l_new.get(), rank, tmp, approx, l_a.get(), null_coo);
        put_vals(tag, "approx", &approx, 1);
        put_csr(tag, "filter_approx", l_a.get());
        ict::compute_factor(ref, a.get(), l_f.get(), no_coo);
        put_csr(tag, "second_sweep", l_f.get());
    }
    return 0;
}
