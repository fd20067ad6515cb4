// Records what the reference executor computes for preconditioner::Isai and for its kernels: the source of
// tests/golden/isai_ref.json (tests/test_isai_reference.py turns the output into that fixture and, where the
// reference's objects are present, runs this program again and compares).  Our own program over the reference's
// public API and its kernel headers, like tools/par_ict_ref_record.cpp; it is built against the objects that
// oracle/ref.mk leaves in oracle/_ref/obj, with that file's flags:
//
//   g++ -std=c++14 -O1 -fPIC -ffp-contract=off -pthread -w -Ioracle/_ref/include -I$GINKGO_REF/include
//       -I$GINKGO_REF tools/isai_ref_record.cpp $(find oracle/_ref/obj -name '*.o') -o isai_ref_record -lm
//
// Input (stdin), any number of times:   case <name> <kind> <sparsity_power> <excess_limit> <n> <nnz>, kind one of
// lower upper general spd, then n + 1 row pointers, nnz column indices and nnz values (hexadecimal floats).
// Output (stdout): one line per array, "<case> <section> <what> <count> <items...>", values as hexadecimal floats:
//   generate  the approximate inverse of Isai::generate (for spd: L, the second operator of the composition);
//   kernel    generate_tri_inverse / generate_general_inverse alone on that pattern with zeroed values: the matrix
//             (long rows stay zero), both prefix arrays, counts = { rows over the limit, their entries, longest row,
//             blocks of the excess loop };
//   excess/b  generate_excess_system of block b of the loop over excess_limit: its row range, system and rhs.
// The counts also go to stderr, one line per case.
#include <ginkgo/ginkgo.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "core/preconditioner/isai_kernels.hpp"

using csr = gko::matrix::Csr<double, gko::int32>;
using dense = gko::matrix::Dense<double>;
namespace isai = gko::kernels::reference::isai;
using gko::preconditioner::isai_type;

static void put_ints(const std::string& tag, const std::string& what, const gko::int32* p, size_t count)
{
    std::printf("%s %s %zu", tag.c_str(), what.c_str(), count);
    for (size_t i = 0; i < count; ++i) std::printf(" %d", p[i]);
    std::printf("\n");
}

static void put_vals(const std::string& tag, const std::string& what, const double* p, size_t count)
{
    std::printf("%s %s %zu", tag.c_str(), what.c_str(), count);
    for (size_t i = 0; i < count; ++i) std::printf(" %a", p[i]);
    std::printf("\n");
}

static void put_csr(const std::string& tag, const std::string& name, const csr* m)
{
    put_ints(tag, name + ".row_ptrs", m->get_const_row_ptrs(), m->get_size()[0] + 1);
    put_ints(tag, name + ".col_idxs", m->get_const_col_idxs(), m->get_num_stored_elements());
    put_vals(tag, name + ".vals", m->get_const_values(), m->get_num_stored_elements());
}

template <isai_type Type>
static std::shared_ptr<const csr> generate(std::shared_ptr<const gko::Executor> ref, std::shared_ptr<csr> a, int power,
                                           long limit)
{
    auto pre = gko::preconditioner::Isai<Type, double, gko::int32>::build()
                   .with_sparsity_power(power)
                   .with_excess_limit(static_cast<gko::size_type>(limit))
                   .on(ref)
                   ->generate(a);
    return pre->get_approximate_inverse();
}

template <>
std::shared_ptr<const csr> generate<isai_type::spd>(std::shared_ptr<const gko::Executor> ref, std::shared_ptr<csr> a,
                                                    int power, long limit)
{
    auto pre = gko::preconditioner::Isai<isai_type::spd, double, gko::int32>::build()
                   .with_sparsity_power(power)
                   .with_excess_limit(static_cast<gko::size_type>(limit))
                   .on(ref)
                   ->generate(a);
    return gko::as<const csr>(pre->get_approximate_inverse()->get_operators()[1]);
}

int main()
{
    auto ref = gko::ReferenceExecutor::create();
    std::string word, name, kind;
    while (std::cin >> word) {
        if (word != "case") return 2;
        long n = 0, nnz = 0, limit = 0;
        int power = 1;
        std::cin >> name >> kind >> power >> limit >> n >> nnz;
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
        a->sort_by_column_index();
        const bool tri = kind == "lower" || kind == "upper";
        std::shared_ptr<const csr> inverse;
        if (kind == "lower") {
            inverse = generate<isai_type::lower>(ref, a, power, limit);
        } else if (kind == "upper") {
            inverse = generate<isai_type::upper>(ref, a, power, limit);
        } else if (kind == "general") {
            inverse = generate<isai_type::general>(ref, a, power, limit);
        } else if (kind == "spd") {
            inverse = generate<isai_type::spd>(ref, a, power, limit);
        } else {
            return 4;
        }

        // the kernel alone, on the pattern with zeroed values
        auto direct = inverse->clone();
        std::fill_n(direct->get_values(), direct->get_num_stored_elements(), 0.0);
        gko::array<gko::int32> rhs_ptrs(ref, n + 1), nz_ptrs(ref, n + 1);
        if (tri) {
            isai::generate_tri_inverse(ref, a.get(), direct.get(), rhs_ptrs.get_data(), nz_ptrs.get_data(), kind == "lower");
        } else {
            isai::generate_general_inverse(ref, a.get(), direct.get(), rhs_ptrs.get_data(), nz_ptrs.get_data(), kind == "spd");
        }
        gko::int32 counts[4] = {0, 0, 0, 0};
        for (long row = 0; row < n; ++row) {
            const gko::int32 len = direct->get_const_row_ptrs()[row + 1] - direct->get_const_row_ptrs()[row];
            counts[2] = std::max(counts[2], len);
            if (len > isai::row_size_limit) {
                ++counts[0];
                counts[1] += len;
            }
        }
        // an inverse whose long rows went through the iterative default solver is not reproducible bit for bit
        if (tri || counts[0] == 0) put_csr(name + " generate", "inverse", inverse.get());
        put_csr(name + " kernel", "direct", direct.get());
        put_ints(name + " kernel", "excess_rhs_ptrs", rhs_ptrs.get_const_data(), n + 1);
        put_ints(name + " kernel", "excess_nz_ptrs", nz_ptrs.get_const_data(), n + 1);

        // the block loop of core/preconditioner/isai.cpp:191-221
        const auto* host_rhs = rhs_ptrs.get_const_data();
        const auto* host_nz = nz_ptrs.get_const_data();
        const long total = host_rhs[n];
        const long lim = limit == 0 ? total : limit;
        long block = 0;
        while (total > 0 && block < n) {
            const long start = block;
            long dim = 0;
            for (; dim < lim && block < n; dim = host_rhs[block] - host_rhs[start]) ++block;
            if (dim == 0) break;
            const long e_nnz = host_nz[block] - host_nz[start];
            auto system = csr::create(ref, gko::dim<2>(dim, dim), e_nnz);
            auto rhs = dense::create(ref, gko::dim<2>(dim, 1));
            isai::generate_excess_system(ref, a.get(), direct.get(), host_rhs, host_nz, system.get(), rhs.get(), start, block);
            const std::string tag = name + " excess/" + std::to_string(counts[3]);
            const gko::int32 range[2] = {static_cast<gko::int32>(start), static_cast<gko::int32>(block)};
            put_ints(tag, "range", range, 2);
            put_csr(tag, "system", system.get());
            put_vals(tag, "rhs_vals", rhs->get_const_values(), dim);
            ++counts[3];
        }
        put_ints(name + " kernel", "counts", counts, 4);
        std::fprintf(stderr, "%s: %d rows over the limit with %d entries, longest row %d, %d blocks\n", name.c_str(), counts[0],
                     counts[1], counts[2], counts[3]);
    }
    return 0;
}
