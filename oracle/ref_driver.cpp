// ref_driver -- TEST INFRASTRUCTURE ONLY.
//
// Runs batches of cases on the reference library's ReferenceExecutor through
// its public API, so that the tests can compare the C oracle, the Python
// restatements and the HIP kernels with the reference itself instead of with
// a restatement of it.  The verbs that pin a single kernel (par_ilut, par_ict,
// isai, cb_gmres, multigrid) call gko::kernels::reference::... directly and
// include that kernel's core/**/*_kernels.hpp for it.  This file is the
// project's own; it is compiled against the reference's headers by
// oracle/ref.mk into oracle/_ref/ and the product never links or loads it.
//
//   ref_driver IN OUT
//
// IN:  "GKRI", u32 ncases, then per case
//        str verb, u32 nparams x (str name, f64 value),
//        u32 narrays x (str name, u8 dtype, u64 count, raw bytes)
// OUT: "GKRO", u32 ncases, then per case
//        u32 status (0 ok, 1 failed), str message, u32 narrays x (as above)
// str = u32 length + bytes; dtype 0 f64, 1 f32, 2 i32, 3 i64, 4 u8.  Values
// travel as raw IEEE bytes both ways (tests/ref_exec.py is the other end).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <ginkgo/ginkgo.hpp>

#include "core/factorization/factorization_kernels.hpp"
#include "core/factorization/par_ict_kernels.hpp"
#include "core/factorization/par_ilut_kernels.hpp"
#include "core/preconditioner/isai_kernels.hpp"
#include "core/solver/cb_gmres_accessor.hpp"
#include "core/solver/cb_gmres_kernels.hpp"
#include "core/solver/multigrid_kernels.hpp"

namespace {

using gko::dim;
using gko::size_type;

template <typename T> struct dt;
template <> struct dt<double> { static const int code = 0; };
template <> struct dt<float> { static const int code = 1; };
template <> struct dt<gko::int32> { static const int code = 2; };
template <> struct dt<gko::int64> { static const int code = 3; };
template <> struct dt<gko::uint8> { static const int code = 4; };
const size_t dt_size[] = {8, 4, 4, 8, 1};

struct Arr {
    int code;
    std::vector<char> bytes;
    size_t count() const { return bytes.size() / dt_size[code]; }
};

struct Case {
    std::string verb;
    std::map<std::string, double> params;
    std::map<std::string, Arr> in;
    std::vector<std::pair<std::string, Arr>> out;

    bool has(const std::string& n) const { return params.count(n) != 0; }
    double p(const std::string& n) const
    {
        auto it = params.find(n);
        if (it == params.end()) throw std::runtime_error("missing parameter " + n);
        return it->second;
    }
    double p(const std::string& n, double dflt) const { return has(n) ? p(n) : dflt; }
    long pi(const std::string& n) const { return static_cast<long>(p(n)); }
    long pi(const std::string& n, long dflt) const { return has(n) ? pi(n) : dflt; }

    template <typename T>
    const T* arr(const std::string& n, size_t* count = nullptr) const
    {
        auto it = in.find(n);
        if (it == in.end()) throw std::runtime_error("missing array " + n);
        if (it->second.code != dt<T>::code) throw std::runtime_error("array " + n + " has the wrong dtype");
        if (count) *count = it->second.count();
        return reinterpret_cast<const T*>(it->second.bytes.data());
    }
    template <typename T>
    void put(const std::string& n, const T* data, size_t count)
    {
        Arr a;
        a.code = dt<T>::code;
        a.bytes.resize(count * sizeof(T));
        if (count) std::memcpy(a.bytes.data(), data, count * sizeof(T));
        out.emplace_back(n, std::move(a));
    }
    template <typename T>
    void put_scalar(const std::string& n, T v) { put(n, &v, 1); }
};

std::shared_ptr<gko::ReferenceExecutor> exec;

template <typename T>
gko::array<T> in_array(const Case& c, const std::string& n)
{
    size_t cnt;
    const T* d = c.arr<T>(n, &cnt);
    gko::array<T> a(exec, cnt);
    if (cnt) std::memcpy(a.get_data(), d, cnt * sizeof(T));
    return a;
}

// Csr from <pre>rp, <pre>ci, <pre>v and the parameters <pre>m, <pre>n
template <typename V, typename I>
std::unique_ptr<gko::matrix::Csr<V, I>> in_csr(const Case& c, const std::string& pre = "")
{
    return gko::matrix::Csr<V, I>::create(
        exec, dim<2>(c.pi(pre + "m"), c.pi(pre + "n")), in_array<V>(c, pre + "v"),
        in_array<I>(c, pre + "ci"), in_array<I>(c, pre + "rp"));
}

template <typename V, typename I>
void out_csr(Case& c, const std::string& pre, const gko::matrix::Csr<V, I>* m)
{
    c.put(pre + "rp", m->get_const_row_ptrs(), m->get_size()[0] + 1);
    c.put(pre + "ci", m->get_const_col_idxs(), m->get_num_stored_elements());
    c.put(pre + "v", m->get_const_values(), m->get_num_stored_elements());
    gko::int64 sz[2] = {static_cast<gko::int64>(m->get_size()[0]), static_cast<gko::int64>(m->get_size()[1])};
    c.put(pre + "size", sz, 2);
}

// Dense from the array <n> (rows x stride, padding included) and the
// parameters <n>_rows, <n>_cols, <n>_stride
template <typename V>
std::unique_ptr<gko::matrix::Dense<V>> in_dense(const Case& c, const std::string& n)
{
    size_type rows = c.pi(n + "_rows"), cols = c.pi(n + "_cols");
    size_type stride = c.pi(n + "_stride", cols);
    auto a = in_array<V>(c, n);
    if (a.get_num_elems() != rows * stride) throw std::runtime_error("dense " + n + ": size is not rows*stride");
    return gko::matrix::Dense<V>::create(exec, dim<2>(rows, cols), std::move(a), stride);
}

// the whole buffer goes back, so the tests also see that padding is untouched
template <typename V>
void out_dense(Case& c, const std::string& n, const gko::matrix::Dense<V>* d)
{
    c.put(n, d->get_const_values(), d->get_num_stored_elements());
}

template <typename V>
std::unique_ptr<gko::matrix::Dense<V>> scalar(V v)
{
    return gko::initialize<gko::matrix::Dense<V>>({v}, exec);
}

// ---- the storage formats, reached from a Csr by the reference's conversions

enum { F_CSR, F_ELL, F_SELLP, F_HYBRID, F_COO, F_FBCSR, F_DENSE };
// the words of the cases as numbers: WORDS of tests/ref_exec.py has each list in the same order.  (The storage of
// cb_gmres is the reference's own solver::cb_gmres::storage_precision.)
enum { BASE_RHS_NORM, BASE_INITIAL_RESNORM, BASE_ABSOLUTE };   // the baseline of a residual-norm criterion
enum { ISAI_LOWER, ISAI_UPPER, ISAI_GENERAL, ISAI_SPD };
enum { CYCLE_V, CYCLE_F, CYCLE_W };
enum { MID_BOTH, MID_POST_SMOOTHER, MID_PRE_SMOOTHER, MID_STANDALONE };
enum { COARSEST_IDENTITY, COARSEST_DIRECT, COARSEST_CG };
enum { GUESS_ZERO, GUESS_RHS, GUESS_PROVIDED };
enum { SMOOTHER_NULL, SMOOTHER_EYE, SMOOTHER_JACOBI };
enum { LEVEL_HALVE, LEVEL_ALL_ROWS, LEVEL_PGM };

template <typename V, typename I>
std::unique_ptr<gko::LinOp> to_format(const Case& c, const gko::matrix::Csr<V, I>* csr)
{
    using namespace gko::matrix;
    switch (c.pi("fmt")) {
    case F_CSR: return csr->clone();
    case F_ELL: {
        auto r = Ell<V, I>::create(exec);
        csr->convert_to(r.get());
        return std::move(r);
    }
    case F_SELLP: {
        auto r = Sellp<V, I>::create(exec, dim<2>{}, c.pi("slice_size", default_slice_size),
                                     c.pi("stride_factor", default_stride_factor), 0);
        csr->convert_to(r.get());
        return std::move(r);
    }
    case F_HYBRID: {
        using H = Hybrid<V, I>;
        std::shared_ptr<typename H::strategy_type> s;
        switch (c.pi("hyb_strategy", 0)) {
        case 0: s = std::make_shared<typename H::automatic>(); break;
        case 1: s = std::make_shared<typename H::column_limit>(c.pi("hyb_columns")); break;
        case 2: s = std::make_shared<typename H::imbalance_limit>(c.p("hyb_percent")); break;
        case 3: s = std::make_shared<typename H::imbalance_bounded_limit>(c.p("hyb_percent"), c.p("hyb_ratio")); break;
        default: throw std::runtime_error("unknown hybrid strategy");
        }
        auto r = H::create(exec, s);
        csr->convert_to(r.get());
        return std::move(r);
    }
    case F_COO: {
        auto r = Coo<V, I>::create(exec);
        csr->convert_to(r.get());
        return std::move(r);
    }
    case F_FBCSR: {
        auto r = Fbcsr<V, I>::create(exec, static_cast<int>(c.pi("bs")));
        csr->convert_to(r.get());
        return std::move(r);
    }
    case F_DENSE: {
        auto r = Dense<V>::create(exec);
        csr->convert_to(r.get());
        return std::move(r);
    }
    }
    throw std::runtime_error("unknown format");
}

template <typename V, typename I>
void out_ell(Case& c, const std::string& pre, const gko::matrix::Ell<V, I>* m)
{
    c.put(pre + "v", m->get_const_values(), m->get_num_stored_elements());
    c.put(pre + "ci", m->get_const_col_idxs(), m->get_num_stored_elements());
    gko::int64 meta[2] = {static_cast<gko::int64>(m->get_num_stored_elements_per_row()),
                          static_cast<gko::int64>(m->get_stride())};
    c.put(pre + "meta", meta, 2);
}

template <typename V, typename I>
void out_coo(Case& c, const std::string& pre, const gko::matrix::Coo<V, I>* m)
{
    c.put(pre + "v", m->get_const_values(), m->get_num_stored_elements());
    c.put(pre + "ri", m->get_const_row_idxs(), m->get_num_stored_elements());
    c.put(pre + "ci", m->get_const_col_idxs(), m->get_num_stored_elements());
}

template <typename V, typename I>
void out_format(Case& c, const gko::LinOp* op)
{
    using namespace gko::matrix;
    if (auto m = dynamic_cast<const Csr<V, I>*>(op)) {
        out_csr(c, "f_", m);
    } else if (auto m = dynamic_cast<const Ell<V, I>*>(op)) {
        out_ell(c, "ell_", m);
    } else if (auto m = dynamic_cast<const Sellp<V, I>*>(op)) {
        size_type slices = gko::ceildiv(m->get_size()[0], m->get_slice_size());
        c.put("sellp_v", m->get_const_values(), m->get_num_stored_elements());
        c.put("sellp_ci", m->get_const_col_idxs(), m->get_num_stored_elements());
        std::vector<gko::int64> len(m->get_const_slice_lengths(), m->get_const_slice_lengths() + slices);
        std::vector<gko::int64> set(m->get_const_slice_sets(), m->get_const_slice_sets() + slices + 1);
        c.put("sellp_len", len.data(), len.size());
        c.put("sellp_set", set.data(), set.size());
    } else if (auto m = dynamic_cast<const Hybrid<V, I>*>(op)) {
        out_ell(c, "ell_", m->get_ell());
        out_coo(c, "coo_", m->get_coo());
    } else if (auto m = dynamic_cast<const Coo<V, I>*>(op)) {
        out_coo(c, "coo_", m);
    } else if (auto m = dynamic_cast<const Fbcsr<V, I>*>(op)) {
        int bs = m->get_block_size();
        c.put("fb_v", m->get_const_values(), m->get_num_stored_elements());
        c.put("fb_ci", m->get_const_col_idxs(), m->get_num_stored_blocks());
        c.put("fb_rp", m->get_const_row_ptrs(), m->get_size()[0] / bs + 1);
    } else if (auto m = dynamic_cast<const Dense<V>*>(op)) {
        out_dense(c, "dense_v", m);
    } else {
        throw std::runtime_error("format without an output rule");
    }
}

// spmv: mode 0 apply, 1 advanced apply, 2 apply2, 3 advanced apply2 (Coo only)
template <typename V, typename I>
void v_spmv(Case& c)
{
    auto csr = in_csr<V, I>(c);
    auto A = to_format<V, I>(c, csr.get());
    auto b = in_dense<V>(c, "b");
    auto x = in_dense<V>(c, "x");
    long mode = c.pi("mode");
    auto alpha = scalar<V>(static_cast<V>(c.p("alpha", 1.0)));
    auto beta = scalar<V>(static_cast<V>(c.p("beta", 0.0)));
    if (mode == 0) {
        A->apply(b.get(), x.get());
    } else if (mode == 1) {
        A->apply(alpha.get(), b.get(), beta.get(), x.get());
    } else {
        auto coo = dynamic_cast<gko::matrix::Coo<V, I>*>(A.get());
        if (!coo) throw std::runtime_error("apply2 is a Coo operation");
        if (mode == 2) {
            coo->apply2(b.get(), x.get());
        } else {
            coo->apply2(alpha.get(), b.get(), x.get());
        }
    }
    out_dense(c, "x", x.get());
}

// convert: Csr -> format (returned) -> Csr (returned as back_*)
template <typename V, typename I>
void v_convert(Case& c)
{
    auto csr = in_csr<V, I>(c);
    auto A = to_format<V, I>(c, csr.get());
    out_format<V, I>(c, A.get());
    auto back = gko::matrix::Csr<V, I>::create(exec);
    gko::as<gko::ConvertibleTo<gko::matrix::Csr<V, I>>>(A.get())->convert_to(back.get());
    out_csr(c, "back_", back.get());
}

// fbcsr_op on an Fbcsr given by its own arrays (bs, rp, ci, v): 0 transpose,
// 1 sort_by_column_index, 2 is_sorted_by_column_index, 3 extract_diagonal,
// 4 to Csr, 5 to Dense, 6 apply, 7 advanced apply
template <typename V, typename I>
void v_fbcsr_op(Case& c)
{
    using F = gko::matrix::Fbcsr<V, I>;
    auto A = F::create(exec, dim<2>(c.pi("m"), c.pi("n")), static_cast<int>(c.pi("bs")), in_array<V>(c, "v"),
                       in_array<I>(c, "ci"), in_array<I>(c, "rp"));
    switch (c.pi("op")) {
    case 0: out_format<V, I>(c, A->transpose().get()); break;
    case 1:
        A->sort_by_column_index();
        out_format<V, I>(c, A.get());
        break;
    case 2: c.put_scalar<gko::int64>("sorted", A->is_sorted_by_column_index()); break;
    case 3: {
        auto d = A->extract_diagonal();
        c.put("diag", d->get_const_values(), d->get_size()[0]);
        break;
    }
    case 4: {
        auto r = gko::matrix::Csr<V, I>::create(exec);
        A->convert_to(r.get());
        out_csr(c, "back_", r.get());
        break;
    }
    case 5: {
        auto r = gko::matrix::Dense<V>::create(exec);
        A->convert_to(r.get());
        out_dense(c, "dense_v", r.get());
        break;
    }
    case 6:
    case 7: {
        auto b = in_dense<V>(c, "b");
        auto x = in_dense<V>(c, "x");
        if (c.pi("op") == 6) {
            A->apply(b.get(), x.get());
        } else {
            A->apply(scalar<V>(c.p("alpha")).get(), b.get(), scalar<V>(c.p("beta")).get(), x.get());
        }
        out_dense(c, "x", x.get());
        break;
    }
    default: throw std::runtime_error("unknown fbcsr op");
    }
}

template <typename V, typename I>
void v_csr_op(Case& c)
{
    auto csr = in_csr<V, I>(c);
    switch (c.pi("op")) {
    case 0: {
        auto t = gko::as<gko::matrix::Csr<V, I>>(csr->transpose());
        out_csr(c, "", t.get());
        break;
    }
    case 1:
        csr->sort_by_column_index();
        out_csr(c, "", csr.get());
        break;
    case 2:
        c.put_scalar<gko::int64>("sorted", csr->is_sorted_by_column_index());
        break;
    case 3: {
        auto d = csr->extract_diagonal();
        c.put("diag", d->get_const_values(), d->get_size()[0]);
        break;
    }
    default: throw std::runtime_error("unknown csr op");
    }
}

// device_matrix_data: op 0 sum_duplicates, 1 remove_zeros, 2 sort_row_major
template <typename V, typename I>
void v_mdata(Case& c)
{
    gko::device_matrix_data<V, I> d(exec, dim<2>(c.pi("m"), c.pi("n")), in_array<I>(c, "ri"),
                                    in_array<I>(c, "ci"), in_array<V>(c, "v"));
    switch (c.pi("op")) {
    case 0: d.sum_duplicates(); break;
    case 1: d.remove_zeros(); break;
    case 2: d.sort_row_major(); break;
    default: throw std::runtime_error("unknown matrix data op");
    }
    c.put("ri", d.get_const_row_idxs(), d.get_num_elems());
    c.put("ci", d.get_const_col_idxs(), d.get_num_elems());
    c.put("v", d.get_const_values(), d.get_num_elems());
}

// Csr x Csr: mode 0 C = A B; 1 C = alpha A B + beta C; 2 C = alpha A I + beta C
template <typename V, typename I>
void v_spgemm(Case& c)
{
    auto A = in_csr<V, I>(c, "a_");
    long mode = c.pi("mode");
    auto alpha = scalar<V>(static_cast<V>(c.p("alpha", 1.0)));
    auto beta = scalar<V>(static_cast<V>(c.p("beta", 0.0)));
    if (mode == 0) {
        auto B = in_csr<V, I>(c, "b_");
        auto C = gko::matrix::Csr<V, I>::create(exec, dim<2>(A->get_size()[0], B->get_size()[1]));
        A->apply(B.get(), C.get());
        out_csr(c, "c_", C.get());
    } else if (mode == 1) {
        auto B = in_csr<V, I>(c, "b_");
        auto C = in_csr<V, I>(c, "c_");
        A->apply(alpha.get(), B.get(), beta.get(), C.get());
        out_csr(c, "c_", C.get());
    } else {
        auto Id = gko::matrix::Identity<V>::create(exec, A->get_size()[1]);
        auto C = in_csr<V, I>(c, "c_");
        A->apply(alpha.get(), Id.get(), beta.get(), C.get());
        out_csr(c, "c_", C.get());
    }
}

// Dense BLAS-1: x is the operand that is changed or reduced; op 0 scale, 1 inv_scale, 2 add_scaled, 3 sub_scaled,
// 4 compute_dot, 5 compute_norm2, 6 compute_norm1, 7 fill, 8 copy_from, 9 row_gather
template <typename V>
void v_dense(Case& c)
{
    using D = gko::matrix::Dense<V>;
    auto x = in_dense<V>(c, "x");
    long op = c.pi("op");
    size_type cols = x->get_size()[1];
    if (op == 7) {   // fill
        x->fill(static_cast<V>(c.p("value")));
        out_dense(c, "x", x.get());
    } else if (op == 8) {   // copy_from a Dense of another stride
        x->copy_from(in_dense<V>(c, "y").get());
        out_dense(c, "x", x.get());
    } else if (op == 9) {   // x = rows of y
        auto idx = in_array<gko::int32>(c, "rows");
        in_dense<V>(c, "y")->row_gather(&idx, x.get());
        out_dense(c, "x", x.get());
    } else if (op <= 3) {
        auto alpha = in_dense<V>(c, "alpha");
        switch (op) {
        case 0: x->scale(alpha.get()); break;
        case 1: x->inv_scale(alpha.get()); break;
        case 2: x->add_scaled(alpha.get(), in_dense<V>(c, "y").get()); break;
        case 3: x->sub_scaled(alpha.get(), in_dense<V>(c, "y").get()); break;
        }
        out_dense(c, "x", x.get());
    } else {
        auto r = D::create(exec, dim<2>(1, cols));
        switch (op) {
        case 4: x->compute_dot(in_dense<V>(c, "y").get(), r.get()); break;
        case 5: x->compute_norm2(r.get()); break;
        case 6: x->compute_norm1(r.get()); break;
        default: throw std::runtime_error("unknown dense op");
        }
        out_dense(c, "r", r.get());
    }
}

// factor: kind 0 ParIlu, 1 ParIc, 2 Ilu, 3 Ic, 4 Lu (the combined factor: its pattern is the symbolic result)
template <typename V, typename I>
void v_factor(Case& c)
{
    using Csr = gko::matrix::Csr<V, I>;
    std::shared_ptr<Csr> A = in_csr<V, I>(c);
    bool skip = c.pi("skip_sorting", 0) != 0;
    switch (c.pi("kind")) {
    case 0: {
        auto f = gko::factorization::ParIlu<V, I>::build().with_iterations(c.pi("iterations")).with_skip_sorting(skip).on(exec)->generate(A);
        out_csr(c, "l_", f->get_l_factor().get());
        out_csr(c, "u_", f->get_u_factor().get());
        break;
    }
    case 1: {
        auto f = gko::factorization::ParIc<V, I>::build().with_iterations(c.pi("iterations")).with_skip_sorting(skip).on(exec)->generate(A);
        out_csr(c, "l_", f->get_l_factor().get());
        out_csr(c, "u_", f->get_lt_factor().get());
        break;
    }
    case 2: {
        auto f = gko::factorization::Ilu<V, I>::build().with_skip_sorting(skip).on(exec)->generate(A);
        out_csr(c, "l_", f->get_l_factor().get());
        out_csr(c, "u_", f->get_u_factor().get());
        break;
    }
    case 3: {
        auto f = gko::factorization::Ic<V, I>::build().with_skip_sorting(skip).on(exec)->generate(A);
        out_csr(c, "l_", f->get_l_factor().get());
        out_csr(c, "u_", f->get_lt_factor().get());
        break;
    }
    case 4: {
        auto f = gko::experimental::factorization::Lu<V, I>::build()
                     .with_symmetric_sparsity(c.pi("symmetric", 0) != 0).with_skip_sorting(skip).on(exec)->generate(A);
        out_csr(c, "lu_", f->get_combined().get());
        break;
    }
    default: throw std::runtime_error("unknown factorization");
    }
}

template <typename V, typename I>
void v_direct(Case& c)
{
    std::shared_ptr<gko::matrix::Csr<V, I>> A = in_csr<V, I>(c);
    auto b = in_dense<V>(c, "b");
    auto x = in_dense<V>(c, "x");
    auto s = gko::experimental::solver::Direct<V, I>::build()
                 .with_factorization(gko::experimental::factorization::Lu<V, I>::build()
                                         .with_symmetric_sparsity(c.pi("symmetric", 0) != 0).on(exec))
                 .with_num_rhs(b->get_size()[1]).on(exec)->generate(A);
    s->apply(b.get(), x.get());
    out_dense(c, "x", x.get());
}

// trs: upper 0/1, unit_diagonal 0/1
template <typename V, typename I>
void v_trs(Case& c)
{
    std::shared_ptr<gko::matrix::Csr<V, I>> A = in_csr<V, I>(c);
    auto b = in_dense<V>(c, "b");
    auto x = in_dense<V>(c, "x");
    bool unit = c.pi("unit_diagonal", 0) != 0;
    std::unique_ptr<gko::LinOp> s;
    if (c.pi("upper")) {
        s = gko::solver::UpperTrs<V, I>::build().with_num_rhs(b->get_size()[1]).with_unit_diagonal(unit).on(exec)->generate(A);
    } else {
        s = gko::solver::LowerTrs<V, I>::build().with_num_rhs(b->get_size()[1]).with_unit_diagonal(unit).on(exec)->generate(A);
    }
    s->apply(b.get(), x.get());
    out_dense(c, "x", x.get());
}

template <typename V, typename I>
std::unique_ptr<typename gko::preconditioner::Jacobi<V, I>::Factory> jacobi_factory(const Case& c)
{
    auto p = gko::preconditioner::Jacobi<V, I>::build();
    p.with_max_block_size(static_cast<gko::uint32>(c.pi("max_block_size", 32)));
    if (c.has("max_block_stride")) p.with_max_block_stride(static_cast<gko::uint32>(c.pi("max_block_stride")));
    if (c.pi("adaptive", 0)) {
        p.with_storage_optimization(gko::precision_reduction::autodetect());
        p.with_accuracy(c.p("accuracy", 1e-1));
    }
    if (c.in.count("block_pointers")) p.with_block_pointers(in_array<I>(c, "block_pointers"));
    if (c.pi("skip_sorting", 0)) p.with_skip_sorting(true);
    return p.on(exec);
}

// jacobi: returns the block pointers, precisions, block storage and
// conditioning; with b given, x = M^-1 b (op 0), alpha M^-1 b + beta x (op 1)
// or the same with the transposed preconditioner (op 2)
template <typename V, typename I>
void v_jacobi(Case& c)
{
    using J = gko::preconditioner::Jacobi<V, I>;
    std::shared_ptr<gko::matrix::Csr<V, I>> A = in_csr<V, I>(c);
    auto j = jacobi_factory<V, I>(c)->generate(A);
    size_type nb = j->get_num_blocks();
    c.put_scalar<gko::int64>("num_blocks", nb);
    c.put("blocks", j->get_blocks(), j->get_num_stored_elements());
    if (j->get_parameters().max_block_size > 1) {
        // scalar Jacobi (max_block_size 1) keeps only the inverted diagonal
        c.put("block_pointers", j->get_parameters().block_pointers.get_const_data(), nb + 1);
        const auto& prec = j->get_parameters().storage_optimization.block_wise;
        std::vector<gko::uint8> pr(prec.get_num_elems());
        for (size_type i = 0; i < pr.size(); i++) pr[i] = static_cast<gko::uint8>(prec.get_const_data()[i]);
        c.put("precisions", pr.data(), pr.size());
        auto sch = j->get_storage_scheme();
        gko::int64 scheme[3] = {static_cast<gko::int64>(sch.block_offset), static_cast<gko::int64>(sch.group_offset),
                                static_cast<gko::int64>(sch.group_power)};
        c.put("scheme", scheme, 3);
        if (j->get_conditioning()) c.put("conditioning", j->get_conditioning(), nb);
    }
    if (c.in.count("b")) {
        auto b = in_dense<V>(c, "b");
        auto x = in_dense<V>(c, "x");
        long op = c.pi("op", 0);
        std::unique_ptr<gko::LinOp> t;
        const gko::LinOp* M = j.get();
        if (op == 2) {
            t = j->transpose();
            M = t.get();
        }
        if (c.has("alpha")) {
            M->apply(scalar<V>(c.p("alpha")).get(), b.get(), scalar<V>(c.p("beta")).get(), x.get());
        } else {
            M->apply(b.get(), x.get());
        }
        out_dense(c, "x", x.get());
    }
}

// solve: solver 0 Cg, 1 Fcg, 2 Bicgstab, 3 Cgs, 4 Bicg, 5 Gmres, 6 Ir, 7 Idr;
// precond 0 none, 1 Jacobi, 2 Ilu(ParIlu), 3 Ilu(exact Ilu)
template <typename S, typename P>
std::unique_ptr<gko::LinOp> generate_solver(P extra, std::shared_ptr<const gko::stop::CriterionFactory> it,
                                            std::shared_ptr<const gko::stop::CriterionFactory> rn,
                                            std::shared_ptr<const gko::LinOpFactory> pre, std::shared_ptr<const gko::LinOp> A)
{
    auto p = S::build();
    p.with_criteria(it, rn);
    extra(p, pre);
    return p.on(exec)->generate(A);
}

struct set_precond {
    template <typename P>
    void operator()(P& p, std::shared_ptr<const gko::LinOpFactory> pre) const
    {
        if (pre) p.with_preconditioner(pre);
    }
};

template <typename V, typename I>
void v_solve(Case& c)
{
    using namespace gko::solver;
    std::shared_ptr<gko::matrix::Csr<V, I>> A = in_csr<V, I>(c);
    auto b = in_dense<V>(c, "b");
    auto x = in_dense<V>(c, "x");
    std::shared_ptr<const gko::stop::CriterionFactory> it =
        gko::stop::Iteration::build().with_max_iters(static_cast<size_type>(c.pi("max_iters"))).on(exec);
    gko::stop::mode base = gko::stop::mode::rhs_norm;
    if (c.pi("baseline", 0) == 1) base = gko::stop::mode::initial_resnorm;
    if (c.pi("baseline", 0) == 2) base = gko::stop::mode::absolute;
    std::shared_ptr<gko::stop::CriterionFactory> rn =
        gko::stop::ResidualNorm<V>::build().with_reduction_factor(static_cast<V>(c.p("reduction"))).with_baseline(base).on(exec);
    // a logger on the solver reports 0 iterations in this version of the
    // reference: it listens on the criterion factory instead
    std::shared_ptr<gko::log::Convergence<V>> log = gko::log::Convergence<V>::create();
    std::const_pointer_cast<gko::stop::CriterionFactory>(it)->add_logger(log);
    rn->add_logger(log);
    std::shared_ptr<const gko::LinOpFactory> pre;
    switch (c.pi("precond", 0)) {
    case 0: break;
    case 1: pre = jacobi_factory<V, I>(c); break;
    case 2:
        pre = gko::preconditioner::Ilu<LowerTrs<V, I>, UpperTrs<V, I>, false, I>::build()
                  .with_factorization_factory(gko::factorization::ParIlu<V, I>::build().with_iterations(c.pi("iterations", 5)).on(exec))
                  .on(exec);
        break;
    case 3:
        pre = gko::preconditioner::Ilu<LowerTrs<V, I>, UpperTrs<V, I>, false, I>::build()
                  .with_factorization_factory(gko::factorization::Ilu<V, I>::build().on(exec))
                  .on(exec);
        break;
    default: throw std::runtime_error("unknown preconditioner");
    }
    std::unique_ptr<gko::LinOp> s;
    switch (c.pi("solver")) {
    case 0: s = generate_solver<Cg<V>>(set_precond{}, it, rn, pre, A); break;
    case 1: s = generate_solver<Fcg<V>>(set_precond{}, it, rn, pre, A); break;
    case 2: s = generate_solver<Bicgstab<V>>(set_precond{}, it, rn, pre, A); break;
    case 3: s = generate_solver<Cgs<V>>(set_precond{}, it, rn, pre, A); break;
    case 4: s = generate_solver<Bicg<V>>(set_precond{}, it, rn, pre, A); break;
    case 5: {
        size_type k = c.pi("krylov_dim", 0);
        s = generate_solver<Gmres<V>>(
            [k](typename Gmres<V>::parameters_type& p, std::shared_ptr<const gko::LinOpFactory> pre) {
                p.with_krylov_dim(k);
                if (pre) p.with_preconditioner(pre);
            },
            it, rn, pre, A);
        break;
    }
    case 6: {
        V relax = static_cast<V>(c.p("relaxation_factor", 1.0));
        s = generate_solver<Ir<V>>(
            [relax](typename Ir<V>::parameters_type& p, std::shared_ptr<const gko::LinOpFactory> pre) {
                p.with_relaxation_factor(relax);
                if (pre) p.with_solver(pre);
            },
            it, rn, pre, A);
        break;
    }
    case 7: {
        size_type sdim = c.pi("subspace_dim", 2);
        V kappa = static_cast<V>(c.p("kappa", 0.7));
        bool det = c.pi("deterministic", 1) != 0;
        s = generate_solver<Idr<V>>(
            [=](typename Idr<V>::parameters_type& p, std::shared_ptr<const gko::LinOpFactory> pre) {
                p.with_subspace_dim(sdim).with_kappa(kappa).with_deterministic(det);
                if (pre) p.with_preconditioner(pre);
            },
            it, rn, pre, A);
        break;
    }
    default: throw std::runtime_error("unknown solver");
    }
    s->apply(b.get(), x.get());
    out_dense(c, "x", x.get());
    c.put_scalar<gko::int64>("iterations", log->get_num_iterations());
    c.put_scalar<gko::int64>("converged", log->has_converged());
    if (auto rnorm = dynamic_cast<const gko::matrix::Dense<V>*>(log->get_residual_norm())) {
        out_dense(c, "resnorm", rnorm);
    }
}

// criterion: one check() of a stopping criterion on given statuses.  kind 0 ResidualNorm (tau is the residual
// norm), 1 ImplicitResidualNorm (tau is the implicit squared norm), 2 Iteration.  b is 1 x nrhs, so that the
// rhs_norm baseline is |b| itself.
template <typename V>
void v_criterion(Case& c)
{
    using D = gko::matrix::Dense<V>;
    std::shared_ptr<D> b = in_dense<V>(c, "b");
    size_type nrhs = b->get_size()[1];
    std::shared_ptr<D> sys = D::create(exec, dim<2>(1, 1));
    sys->fill(gko::one<V>());
    auto x = D::create(exec, dim<2>(1, nrhs));
    x->fill(gko::zero<V>());
    gko::stop::mode base = gko::stop::mode::rhs_norm;
    if (c.pi("baseline", 0) == 1) base = gko::stop::mode::initial_resnorm;
    if (c.pi("baseline", 0) == 2) base = gko::stop::mode::absolute;
    std::shared_ptr<const gko::stop::CriterionFactory> f;
    switch (c.pi("kind")) {
    case 0: f = gko::stop::ResidualNorm<V>::build().with_reduction_factor(static_cast<V>(c.p("reduction"))).with_baseline(base).on(exec); break;
    case 1: f = gko::stop::ImplicitResidualNorm<V>::build().with_reduction_factor(static_cast<V>(c.p("reduction"))).with_baseline(base).on(exec); break;
    case 2: f = gko::stop::Iteration::build().with_max_iters(static_cast<size_type>(c.pi("max_iters"))).on(exec); break;
    default: throw std::runtime_error("unknown criterion");
    }
    auto crit = f->generate(sys, b, x.get(), b.get());
    size_t cnt;
    const gko::uint8* st = c.arr<gko::uint8>("stop_status", &cnt);
    if (cnt != nrhs) throw std::runtime_error("stop_status needs one entry per column");
    gko::array<gko::stopping_status> status(exec, nrhs);
    static_assert(sizeof(gko::stopping_status) == 1, "stopping_status is one byte");
    std::memcpy(status.get_data(), st, nrhs);
    bool one_changed = false;
    bool all = false;
    gko::uint8 id = static_cast<gko::uint8>(c.pi("stopping_id"));
    bool fin = c.pi("set_finalized") != 0;
    if (c.pi("kind") == 2) {
        all = crit->update().num_iterations(static_cast<size_type>(c.pi("iteration"))).check(id, fin, &status, &one_changed);
    } else {
        auto tau = in_dense<V>(c, "tau");
        if (c.pi("kind") == 0) {
            all = crit->update().residual_norm(tau.get()).check(id, fin, &status, &one_changed);
        } else {
            all = crit->update().implicit_sq_residual_norm(tau.get()).check(id, fin, &status, &one_changed);
        }
    }
    c.put("stop_status", reinterpret_cast<const gko::uint8*>(status.get_const_data()), nrhs);
    gko::uint8 flags[2] = {static_cast<gko::uint8>(all), static_cast<gko::uint8>(one_changed)};
    c.put("flags", flags, 2);
}

// ---- the families pinned through JSON fixtures (tests/golden/*_ref.json): one verb each, `op` selects the sub-case.
// Their results carry the names the fixtures use: a Csr as <name>row_ptrs, <name>col_idxs, <name>vals.

using csr = gko::matrix::Csr<double, gko::int32>;
using coo = gko::matrix::Coo<double, gko::int32>;
using dense = gko::matrix::Dense<double>;
using factories = std::vector<std::shared_ptr<const gko::LinOpFactory>>;

void out_parts(Case& c, const std::string& name, const gko::LinOp* op)
{
    auto m = gko::as<csr>(op);
    c.put(name + "row_ptrs", m->get_const_row_ptrs(), m->get_size()[0] + 1);
    c.put(name + "col_idxs", m->get_const_col_idxs(), m->get_num_stored_elements());
    c.put(name + "vals", m->get_const_values(), m->get_num_stored_elements());
}

// row-major without the padding of a strided view
void out_rows(Case& c, const std::string& name, const dense* m)
{
    std::vector<double> v;
    for (size_type i = 0; i < m->get_size()[0]; ++i) {
        for (size_type j = 0; j < m->get_size()[1]; ++j) v.push_back(m->at(i, j));
    }
    c.put(name, v.data(), v.size());
}

template <typename T>
void out_counts(Case& c, const std::string& name, const T* p, size_t count)
{
    std::vector<gko::int64> v(p, p + count);
    c.put(name, v.data(), v.size());
}

struct iteration_logger : gko::log::Logger {
    mutable gko::int64 last = -1;
    mutable std::vector<double> tau;
    void on_iteration_complete(const gko::LinOp*, const size_type& it, const gko::LinOp*, const gko::LinOp*,
                               const gko::LinOp* t) const override
    {
        last = static_cast<gko::int64>(it);
        if (t != nullptr) {
            auto d = gko::as<dense>(t);
            tau.assign(d->get_const_values(), d->get_const_values() + d->get_size()[1]);
        }
    }
    iteration_logger() : gko::log::Logger(gko::log::Logger::iteration_complete_mask) {}
};

// ParIlut / ParIct ::generate with the parameters iterations, fill_in_limit, approximate_select
template <typename Factorization>
std::unique_ptr<Factorization> threshold_factorization(const Case& c, std::shared_ptr<csr> a)
{
    return Factorization::build()
        .with_iterations(static_cast<size_type>(c.pi("iterations")))
        .with_fill_in_limit(c.p("fill_in_limit"))
        .with_approximate_select(c.pi("approximate_select") != 0)
        .on(exec)
        ->generate(a);
}

// par_ilut: op 0 ParIlut::generate; op 1 each of the five kernels alone on the intermediate matrices of the first
// iteration (core/factorization/par_ilut.cpp:257-344) at fill_in_limit 1.2
void v_par_ilut(Case& c)
{
    namespace ilut = gko::kernels::reference::par_ilut_factorization;
    namespace fact = gko::kernels::reference::factorization;
    auto a = gko::share(in_csr<double, gko::int32>(c));
    const auto size = a->get_size();
    const size_type n = size[0];
    if (c.pi("op") == 0) {
        auto f = threshold_factorization<gko::factorization::ParIlut<double, gko::int32>>(c, a);
        const gko::int32 nnz[2] = {static_cast<gko::int32>(f->get_l_factor()->get_num_stored_elements()),
                                   static_cast<gko::int32>(f->get_u_factor()->get_num_stored_elements())};
        c.put("nnz", nnz, 2);
        out_parts(c, "l.", f->get_l_factor().get());
        out_parts(c, "u.", f->get_u_factor().get());
        return;
    }
    if (c.pi("op") != 1) throw std::runtime_error("unknown par_ilut op");
    gko::array<gko::int32> l_rp(exec, n + 1), u_rp(exec, n + 1);
    fact::initialize_row_ptrs_l_u(exec, a.get(), l_rp.get_data(), u_rp.get_data());
    const size_t l_nnz = l_rp.get_data()[n], u_nnz = u_rp.get_data()[n];
    auto l = csr::create(exec, size, gko::array<double>(exec, l_nnz), gko::array<gko::int32>(exec, l_nnz), std::move(l_rp));
    auto u = csr::create(exec, size, gko::array<double>(exec, u_nnz), gko::array<gko::int32>(exec, u_nnz), std::move(u_rp));
    fact::initialize_l_u(exec, a.get(), l.get(), u.get());
    const gko::int32 l_limit = static_cast<gko::int32>(l_nnz * 1.2), u_limit = static_cast<gko::int32>(u_nnz * 1.2);
    auto lu = csr::create(exec, size);
    l->apply(u.get(), lu.get());
    out_parts(c, "lu.", lu.get());
    auto l_new = csr::create(exec, size), u_new = csr::create(exec, size);
    ilut::add_candidates(exec, lu.get(), a.get(), l.get(), u.get(), l_new.get(), u_new.get());
    out_parts(c, "add_candidates.l.", l_new.get());
    out_parts(c, "add_candidates.u.", u_new.get());
    auto u_new_csc = gko::as<csr>(u_new->transpose());
    const coo* no_coo = nullptr;
    ilut::compute_l_u_factors(exec, a.get(), l_new.get(), no_coo, u_new.get(), no_coo, u_new_csc.get());
    out_parts(c, "sweep.l.", l_new.get());
    out_parts(c, "sweep.u.", u_new.get());
    out_parts(c, "sweep.u_csc.", u_new_csc.get());
    const gko::int32 ln = static_cast<gko::int32>(l_new->get_num_stored_elements());
    const gko::int32 un = static_cast<gko::int32>(u_new->get_num_stored_elements());
    const gko::int32 ranks[2] = {std::max<gko::int32>(0, ln - l_limit - 1), std::max<gko::int32>(0, un - u_limit - 1)};
    c.put("ranks", ranks, 2);
    gko::array<double> tmp(exec), tmp2(exec);
    double select[2] = {}, approx[2] = {};
    ilut::threshold_select(exec, l_new.get(), ranks[0], tmp, tmp2, select[0]);
    ilut::threshold_select(exec, u_new_csc.get(), ranks[1], tmp, tmp2, select[1]);
    c.put("select", select, 2);
    coo* null_coo = nullptr;
    auto l_f = csr::create(exec, size), u_f = csr::create(exec, size);
    auto l_coo = coo::create(exec, size);
    ilut::threshold_filter(exec, l_new.get(), select[0], l_f.get(), l_coo.get(), true);
    ilut::threshold_filter(exec, u_new.get(), select[1], u_f.get(), null_coo, false);
    out_parts(c, "filter.l.", l_f.get());
    c.put("filter.l.row_idxs", l_coo->get_const_row_idxs(), l_f->get_num_stored_elements());
    out_parts(c, "filter.u.", u_f.get());
    auto l_a = csr::create(exec, size), ut_a = csr::create(exec, size);
    ilut::threshold_filter_approx(exec, l_new.get(), ranks[0], tmp, approx[0], l_a.get(), null_coo);
    ilut::threshold_filter_approx(exec, u_new_csc.get(), ranks[1], tmp, approx[1], ut_a.get(), null_coo);
    c.put("approx", approx, 2);
    out_parts(c, "filter_approx.l.", l_a.get());
    out_parts(c, "filter_approx.u_csc.", ut_a.get());
}

// par_ict: op 0 ParIct::generate; op 1 each kernel alone on the intermediate matrices of the first iteration
// (core/factorization/par_ict.cpp:228-292) at fill_in_limit 1.2
void v_par_ict(Case& c)
{
    namespace ict = gko::kernels::reference::par_ict_factorization;
    namespace ilut = gko::kernels::reference::par_ilut_factorization;
    namespace fact = gko::kernels::reference::factorization;
    auto a = gko::share(in_csr<double, gko::int32>(c));
    const auto size = a->get_size();
    const size_type n = size[0];
    if (c.pi("op") == 0) {
        auto f = threshold_factorization<gko::factorization::ParIct<double, gko::int32>>(c, a);
        const gko::int32 nnz = static_cast<gko::int32>(f->get_l_factor()->get_num_stored_elements());
        c.put("nnz", &nnz, 1);
        out_parts(c, "l.", f->get_l_factor().get());
        return;
    }
    if (c.pi("op") != 1) throw std::runtime_error("unknown par_ict op");
    gko::array<gko::int32> l_rp(exec, n + 1);
    fact::initialize_row_ptrs_l(exec, a.get(), l_rp.get_data());
    const size_t l_nnz = l_rp.get_data()[n];
    auto l = csr::create(exec, size, gko::array<double>(exec, l_nnz), gko::array<gko::int32>(exec, l_nnz), std::move(l_rp));
    fact::initialize_l(exec, a.get(), l.get(), true);
    out_parts(c, "initialize_l.", l.get());
    const gko::int32 l_limit = static_cast<gko::int32>(l_nnz * 1.2);
    auto lh = gko::as<csr>(l->conj_transpose());
    auto llh = csr::create(exec, size);
    l->apply(lh.get(), llh.get());
    out_parts(c, "llh.", llh.get());
    auto l_new = csr::create(exec, size);
    ict::add_candidates(exec, llh.get(), a.get(), l.get(), l_new.get());
    out_parts(c, "add_candidates.", l_new.get());
    const coo* no_coo = nullptr;
    ict::compute_factor(exec, a.get(), l_new.get(), no_coo);
    out_parts(c, "sweep.", l_new.get());
    const gko::int32 ln = static_cast<gko::int32>(l_new->get_num_stored_elements());
    const gko::int32 rank = std::max<gko::int32>(0, ln - l_limit - 1);
    c.put("ranks", &rank, 1);
    gko::array<double> tmp(exec), tmp2(exec);
    double select = 0.0, approx = 0.0;
    ilut::threshold_select(exec, l_new.get(), rank, tmp, tmp2, select);
    c.put("select", &select, 1);
    coo* null_coo = nullptr;
    auto l_f = csr::create(exec, size);
    ilut::threshold_filter(exec, l_new.get(), select, l_f.get(), null_coo, true);
    out_parts(c, "filter.", l_f.get());
    auto l_a = csr::create(exec, size);
    ilut::threshold_filter_approx(exec, l_new.get(), rank, tmp, approx, l_a.get(), null_coo);
    c.put("approx", &approx, 1);
    out_parts(c, "filter_approx.", l_a.get());
    ict::compute_factor(exec, a.get(), l_f.get(), no_coo);
    out_parts(c, "second_sweep.", l_f.get());
}

template <gko::preconditioner::isai_type Type>
std::shared_ptr<const gko::LinOp> isai_inverse(const Case& c, std::shared_ptr<csr> a)
{
    return gko::preconditioner::Isai<Type, double, gko::int32>::build()
        .with_sparsity_power(static_cast<int>(c.pi("sparsity_power")))
        .with_excess_limit(static_cast<size_type>(c.pi("excess_limit")))
        .on(exec)
        ->generate(a)
        ->get_approximate_inverse();
}

// isai: Isai::generate by kind, sparsity_power and excess_limit (for spd: L, the second operator of the composition),
// then generate_tri_inverse / generate_general_inverse alone on that pattern with zeroed values (long rows stay zero)
// with both prefix arrays and counts = { rows over the limit, their entries, longest row, blocks of the excess loop },
// and generate_excess_system of every block b of the loop over excess_limit as excess/<b>/...
void v_isai(Case& c)
{
    namespace isai = gko::kernels::reference::isai;
    using gko::preconditioner::isai_type;
    auto a = gko::share(in_csr<double, gko::int32>(c));
    const long n = a->get_size()[0], kind = c.pi("kind"), limit = c.pi("excess_limit");
    a->sort_by_column_index();
    const bool tri = kind == ISAI_LOWER || kind == ISAI_UPPER;
    std::shared_ptr<const csr> inverse;
    switch (kind) {
    case ISAI_LOWER: inverse = gko::as<const csr>(isai_inverse<isai_type::lower>(c, a)); break;
    case ISAI_UPPER: inverse = gko::as<const csr>(isai_inverse<isai_type::upper>(c, a)); break;
    case ISAI_GENERAL: inverse = gko::as<const csr>(isai_inverse<isai_type::general>(c, a)); break;
    case ISAI_SPD:
        inverse = gko::as<const csr>(
            gko::as<const gko::Composition<double>>(isai_inverse<isai_type::spd>(c, a))->get_operators()[1]);
        break;
    default: throw std::runtime_error("unknown isai kind");
    }
    auto direct = inverse->clone();
    std::fill_n(direct->get_values(), direct->get_num_stored_elements(), 0.0);
    gko::array<gko::int32> rhs_ptrs(exec, n + 1), nz_ptrs(exec, n + 1);
    if (tri) {
        isai::generate_tri_inverse(exec, a.get(), direct.get(), rhs_ptrs.get_data(), nz_ptrs.get_data(), kind == ISAI_LOWER);
    } else {
        isai::generate_general_inverse(exec, a.get(), direct.get(), rhs_ptrs.get_data(), nz_ptrs.get_data(), kind == ISAI_SPD);
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
    if (tri || counts[0] == 0) out_parts(c, "generate/inverse.", inverse.get());
    out_parts(c, "kernel/direct.", direct.get());
    c.put("kernel/excess_rhs_ptrs", rhs_ptrs.get_const_data(), n + 1);
    c.put("kernel/excess_nz_ptrs", nz_ptrs.get_const_data(), n + 1);
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
        auto system = csr::create(exec, gko::dim<2>(dim, dim), e_nnz);
        auto rhs = dense::create(exec, gko::dim<2>(dim, 1));
        isai::generate_excess_system(exec, a.get(), direct.get(), host_rhs, host_nz, system.get(), rhs.get(), start, block);
        const std::string tag = "excess/" + std::to_string(counts[3]) + "/";
        const gko::int32 range[2] = {static_cast<gko::int32>(start), static_cast<gko::int32>(block)};
        c.put(tag + "range", range, 2);
        out_parts(c, tag + "system.", system.get());
        c.put(tag + "rhs_vals", rhs->get_const_values(), dim);
        ++counts[3];
    }
    c.put("kernel/counts", counts, 4);
}

gko::stop::mode baseline_mode(long word)
{
    switch (word) {
    case BASE_RHS_NORM: return gko::stop::mode::rhs_norm;
    case BASE_INITIAL_RESNORM: return gko::stop::mode::initial_resnorm;
    case BASE_ABSOLUTE: return gko::stop::mode::absolute;
    }
    throw std::runtime_error("unknown baseline");
}

// the stored bits of a Krylov basis as integers of the storage's width; the wire has no 16-bit type, so those go as
// bytes
template <typename Stored>
void out_raw(Case& c, const std::string& name, const Stored* p, size_t count)
{
    if (sizeof(Stored) == 8) {
        c.put(name, reinterpret_cast<const gko::int64*>(p), count);
    } else if (sizeof(Stored) == 4) {
        c.put(name, reinterpret_cast<const gko::int32*>(p), count);
    } else {
        static_assert(sizeof(Stored) >= 2, "no storage type is narrower than 16 bits");
        c.put(name, reinterpret_cast<const gko::uint8*>(p), 2 * count);
    }
}

// the scalars of an integer basis, (krylov_dim + 1) x nrhs; nothing for the floating storages
template <typename Range>
void out_scalars(Case& c, Range range, size_t count, std::true_type)
{
    c.put("scalars", range.get_accessor().get_const_scalar(), count);
}

template <typename Range>
void out_scalars(Case&, Range, size_t, std::false_type)
{}

// initialize, restart, `steps` times { next = A next; arnoldi } with column stop_col stopped before step stop_step
// (-1: never), then solve_krylov
template <typename Storage>
void cb_gmres_kernels(Case& c, const csr* a, const dense* b)
{
    namespace kernels = gko::kernels::reference::cb_gmres;
    using helper = gko::cb_gmres::Range3dHelper<double, Storage>;
    const size_type n = b->get_size()[0], nrhs = b->get_size()[1], kd = c.pi("krylov_dim");
    const long steps = c.pi("steps"), stop_col = c.pi("stop_col"), stop_step = c.pi("stop_step");
    helper h(exec, gko::dim<3>{kd + 1, n, nrhs});
    auto range = h.get_range();
    auto residual = dense::create(exec, dim<2>{n, nrhs});
    auto next = dense::create(exec, dim<2>{n, nrhs});
    auto pv = dense::create(exec, dim<2>{n, nrhs});
    auto hessenberg = dense::create(exec, dim<2>{kd + 1, kd * nrhs});
    auto buffer = dense::create(exec, dim<2>{kd + 1, nrhs});
    auto gsin = dense::create(exec, dim<2>{kd, nrhs});
    auto gcos = dense::create(exec, dim<2>{kd, nrhs});
    auto rnc = dense::create(exec, dim<2>{kd + 1, nrhs});
    auto residual_norm = dense::create(exec, dim<2>{1, nrhs});
    auto arnoldi_norm = dense::create(exec, dim<2>{3, nrhs});
    auto y = dense::create(exec, dim<2>{kd, nrhs});
    auto before = dense::create(exec, dim<2>{n, nrhs});
    hessenberg->fill(0.0);
    buffer->fill(0.0);
    arnoldi_norm->fill(0.0);
    y->fill(0.0);
    gko::array<size_type> final_iter_nums(exec, nrhs), num_reorth(exec, 1);
    gko::array<gko::stopping_status> stop_status(exec, nrhs), reorth_status(exec, nrhs);
    gko::array<char> tmp(exec);

    kernels::initialize(exec, b, residual.get(), gsin.get(), gcos.get(), &stop_status, kd);
    out_rows(c, "initialize/residual", residual.get());
    kernels::restart(exec, residual.get(), residual_norm.get(), rnc.get(), arnoldi_norm.get(), range, next.get(),
                     &final_iter_nums, tmp, kd);
    out_rows(c, "restart/residual_norm", residual_norm.get());
    out_rows(c, "restart/residual_norm_collection", rnc.get());
    out_rows(c, "restart/next", next.get());
    out_raw(c, "restart/basis", h.get_bases().get_const_data(), (kd + 1) * n * nrhs);
    for (long s = 0; s < steps; ++s) {
        if (s == stop_step) stop_status.get_data()[stop_col].stop(1);
        pv->copy_from(next.get());
        a->apply(pv.get(), next.get());
        auto hessenberg_iter = hessenberg->create_submatrix(gko::span{0, s + 2}, gko::span{nrhs * s, nrhs * (s + 1)});
        auto buffer_iter = buffer->create_submatrix(gko::span{0, s + 2}, gko::span{0, nrhs});
        kernels::arnoldi(exec, next.get(), gsin.get(), gcos.get(), residual_norm.get(), rnc.get(), range,
                         hessenberg_iter.get(), buffer_iter.get(), arnoldi_norm.get(), s, &final_iter_nums, &stop_status,
                         &reorth_status, &num_reorth);
        const std::string at = "arnoldi/" + std::to_string(s) + "/";
        out_rows(c, at + "next", next.get());
        out_rows(c, at + "hessenberg_iter", hessenberg_iter.get());
        out_rows(c, at + "arnoldi_norm", arnoldi_norm.get());
        out_rows(c, at + "residual_norm", residual_norm.get());
        out_rows(c, at + "residual_norm_collection", rnc.get());
        out_counts(c, at + "final_iter_nums", final_iter_nums.get_const_data(), nrhs);
    }
    out_rows(c, "givens_sin", gsin.get());
    out_rows(c, "givens_cos", gcos.get());
    auto hessenberg_view = hessenberg->create_submatrix(gko::span{0, steps}, gko::span{0, nrhs * steps});
    kernels::solve_krylov(exec, rnc.get(), range.get_accessor().to_const(), hessenberg_view.get(), y.get(), before.get(),
                          &final_iter_nums);
    out_rows(c, "solve_krylov/y", y.get());
    out_rows(c, "solve_krylov/before_preconditioner", before.get());
    out_raw(c, "basis", h.get_bases().get_const_data(), (kd + 1) * n * nrhs);
    out_scalars(c, range, (kd + 1) * nrhs, gko::cb_gmres::detail::has_3d_scaled_accessor<decltype(range)>{});
}

// cb_gmres: op 0 a whole solve from x = 0 (storage, krylov_dim, max_iters, reduction, baseline, jacobi = the
// block-Jacobi max_block_size or 0 for no preconditioner); op 1 the four kernels (cb_gmres_kernels above).
// storage is the reference's storage_precision: 0 keep, 1 reduce1, 2 reduce2, 3 integer, 4 ireduce1, 5 ireduce2
void v_cb_gmres(Case& c)
{
    using gko::solver::cb_gmres::storage_precision;
    auto a = gko::share(in_csr<double, gko::int32>(c));
    auto b = in_dense<double>(c, "b");
    const long storage = c.pi("storage");
    if (c.pi("op") == 0) {
        auto builder = gko::solver::CbGmres<double>::build()
                           .with_krylov_dim(static_cast<size_type>(c.pi("krylov_dim")))
                           .with_storage_precision(static_cast<storage_precision>(storage))
                           .with_criteria(gko::stop::Iteration::build()
                                              .with_max_iters(static_cast<size_type>(c.pi("max_iters")))
                                              .on(exec),
                                          gko::stop::ResidualNorm<double>::build()
                                              .with_baseline(baseline_mode(c.pi("baseline")))
                                              .with_reduction_factor(c.p("reduction"))
                                              .on(exec));
        if (c.pi("jacobi") > 0) {
            builder.with_preconditioner(gko::preconditioner::Jacobi<double, gko::int32>::build()
                                            .with_max_block_size(static_cast<gko::uint32>(c.pi("jacobi")))
                                            .on(exec));
        }
        auto solver = builder.on(exec)->generate(a);
        auto logger = std::make_shared<iteration_logger>();
        solver->add_logger(logger);
        auto x = dense::create(exec, b->get_size());
        x->fill(0.0);
        solver->apply(b.get(), x.get());
        out_rows(c, "x", x.get());
        c.put_scalar<gko::int64>("iterations", logger->last);
        c.put("residual_norm", logger->tau.data(), logger->tau.size());
        return;
    }
    if (c.pi("op") != 1) throw std::runtime_error("unknown cb_gmres op");
    switch (storage) {
    case 0: return cb_gmres_kernels<double>(c, a.get(), b.get());
    case 1: return cb_gmres_kernels<float>(c, a.get(), b.get());
    case 2: return cb_gmres_kernels<gko::half>(c, a.get(), b.get());
    case 3: return cb_gmres_kernels<gko::int64>(c, a.get(), b.get());
    case 4: return cb_gmres_kernels<gko::int32>(c, a.get(), b.get());
    case 5: return cb_gmres_kernels<gko::int16>(c, a.get(), b.get());
    default: throw std::runtime_error("unknown storage");
    }
}

gko::solver::initial_guess_mode guess_mode(long word)
{
    switch (word) {
    case GUESS_ZERO: return gko::solver::initial_guess_mode::zero;
    case GUESS_RHS: return gko::solver::initial_guess_mode::rhs;
    case GUESS_PROVIDED: return gko::solver::initial_guess_mode::provided;
    }
    throw std::runtime_error("unknown initial guess");
}

// the i32 array `name` of smoother words, of any length
factories smoothers(const Case& c, const std::string& name)
{
    factories out;
    size_t count;
    const gko::int32* words = c.arr<gko::int32>(name, &count);
    for (size_t i = 0; i < count; ++i) {
        switch (words[i]) {
        case SMOOTHER_NULL: out.push_back(nullptr); break;
        case SMOOTHER_EYE: out.push_back(gko::share(gko::matrix::IdentityFactory<double>::create(exec))); break;
        case SMOOTHER_JACOBI:
            out.push_back(gko::share(gko::preconditioner::Jacobi<double, gko::int32>::build().with_max_block_size(1u).on(exec)));
            break;
        default: throw std::runtime_error("unknown smoother");
        }
    }
    return out;
}

// solver::Multigrid over the given level factories, applied to b and x: cycle, mid_case, post_uses_pre, max_levels,
// min_coarse_rows, coarsest (direct: Lu with symmetric sparsity; cg: ten iterations), relax, smoother_iters, guess,
// max_iters, reduction (0: Iteration only) and the smoother lists pre, mid, post.  With cg_max_iters and cg_reduction
// that Multigrid preconditions a Cg instead, which is applied.  The solve of multigrid and of pgm.
void multigrid_solve(Case& c, const factories& levels)
{
    namespace mg = gko::solver::multigrid;
    auto a = gko::share(in_csr<double, gko::int32>(c));
    auto b = in_dense<double>(c, "b");
    auto x = in_dense<double>(c, "x");
    factories coarsest;
    switch (c.pi("coarsest")) {
    case COARSEST_IDENTITY: break;
    case COARSEST_DIRECT:
        coarsest.push_back(gko::share(gko::experimental::solver::Direct<double, gko::int32>::build()
                                          .with_factorization(gko::experimental::factorization::Lu<double, gko::int32>::build()
                                                                  .with_symmetric_sparsity(true)
                                                                  .on(exec))
                                          .on(exec)));
        break;
    case COARSEST_CG:
        coarsest.push_back(gko::share(
            gko::solver::Cg<double>::build().with_criteria(gko::stop::Iteration::build().with_max_iters(10u).on(exec)).on(exec)));
        break;
    default: throw std::runtime_error("unknown coarsest solver");
    }
    std::vector<std::shared_ptr<const gko::stop::CriterionFactory>> criteria;
    criteria.push_back(
        gko::share(gko::stop::Iteration::build().with_max_iters(static_cast<size_type>(c.pi("max_iters"))).on(exec)));
    if (c.p("reduction") != 0.0) {
        criteria.push_back(gko::share(gko::stop::ResidualNorm<double>::build()
                                          .with_baseline(gko::stop::mode::rhs_norm)
                                          .with_reduction_factor(c.p("reduction"))
                                          .on(exec)));
    }
    mg::mid_smooth_type mid_case;
    switch (c.pi("mid_case")) {
    case MID_BOTH: mid_case = mg::mid_smooth_type::both; break;
    case MID_POST_SMOOTHER: mid_case = mg::mid_smooth_type::post_smoother; break;
    case MID_PRE_SMOOTHER: mid_case = mg::mid_smooth_type::pre_smoother; break;
    case MID_STANDALONE: mid_case = mg::mid_smooth_type::standalone; break;
    default: throw std::runtime_error("unknown mid_case");
    }
    mg::cycle cycle;
    switch (c.pi("cycle")) {
    case CYCLE_V: cycle = mg::cycle::v; break;
    case CYCLE_F: cycle = mg::cycle::f; break;
    case CYCLE_W: cycle = mg::cycle::w; break;
    default: throw std::runtime_error("unknown cycle");
    }
    auto factory = gko::solver::Multigrid::build()
                      .with_mg_level(levels)
                      .with_pre_smoother(smoothers(c, "pre"))
                      .with_mid_smoother(smoothers(c, "mid"))
                      .with_post_smoother(smoothers(c, "post"))
                      .with_post_uses_pre(c.pi("post_uses_pre") != 0)
                      .with_mid_case(mid_case)
                      .with_max_levels(static_cast<size_type>(c.pi("max_levels")))
                      .with_min_coarse_rows(static_cast<size_type>(c.pi("min_coarse_rows")))
                      .with_coarsest_solver(coarsest)
                      .with_cycle(cycle)
                      .with_smoother_relax(c.p("relax"))
                      .with_smoother_iters(static_cast<size_type>(c.pi("smoother_iters")))
                      .with_default_initial_guess(guess_mode(c.pi("guess")))
                      .with_criteria(criteria)
                      .on(exec);
    auto logger = std::make_shared<iteration_logger>();
    if (c.has("cg_max_iters")) {
        auto cg = gko::solver::Cg<double>::build()
                      .with_preconditioner(gko::share(std::move(factory)))
                      .with_criteria(gko::stop::Iteration::build()
                                         .with_max_iters(static_cast<size_type>(c.pi("cg_max_iters")))
                                         .on(exec),
                                     gko::stop::ResidualNorm<double>::build()
                                         .with_baseline(gko::stop::mode::rhs_norm)
                                         .with_reduction_factor(c.p("cg_reduction"))
                                         .on(exec))
                      .on(exec)
                      ->generate(a);
        cg->add_logger(logger);
        cg->apply(b.get(), x.get());
        out_rows(c, "x", x.get());
        c.put_scalar<gko::int64>("iterations", logger->last);
        return;
    }
    auto solver = factory->generate(a);
    solver->add_logger(logger);
    solver->apply(b.get(), x.get());
    out_rows(c, "x", x.get());
    c.put_scalar<gko::int64>("iterations", logger->last);
    std::vector<gko::int64> rows;
    for (const auto& level : solver->get_mg_level_list()) {
        rows.push_back(static_cast<gko::int64>(level->get_coarse_op()->get_size()[0]));
    }
    c.put("levels", rows.data(), rows.size());
}

// FixedCoarsening on every second row (or on every row: a level that does not reduce) of whatever matrix it is handed
struct strided_coarsening : gko::EnablePolymorphicObject<strided_coarsening, gko::LinOpFactory> {
    explicit strided_coarsening(std::shared_ptr<const gko::Executor> e, long stride = 2)
        : gko::EnablePolymorphicObject<strided_coarsening, gko::LinOpFactory>(e), stride_(stride)
    {}
    std::unique_ptr<gko::LinOp> generate_impl(std::shared_ptr<const gko::LinOp> op) const override
    {
        const long n = static_cast<long>(op->get_size()[0]);
        const long m = (n + stride_ - 1) / stride_;
        gko::array<gko::int32> rows(this->get_executor(), m);
        for (long i = 0; i < m; ++i) rows.get_data()[i] = static_cast<gko::int32>(i * stride_);
        return gko::multigrid::FixedCoarsening<double, gko::int32>::build().with_coarse_rows(rows).on(this->get_executor())->generate(op);
    }
    long stride_;
};

// multigrid: op 0 the three kcycle kernels on alpha rho gamma beta zeta (1 x nrhs) and v g d e (n x nrhs);
// op 1 FixedCoarsening on coarse_rows; op 2 the smoother Multigrid builds, Ir over scalar Jacobi (sweeps, zero_guess,
// relax); op 3 a whole solve (multigrid_solve) over the mg_level words halve / all_rows
void v_multigrid(Case& c)
{
    namespace kernels = gko::kernels::reference::multigrid;
    switch (c.pi("op")) {
    case 0: {
        auto alpha = in_dense<double>(c, "alpha"), rho = in_dense<double>(c, "rho"), gamma = in_dense<double>(c, "gamma");
        auto beta = in_dense<double>(c, "beta"), zeta = in_dense<double>(c, "zeta");
        auto v = in_dense<double>(c, "v"), g = in_dense<double>(c, "g"), d = in_dense<double>(c, "d"), e = in_dense<double>(c, "e");
        const long nrhs = alpha->get_size()[1];
        auto d2 = gko::clone(d), e2 = gko::clone(e);
        kernels::kcycle_step_1(exec, alpha.get(), rho.get(), v.get(), g.get(), d.get(), e.get());
        out_rows(c, "step_1/g", g.get());
        out_rows(c, "step_1/d", d.get());
        out_rows(c, "step_1/e", e.get());
        kernels::kcycle_step_2(exec, alpha.get(), rho.get(), gamma.get(), beta.get(), zeta.get(), d2.get(), e2.get());
        out_rows(c, "step_2/e", e2.get());
        // old = beta, new = 0.25 beta: equal to the threshold in every column, then one column just above it
        auto fresh = gko::clone(beta);
        for (long j = 0; j < nrhs; ++j) fresh->at(0, j) = 0.25 * beta->at(0, j);
        bool equal = false, above = true;
        kernels::kcycle_check_stop(exec, beta.get(), fresh.get(), 0.25, equal);
        fresh->at(0, nrhs - 1) = std::nextafter(fresh->at(0, nrhs - 1), 1e300);
        kernels::kcycle_check_stop(exec, beta.get(), fresh.get(), 0.25, above);
        const gko::int64 stops[2] = {equal, above};
        c.put("check_stop/is_stop", stops, 2);
        break;
    }
    case 1: {
        auto a = gko::share(in_csr<double, gko::int32>(c));
        auto level = gko::multigrid::FixedCoarsening<double, gko::int32>::build()
                         .with_coarse_rows(in_array<gko::int32>(c, "coarse_rows"))
                         .with_skip_sorting(c.pi("skip_sorting") != 0)
                         .on(exec)
                         ->generate(a);
        out_parts(c, "fine/", level->get_fine_op().get());
        out_parts(c, "restrict/", level->get_restrict_op().get());
        out_parts(c, "prolong/", level->get_prolong_op().get());
        out_parts(c, "coarse/", level->get_coarse_op().get());
        break;
    }
    case 2: {
        auto a = gko::share(in_csr<double, gko::int32>(c));
        auto b = in_dense<double>(c, "b");
        auto x = in_dense<double>(c, "x");
        std::shared_ptr<const gko::LinOpFactory> inner =
            gko::preconditioner::Jacobi<double, gko::int32>::build().with_max_block_size(1u).on(exec);
        // build_smoother's Ir (include/ginkgo/core/solver/ir.hpp:314-326) with the initial-guess mode as a factory
        // parameter: apply_with_initial_guess itself is reserved to Multigrid
        auto smoother = gko::solver::Ir<double>::build()
                            .with_solver(inner)
                            .with_relaxation_factor(c.p("relax"))
                            .with_criteria(gko::stop::Iteration::build()
                                               .with_max_iters(static_cast<size_type>(c.pi("sweeps")))
                                               .on(exec))
                            .with_default_initial_guess(guess_mode(c.pi("zero_guess") ? GUESS_ZERO : GUESS_PROVIDED))
                            .on(exec)
                            ->generate(a);
        smoother->apply(b.get(), x.get());
        out_rows(c, "x", x.get());
        break;
    }
    case 3: {
        factories levels;
        size_t count;
        const gko::int32* words = c.arr<gko::int32>("mg_level", &count);
        for (size_t i = 0; i < count; ++i) {
            if (words[i] != LEVEL_HALVE && words[i] != LEVEL_ALL_ROWS) throw std::runtime_error("unknown mg_level");
            levels.push_back(std::make_shared<strided_coarsening>(exec, words[i] == LEVEL_ALL_ROWS ? 1 : 2));
        }
        multigrid_solve(c, levels);
        break;
    }
    default: throw std::runtime_error("unknown multigrid op");
    }
}

// pgm: op 0 Pgm::generate (pgm_max_iterations, pgm_max_unassigned_ratio, pgm_deterministic, skip_sorting): the
// aggregates, the restriction, the fine operator's column order and the coarse matrix; op 1 a whole solve
// (multigrid_solve) with that Pgm factory for every mg_level word
void v_pgm(Case& c)
{
    using pgm = gko::multigrid::Pgm<double, gko::int32>;
    long op = c.pi("op");
    auto factory = gko::share(pgm::build()
                                  .with_max_iterations(static_cast<unsigned>(c.pi("pgm_max_iterations")))
                                  .with_max_unassigned_ratio(c.p("pgm_max_unassigned_ratio"))
                                  .with_deterministic(c.pi("pgm_deterministic") != 0)
                                  .with_skip_sorting(op == 0 && c.pi("skip_sorting") != 0)
                                  .on(exec));
    if (op == 0) {
        auto a = gko::share(in_csr<double, gko::int32>(c));
        auto level = factory->generate(a);
        const size_t n = a->get_size()[0];
        out_counts(c, "agg", level->get_const_agg(), n);
        auto restriction = gko::as<gko::matrix::SparsityCsr<double, gko::int32>>(level->get_restrict_op());
        c.put_scalar<gko::int64>("num_agg", restriction->get_size()[0]);
        c.put("restrict/row_ptrs", restriction->get_const_row_ptrs(), restriction->get_size()[0] + 1);
        c.put("restrict/col_idxs", restriction->get_const_col_idxs(), n);
        auto fine = gko::as<csr>(level->get_fine_op());
        c.put("fine/col_idxs", fine->get_const_col_idxs(), fine->get_num_stored_elements());
        out_parts(c, "coarse/", level->get_coarse_op().get());
    } else if (op == 1) {
        size_t count;
        const gko::int32* words = c.arr<gko::int32>("mg_level", &count);
        for (size_t i = 0; i < count; ++i) {
            if (words[i] != LEVEL_PGM) throw std::runtime_error("unknown mg_level");
        }
        multigrid_solve(c, factories(count, factory));
    } else {
        throw std::runtime_error("unknown pgm op");
    }
}

// ---- dispatch: vt 0 double, 1 float; it 0 int32, 1 int64

void run(Case& c)
{
    long vt = c.pi("vt", 0), it = c.pi("it", 0);
    const std::string& v = c.verb;
    bool base = vt == 0 && it == 0;
    if (v == "spmv") {
        if (base) return v_spmv<double, gko::int32>(c);
        if (c.pi("fmt") != F_CSR) throw std::runtime_error("only Csr has other types");
        if (vt == 0 && it == 1) return v_spmv<double, gko::int64>(c);
        if (vt == 1 && it == 0) return v_spmv<float, gko::int32>(c);
    } else if (v == "dense") {
        if (vt == 0) return v_dense<double>(c);
        if (vt == 1) return v_dense<float>(c);
    } else if (v == "criterion") {
        if (vt == 0) return v_criterion<double>(c);
        if (vt == 1) return v_criterion<float>(c);
    } else if (v == "solve" && vt == 1 && it == 0) {
        return v_solve<float, gko::int32>(c);
    } else if (base) {
        if (v == "convert") return v_convert<double, gko::int32>(c);
        if (v == "fbcsr_op") return v_fbcsr_op<double, gko::int32>(c);
        if (v == "csr_op") return v_csr_op<double, gko::int32>(c);
        if (v == "mdata") return v_mdata<double, gko::int32>(c);
        if (v == "spgemm") return v_spgemm<double, gko::int32>(c);
        if (v == "factor") return v_factor<double, gko::int32>(c);
        if (v == "direct") return v_direct<double, gko::int32>(c);
        if (v == "trs") return v_trs<double, gko::int32>(c);
        if (v == "jacobi") return v_jacobi<double, gko::int32>(c);
        if (v == "solve") return v_solve<double, gko::int32>(c);
        if (v == "par_ilut") return v_par_ilut(c);
        if (v == "par_ict") return v_par_ict(c);
        if (v == "isai") return v_isai(c);
        if (v == "cb_gmres") return v_cb_gmres(c);
        if (v == "multigrid") return v_multigrid(c);
        if (v == "pgm") return v_pgm(c);
    }
    throw std::runtime_error("no verb " + v + " for these types");
}

// ---- the wire format

struct Reader {
    FILE* f;
    void raw(void* p, size_t n)
    {
        if (n && std::fread(p, 1, n, f) != n) throw std::runtime_error("short input");
    }
    template <typename T> T get() { T v; raw(&v, sizeof(T)); return v; }
    std::string str()
    {
        std::string s(get<uint32_t>(), '\0');
        raw(&s[0], s.size());
        return s;
    }
};

struct Writer {
    FILE* f;
    void raw(const void* p, size_t n)
    {
        if (n && std::fwrite(p, 1, n, f) != n) throw std::runtime_error("short output");
    }
    template <typename T> void put(T v) { raw(&v, sizeof(T)); }
    void str(const std::string& s)
    {
        put<uint32_t>(s.size());
        raw(s.data(), s.size());
    }
};

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: ref_driver IN OUT\n");
        return 2;
    }
    try {
        exec = gko::ReferenceExecutor::create();
        Reader r{std::fopen(argv[1], "rb")};
        Writer w{std::fopen(argv[2], "wb")};
        if (!r.f || !w.f) throw std::runtime_error("cannot open the files");
        char magic[4];
        r.raw(magic, 4);
        if (std::memcmp(magic, "GKRI", 4)) throw std::runtime_error("not a ref_driver input");
        uint32_t ncases = r.get<uint32_t>();
        w.raw("GKRO", 4);
        w.put<uint32_t>(ncases);
        for (uint32_t i = 0; i < ncases; i++) {
            Case c;
            c.verb = r.str();
            for (uint32_t n = r.get<uint32_t>(); n > 0; n--) {
                auto name = r.str();
                c.params[name] = r.get<double>();
            }
            for (uint32_t n = r.get<uint32_t>(); n > 0; n--) {
                auto name = r.str();
                Arr a;
                a.code = r.get<uint8_t>();
                if (a.code < 0 || a.code > 4) throw std::runtime_error("bad dtype");
                a.bytes.resize(r.get<uint64_t>() * dt_size[a.code]);
                r.raw(a.bytes.data(), a.bytes.size());
                c.in[name] = std::move(a);
            }
            std::string msg;
            try {
                run(c);
            } catch (const std::exception& e) {
                msg = e.what();
                if (msg.empty()) msg = "failed";
            }
            w.put<uint32_t>(msg.empty() ? 0 : 1);
            w.str(msg);
            if (!msg.empty()) c.out.clear();
            w.put<uint32_t>(c.out.size());
            for (auto& o : c.out) {
                w.str(o.first);
                w.put<uint8_t>(o.second.code);
                w.put<uint64_t>(o.second.count());
                w.raw(o.second.bytes.data(), o.second.bytes.size());
            }
        }
        if (std::fclose(w.f)) throw std::runtime_error("cannot close the output");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "ref_driver: %s\n", e.what());
        return 1;
    }
    return 0;
}
