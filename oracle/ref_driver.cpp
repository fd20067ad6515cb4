// ref_driver -- TEST INFRASTRUCTURE ONLY.
//
// Runs batches of cases on the reference library's ReferenceExecutor through
// its public API, so that the tests can compare the C oracle, the Python
// restatements and the HIP kernels with the reference itself instead of with
// a restatement of it.  This file is the project's own; it is compiled
// against the reference's headers by oracle/ref.mk into oracle/_ref/ and the
// product never links or loads it.
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
