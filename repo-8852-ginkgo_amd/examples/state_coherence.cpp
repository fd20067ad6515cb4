// Scenario driver of tests/test_state_coherence_gpu.py: does a matrix object's cached state (srow, row and column
// statistics, the column-partitioned copy, the sorted-rows state of Coo) follow every change made to the matrix?
//
//   state_coherence <dir>
//
// <dir>/scenarios.txt holds one scenario per line:  id object strategy mutator base payload three dump
//   object    csr | csr64 | csrf | coo | hybrid | cg
//   strategy  classical | load_balance | merge_path | automatical | sparselib | gkomi_partitioned[N]  (N: pinned blocks)
//   mutator   what changes the warm object (see mutate_csr / run_coo below); "set_strategy=<name>" carries the new one
//   base, payload   sub-directories of <dir> with the matrix before and after the change as raw little-endian arrays:
//             meta.txt "rows cols nnz", rp.i32 (or ri.i32 for coo), ci.i32, v.f64, b1.f64 (cols x 1), b3.f64 (cols x 3,
//             row-major), c1.f64, c3.f64 (rows x 1 / 3: the input of the alpha/beta applies)
//   three     1: also apply to three columns;  dump 1: also write the object's final arrays
// Every scenario: create + fill + apply once (warm), change through the mutator, apply again, then a FRESH object of
// the final strategy from the payload's arrays in the same process.  Products go to <dir>/out/<id>.<tag>.f64
// (tags: w1 = warm apply; y1 ya1 y3 ya3 = after the change; f1 fa1 f3 fa3 = fresh object; "a" = alpha/beta apply with
// alpha = -0.75, beta = 1.5), facts to <dir>/out/<id>.info as "key value" lines.  The test knows the final matrix
// without asking this program.
#include <ginkgo/ginkgo.hpp>

#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <limits>
#include <map>
#include <sstream>
#include <string>
#include <vector>

namespace {

constexpr double ALPHA = -0.75, BETA = 1.5;

template <typename T>
std::vector<T> read_raw(const std::string& path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("cannot open " + path);
    const auto bytes = static_cast<size_t>(f.tellg());
    std::vector<T> out(bytes / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(out.data()), static_cast<std::streamsize>(out.size() * sizeof(T)));
    return out;
}

template <typename T>
void write_raw(const std::string& path, const std::vector<T>& data)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(data.data()), static_cast<std::streamsize>(data.size() * sizeof(T)));
    if (!f) throw std::runtime_error("cannot write " + path);
}

struct host_matrix {
    gko::size_type rows{}, cols{}, nnz{};
    std::vector<int32_t> rp, ri, ci;  // rp or ri, whichever the directory has
    std::vector<double> v, b1, b3, c1, c3;
};

bool exists(const std::string& p) { return static_cast<bool>(std::ifstream(p)); }

const host_matrix& load(const std::string& dir, const std::string& name)
{
    static std::map<std::string, host_matrix> cache;
    auto it = cache.find(name);
    if (it != cache.end()) return it->second;
    host_matrix m;
    const std::string d = dir + "/" + name + "/";
    std::ifstream meta(d + "meta.txt");
    if (!(meta >> m.rows >> m.cols >> m.nnz)) throw std::runtime_error("bad meta in " + d);
    if (exists(d + "rp.i32")) m.rp = read_raw<int32_t>(d + "rp.i32");
    if (exists(d + "ri.i32")) m.ri = read_raw<int32_t>(d + "ri.i32");
    m.ci = read_raw<int32_t>(d + "ci.i32");
    m.v = read_raw<double>(d + "v.f64");
    if (m.ci.size() != m.nnz || m.v.size() != m.nnz || (!m.rp.empty() && m.rp.size() != m.rows + 1) || (!m.ri.empty() && m.ri.size() != m.nnz))
        throw std::runtime_error("array sizes do not match meta in " + d);
    for (auto p : {std::make_pair("b1.f64", &m.b1), std::make_pair("b3.f64", &m.b3), std::make_pair("c1.f64", &m.c1), std::make_pair("c3.f64", &m.c3)})
        if (exists(d + p.first)) *p.second = read_raw<double>(d + p.first);
    return cache.emplace(name, std::move(m)).first->second;
}

struct scenario {
    std::string id, object, strategy, mutator, base, payload;
    int three{}, dump{};
};

using exec_ptr = std::shared_ptr<const gko::Executor>;

template <typename V>
std::unique_ptr<gko::matrix::Dense<V>> to_device(exec_ptr exec, const std::vector<double>& data, gko::size_type rows, gko::size_type cols)
{
    if (data.size() != rows * cols) throw std::runtime_error("vector of the wrong size");
    auto h = gko::matrix::Dense<V>::create(exec->get_master(), gko::dim<2>(rows, cols));
    for (gko::size_type i = 0; i < rows; ++i) for (gko::size_type j = 0; j < cols; ++j) h->at(i, j) = static_cast<V>(data[i * cols + j]);
    return h->clone(exec);
}

template <typename V>
std::vector<double> to_host(const gko::matrix::Dense<V>* d)
{
    auto h = d->clone(d->get_executor()->get_master());
    const auto rows = h->get_size()[0], cols = h->get_size()[1];
    std::vector<double> out(rows * cols);
    for (gko::size_type i = 0; i < rows; ++i) for (gko::size_type j = 0; j < cols; ++j) out[i * cols + j] = static_cast<double>(h->at(i, j));
    return out;
}

template <typename T, typename S>
void upload(exec_ptr exec, const std::vector<S>& src, T* dst)
{
    std::vector<T> tmp(src.begin(), src.end());
    exec->copy_from(exec->get_master().get(), tmp.size(), tmp.data(), dst);
}

template <typename T, typename S>
gko::array<T> device_array(exec_ptr exec, const std::vector<S>& src)
{
    std::vector<T> tmp(src.begin(), src.end());
    return gko::array<T>(exec, tmp.begin(), tmp.end());
}

// applies op to the vectors of m (b of op's column count, c of its row count) and writes <id>.<prefix>{1,a1,3,a3}
template <typename V, typename Op>
void apply_all(exec_ptr exec, const std::string& out, const scenario& s, const std::string& prefix, const Op* op, const host_matrix& m, bool three)
{
    const auto rows = op->get_size()[0], cols = op->get_size()[1];
    auto alpha = to_device<V>(exec, {ALPHA}, 1, 1);
    auto beta = to_device<V>(exec, {BETA}, 1, 1);
    for (gko::size_type k : {gko::size_type{1}, gko::size_type{3}}) {
        if (k == 3 && !three) continue;
        auto b = to_device<V>(exec, k == 1 ? m.b1 : m.b3, cols, k);
        auto y = to_device<V>(exec, std::vector<double>(rows * k, std::numeric_limits<double>::quiet_NaN()), rows, k);  // a simple apply never reads its output
        op->apply(b.get(), y.get());
        write_raw(out + s.id + "." + prefix + std::to_string(k) + ".f64", to_host(y.get()));
        auto c = to_device<V>(exec, k == 1 ? m.c1 : m.c3, rows, k);
        op->apply(alpha.get(), b.get(), beta.get(), c.get());
        write_raw(out + s.id + "." + prefix + "a" + std::to_string(k) + ".f64", to_host(c.get()));
    }
}

template <typename V, typename I>
std::shared_ptr<typename gko::matrix::Csr<V, I>::strategy_type> make_strategy(const std::string& name)
{
    using csr = gko::matrix::Csr<V, I>;
    if (name == "classical") return std::make_shared<typename csr::classical>();
    if (name == "load_balance") return std::make_shared<typename csr::load_balance>();
    if (name == "merge_path") return std::make_shared<typename csr::merge_path>();
    if (name == "automatical") return std::make_shared<typename csr::automatical>();
    if (name == "sparselib") return std::make_shared<typename csr::sparselib>();
    if (name.rfind("gkomi_partitioned", 0) == 0) {
        const std::string n = name.substr(std::string("gkomi_partitioned").size());
        return std::make_shared<typename csr::gkomi_partitioned>(n.empty() ? 0 : std::stoi(n));
    }
    throw std::runtime_error("unknown strategy " + name);
}

template <typename V, typename I>
std::unique_ptr<gko::matrix::Csr<V, I>> make_csr(exec_ptr exec, const host_matrix& m, const std::string& strategy)
{
    if (m.rp.empty()) throw std::runtime_error("matrix without row pointers");
    auto A = gko::matrix::Csr<V, I>::create(exec, gko::dim<2>(m.rows, m.cols), m.nnz, make_strategy<V, I>(strategy));
    upload(exec, m.rp, A->get_row_ptrs());
    upload(exec, m.ci, A->get_col_idxs());
    upload(exec, m.v, A->get_values());
    return A;
}

template <typename V, typename I>
gko::matrix_data<V, I> host_data(const host_matrix& m)
{
    gko::matrix_data<V, I> d(gko::dim<2>(m.rows, m.cols));
    d.nonzeros.reserve(m.nnz);
    for (gko::size_type r = 0; r < m.rows; ++r)
        for (int32_t k = m.rp[r]; k < m.rp[r + 1]; ++k) d.nonzeros.push_back({static_cast<I>(r), static_cast<I>(m.ci[k]), static_cast<V>(m.v[k])});
    return d;
}

std::vector<int32_t> row_idxs_of(const host_matrix& m)
{
    if (!m.ri.empty()) return m.ri;
    std::vector<int32_t> ri(m.nnz);
    for (gko::size_type r = 0; r < m.rows; ++r) for (int32_t k = m.rp[r]; k < m.rp[r + 1]; ++k) ri[k] = static_cast<int32_t>(r);
    return ri;
}

template <typename V, typename I>
void dump_csr(const std::string& out, const scenario& s, const gko::matrix::Csr<V, I>* A)
{
    auto exec = A->get_executor();
    const auto n = A->get_size()[0], nnz = A->get_num_stored_elements();
    std::vector<I> rp(n + 1), ci(nnz);
    std::vector<V> v(nnz);
    exec->get_master()->copy_from(exec.get(), n + 1, A->get_const_row_ptrs(), rp.data());
    exec->get_master()->copy_from(exec.get(), nnz, A->get_const_col_idxs(), ci.data());
    exec->get_master()->copy_from(exec.get(), nnz, A->get_const_values(), v.data());
    write_raw(out + s.id + ".rp.raw", rp);
    write_raw(out + s.id + ".ci.raw", ci);
    write_raw(out + s.id + ".v.raw", v);
}

template <typename A>
int has_copy(const A* a) { return a->has_partitioned_copy() ? 1 : 0; }

// the change itself: every path by which a user can alter a warm Csr
template <typename V, typename I>
void mutate_csr(exec_ptr exec, gko::matrix::Csr<V, I>* A, const scenario& s, const host_matrix& to, std::string& final_strategy)
{
    const std::string& m = s.mutator;
    if (m == "values") {
        upload(exec, to.v, A->get_values());
    } else if (m == "cols") {            // columns and values, e.g. a permutation inside the rows
        upload(exec, to.ci, A->get_col_idxs());
        upload(exec, to.v, A->get_values());
    } else if (m == "cols_only") {       // other columns under the same values: another matrix
        upload(exec, to.ci, A->get_col_idxs());
    } else if (m == "sort") {
        if constexpr (std::is_same<V, double>::value && std::is_same<I, gko::int32>::value) A->sort_by_column_index();
        else throw std::runtime_error("sort: double / int32 only");
    } else if (m == "rowptrs") {
        upload(exec, to.rp, A->get_row_ptrs());
    } else if (m == "read_md") {
        A->read(host_data<V, I>(to));
    } else if (m == "read_dmd") {
        gko::device_matrix_data<V, I> d(gko::dim<2>(to.rows, to.cols), device_array<I>(exec, row_idxs_of(to)), device_array<I>(exec, to.ci),
                                       device_array<V>(exec, to.v));
        A->read(std::move(d));
    } else if (m == "builder") {         // CsrBuilder: whole arrays replaced
        gko::matrix::CsrBuilder<V, I> builder(A);
        builder.get_col_idx_array() = device_array<I>(exec, to.ci);
        builder.get_value_array() = device_array<V>(exec, to.v);
    } else if (m.rfind("set_strategy=", 0) == 0) {
        final_strategy = m.substr(13);
        A->set_strategy(make_strategy<V, I>(final_strategy));
    } else {
        throw std::runtime_error("unknown mutator " + m);
    }
}

template <typename V, typename I>
void run_csr(exec_ptr exec, const std::string& dir, const scenario& s, std::ostream& info)
{
    const std::string out = dir + "/out/";
    const auto& from = load(dir, s.base);
    const auto& to = load(dir, s.payload);
    auto A = make_csr<V, I>(exec, from, s.strategy);
    apply_all<V>(exec, out, s, "w", A.get(), from, s.three);
    info << "has_copy_warm " << has_copy(A.get()) << "\n";
    std::string final_strategy = s.strategy;
    if (s.mutator == "repeated") {
        // the documented idiom for repeated writes: ask the getter again after each apply, write, apply
        for (int round = 1; round <= 3; ++round) {
            const auto& r = load(dir, s.payload + "_r" + std::to_string(round));
            upload(exec, r.v, A->get_values());
            apply_all<V>(exec, out, s, "r" + std::to_string(round) + "y", A.get(), r, false);
        }
        upload(exec, to.v, A->get_values());
    } else {
        mutate_csr<V, I>(exec, A.get(), s, to, final_strategy);
    }
    apply_all<V>(exec, out, s, "y", A.get(), to, s.three);
    info << "has_copy_after " << has_copy(A.get()) << "\n";
    if (s.dump) dump_csr(out, s, A.get());
    auto F = make_csr<V, I>(exec, to, final_strategy);
    apply_all<V>(exec, out, s, "f", F.get(), to, s.three);
    info << "has_copy_fresh " << has_copy(F.get()) << "\n";
}

// double / int32 only: conversions between precisions, transpose
void run_csr_special(exec_ptr exec, const std::string& dir, const scenario& s, std::ostream& info)
{
    using csr = gko::matrix::Csr<double, gko::int32>;
    const std::string out = dir + "/out/";
    const auto& from = load(dir, s.base);
    const auto& to = load(dir, s.payload);
    auto A = make_csr<double, gko::int32>(exec, from, s.strategy);
    apply_all<double>(exec, out, s, "w", A.get(), from, s.three);
    info << "has_copy_warm " << has_copy(A.get()) << "\n";
    if (s.mutator == "convert_from_float") {
        // Csr<float>::convert_to(Csr<double>*) into the warm object (the payload's values are floats exactly)
        auto S = make_csr<float, gko::int32>(exec, to, s.strategy);
        S->convert_to(A.get());
        apply_all<double>(exec, out, s, "y", A.get(), to, s.three);
        info << "has_copy_after " << has_copy(A.get()) << "\n";
        info << "strategy_after " << A->get_strategy()->get_name() << "\n";
    } else if (s.mutator == "transpose") {
        // the result is a new object: it must not share state with the warm matrix, nor disturb it
        auto T = A->transpose();
        apply_all<double>(exec, out, s, "y", static_cast<const csr*>(T.get()), to, s.three);
        info << "has_copy_after " << has_copy(T.get()) << "\n";
        if (s.dump) dump_csr(out, s, T.get());
        apply_all<double>(exec, out, s, "o", A.get(), from, s.three);  // the original once more
        info << "has_copy_original " << has_copy(A.get()) << "\n";
    } else {
        throw std::runtime_error("unknown mutator " + s.mutator);
    }
    auto F = make_csr<double, gko::int32>(exec, to, s.strategy);
    apply_all<double>(exec, out, s, "f", F.get(), to, s.three);
    info << "has_copy_fresh " << has_copy(F.get()) << "\n";
}

using coo = gko::matrix::Coo<double, gko::int32>;

std::unique_ptr<coo> make_coo(exec_ptr exec, const host_matrix& m)
{
    auto C = coo::create(exec, gko::dim<2>(m.rows, m.cols), m.nnz);
    upload(exec, row_idxs_of(m), C->get_row_idxs());
    upload(exec, m.ci, C->get_col_idxs());
    upload(exec, m.v, C->get_values());
    return C;
}

// apply, advanced apply, and apply2 (x += A b, x += alpha A b) on one and three columns
void apply_all_coo(exec_ptr exec, const std::string& out, const scenario& s, const std::string& prefix, const coo* C, const host_matrix& m)
{
    using vec = gko::matrix::Dense<double>;
    apply_all<double>(exec, out, s, prefix, C, m, true);
    auto alpha = to_device<double>(exec, {ALPHA}, 1, 1);
    for (gko::size_type k : {gko::size_type{1}, gko::size_type{3}}) {
        auto b = to_device<double>(exec, k == 1 ? m.b1 : m.b3, m.cols, k);
        std::unique_ptr<vec> c = to_device<double>(exec, k == 1 ? m.c1 : m.c3, m.rows, k);
        C->apply2(b.get(), c.get());
        write_raw(out + s.id + "." + prefix + "p" + std::to_string(k) + ".f64", to_host(c.get()));
        c = to_device<double>(exec, k == 1 ? m.c1 : m.c3, m.rows, k);
        C->apply2(alpha.get(), b.get(), c.get());
        write_raw(out + s.id + "." + prefix + "q" + std::to_string(k) + ".f64", to_host(c.get()));
    }
}

void run_coo(exec_ptr exec, const std::string& dir, const scenario& s, std::ostream& info)
{
    const std::string out = dir + "/out/";
    const auto& from = load(dir, s.base);
    const auto& to = load(dir, s.payload);
    auto C = make_coo(exec, from);
    apply_all_coo(exec, out, s, "w", C.get(), from);
    info << "sorted_warm " << C->is_sorted_by_row() << "\n";
    if (s.mutator == "rows") {
        upload(exec, row_idxs_of(to), C->get_row_idxs());
    } else if (s.mutator == "resize") {
        C->resize(gko::dim<2>(to.rows, to.cols), to.nnz);
        upload(exec, row_idxs_of(to), C->get_row_idxs());
        upload(exec, to.ci, C->get_col_idxs());
        upload(exec, to.v, C->get_values());
    } else if (s.mutator == "convert_from_csr") {
        auto A = make_csr<double, gko::int32>(exec, to, "automatical");
        A->convert_to(C.get());
    } else {
        throw std::runtime_error("unknown mutator " + s.mutator);
    }
    apply_all_coo(exec, out, s, "y", C.get(), to);
    info << "sorted_after " << C->is_sorted_by_row() << "\n";
    auto F = make_coo(exec, to);
    apply_all_coo(exec, out, s, "f", F.get(), to);
    info << "sorted_fresh " << F->is_sorted_by_row() << "\n";
}

void run_hybrid(exec_ptr exec, const std::string& dir, const scenario& s, std::ostream& info)
{
    using hybrid = gko::matrix::Hybrid<double, gko::int32>;
    const std::string out = dir + "/out/";
    const auto& from = load(dir, s.base);
    const auto& to = load(dir, s.payload);
    if (s.mutator != "convert_from_csr") throw std::runtime_error("unknown mutator " + s.mutator);
    auto limit = [] { return std::make_shared<hybrid::column_limit>(3); };  // rows longer than 3: a COO part exists
    auto H = hybrid::create(exec, limit());
    make_csr<double, gko::int32>(exec, from, "automatical")->convert_to(H.get());
    apply_all<double>(exec, out, s, "w", H.get(), from, true);
    info << "coo_nnz_warm " << H->get_coo_num_stored_elements() << "\n";
    make_csr<double, gko::int32>(exec, to, "automatical")->convert_to(H.get());
    apply_all<double>(exec, out, s, "y", H.get(), to, true);
    info << "coo_nnz_after " << H->get_coo_num_stored_elements() << "\n";
    auto F = hybrid::create(exec, limit());
    make_csr<double, gko::int32>(exec, to, "automatical")->convert_to(F.get());
    apply_all<double>(exec, out, s, "f", F.get(), to, true);
}

// a solver generated once and used twice (time stepping): the second solve must see the new values
void run_cg(exec_ptr exec, const std::string& dir, const scenario& s, std::ostream& info)
{
    using vec = gko::matrix::Dense<double>;
    const std::string out = dir + "/out/";
    const auto& from = load(dir, s.base);
    const auto& to = load(dir, s.payload);
    if (s.mutator != "values") throw std::runtime_error("unknown mutator " + s.mutator);
    auto factory = [&] {
        return gko::solver::Cg<double>::build()
            .with_criteria(gko::stop::Iteration::build().with_max_iters(1000u).on(exec),
                           gko::stop::ResidualNorm<double>::build().with_reduction_factor(1e-10).on(exec))
            .on(exec);
    };
    auto solve = [&](const gko::solver::Cg<double>* solver, const host_matrix& m, const std::string& tag) {
        auto b = to_device<double>(exec, m.b1, m.rows, 1);
        auto x = vec::create(exec, gko::dim<2>(m.rows, 1));
        x->fill(0.0);
        solver->apply(b.get(), x.get());
        write_raw(out + s.id + "." + tag + ".f64", to_host(x.get()));
        info << "iterations_" << tag << " " << solver->get_last_iteration_count() << "\nconverged_" << tag << " " << solver->has_converged() << "\n";
    };
    auto A = gko::share(make_csr<double, gko::int32>(exec, from, s.strategy));
    auto solver = factory()->generate(A);
    solve(solver.get(), from, "w1");
    upload(exec, to.v, A->get_values());
    solve(solver.get(), to, "y1");
    auto F = gko::share(make_csr<double, gko::int32>(exec, to, s.strategy));
    auto fresh = factory()->generate(F);
    solve(fresh.get(), to, "f1");
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::cerr << "usage: state_coherence <dir>\n";
        return 2;
    }
    const std::string dir = argv[1];
    try {
        auto exec = gko::HipExecutor::create(0, gko::OmpExecutor::create());
        std::ifstream list(dir + "/scenarios.txt");
        if (!list) throw std::runtime_error("no scenarios.txt in " + dir);
        std::string line;
        int done = 0;
        while (std::getline(list, line)) {
            if (line.empty()) continue;
            std::istringstream is(line);
            scenario s;
            if (!(is >> s.id >> s.object >> s.strategy >> s.mutator >> s.base >> s.payload >> s.three >> s.dump)) throw std::runtime_error("bad scenario line: " + line);
            std::ostringstream info;
            const bool special = s.mutator == "convert_from_float" || s.mutator == "transpose";
            if (s.object == "csr" && special) run_csr_special(exec, dir, s, info);
            else if (s.object == "csr") run_csr<double, gko::int32>(exec, dir, s, info);
            else if (s.object == "csr64") run_csr<double, gko::int64>(exec, dir, s, info);
            else if (s.object == "csrf") run_csr<float, gko::int32>(exec, dir, s, info);
            else if (s.object == "coo") run_coo(exec, dir, s, info);
            else if (s.object == "hybrid") run_hybrid(exec, dir, s, info);
            else if (s.object == "cg") run_cg(exec, dir, s, info);
            else throw std::runtime_error("unknown object " + s.object);
            exec->synchronize();
            std::ofstream(dir + "/out/" + s.id + ".info") << info.str();
            std::cout << "done " << s.id << std::endl;
            ++done;
        }
        std::cout << "scenarios " << done << "\n";
    } catch (const std::exception& e) {
        std::cerr << "state_coherence: " << e.what() << "\n";
        return 1;
    }
    return 0;
}
