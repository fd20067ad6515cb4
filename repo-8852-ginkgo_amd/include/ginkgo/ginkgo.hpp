// Host-side mirror of the Ginkgo public interface for the SpMV + Krylov hot
// path, on top of the C ABI in include/gkomi.h (header-only, C++14).
//
// It reproduces the names, argument meaning and error behaviour of the
// reference's operator interface so that code written against
// <ginkgo/ginkgo.hpp> for this path -- e.g. the reference's
// examples/simple-solver/simple-solver.cpp -- compiles and runs unchanged:
//   gko::Executor / OmpExecutor / ReferenceExecutor / HipExecutor
//     (include/ginkgo/core/base/executor.hpp:602-1017, 1591-1781),
//   gko::array, gko::dim, gko::LinOp, gko::LinOpFactory
//     (include/ginkgo/core/base/{array,dim,lin_op}.hpp),
//   gko::matrix::{Dense, Csr, Coo, Ell, Sellp, Hybrid},
//   gko::stop::{Iteration, ResidualNorm, Combined},
//   gko::solver::{Cg, Gmres, LowerTrs, UpperTrs},
//   gko::preconditioner::{Jacobi, Ilu}, gko::factorization::{ParIlu, ParIlut, ParIct},
//   gko::read / gko::write (MatrixMarket), gko::initialize, gko::share, lend.
//
// Kernels exist only for HipExecutor (the MI355X backend).  The host executors
// are memory spaces: running a kernel on them throws gko::NotCompiled, exactly
// what a Ginkgo build without the reference/omp modules does
// (core/device_hooks/common_kernels.inc.cpp:94).  Only fp64 values / int32
// indices are instantiated (north_star scope).
#ifndef GKOMI_GINKGO_HPP_
#define GKOMI_GINKGO_HPP_

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <cstdlib>
#include <functional>
#include <initializer_list>
#include <iomanip>
#include <iostream>
#include <istream>
#include <limits>
#include <memory>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../../include/gkomi.h"

namespace gko {

using size_type = std::size_t;
using int32 = std::int32_t;
using int64 = std::int64_t;
using uint8 = std::uint8_t;
using uint64 = std::uint64_t;
using uint32 = std::uint32_t;
template <typename T>
using remove_complex = T;
template <typename T>
constexpr T zero() { return T{}; }
template <typename T>
constexpr T one() { return T(1); }

// ---- exceptions (include/ginkgo/core/base/exception.hpp:86-632) -------------
class Error : public std::exception {
public:
    Error(const std::string& file, int line, const std::string& what)
        : what_(file + ":" + std::to_string(line) + ": " + what) {}
    const char* what() const noexcept override { return what_.c_str(); }
private:
    std::string what_;
};
#define GKOMI_DEFINE_ERROR(Name)                                              \
    class Name : public Error {                                               \
    public:                                                                   \
        Name(const std::string& f, int l, const std::string& w) : Error(f, l, #Name ": " + w) {} \
    }
GKOMI_DEFINE_ERROR(NotImplemented);
GKOMI_DEFINE_ERROR(NotCompiled);
GKOMI_DEFINE_ERROR(NotSupported);
GKOMI_DEFINE_ERROR(HipError);
GKOMI_DEFINE_ERROR(DimensionMismatch);
GKOMI_DEFINE_ERROR(BadDimension);
GKOMI_DEFINE_ERROR(AllocationError);
GKOMI_DEFINE_ERROR(StreamError);
GKOMI_DEFINE_ERROR(ValueMismatch);
#undef GKOMI_DEFINE_ERROR
#define GKO_NOT_COMPILED(module) throw ::gko::NotCompiled(__FILE__, __LINE__, #module " kernels are not part of this backend")
#define GKO_NOT_SUPPORTED(what) throw ::gko::NotSupported(__FILE__, __LINE__, what)
#define GKO_NOT_IMPLEMENTED throw ::gko::NotImplemented(__FILE__, __LINE__, __func__)

namespace detail {
// translate a C-ABI return code into the gko::Error family
inline void check(int code, const char* file, int line, const char* call)
{
    if (code == 0) return;
    const std::string msg = std::string(call) + ": " + gkomi_error_string(code);
    if (code > 0) throw HipError(file, line, msg);
    if (code == GKOMI_ENOTSUPPORTED) throw NotSupported(file, line, msg);
    if (code == GKOMI_ENOTIMPL) throw NotImplemented(file, line, msg);
    if (code == GKOMI_EINVAL) throw BadDimension(file, line, msg);
    throw Error(file, line, msg);
}
}  // namespace detail

class Executor;
// ---- logging hook (include/ginkgo/core/log/logger.hpp: operation_launched / operation_completed,
// fired by Executor::run around every kernel, executor.hpp:1153-1158).  Here every C-ABI call of
// the mirror is such an operation; its name is the entry point.  Loggers are attached with
// Executor::add_logger like in the reference; GKOMI_ROCTX=1 additionally brackets every operation
// with a roctx range for rocprofv3 --marker-trace.
namespace log {
class Logger {
public:
    virtual ~Logger() = default;
    virtual void on_operation_launched(const Executor*, const char* /*operation*/) const {}
    virtual void on_operation_completed(const Executor*, const char* /*operation*/) const {}
};
}  // namespace log

namespace detail {
struct logger_registry {
    std::vector<std::pair<const Executor*, std::shared_ptr<const log::Logger>>> loggers;
    bool roctx{false};
    logger_registry()
    {
        const char* v = std::getenv("GKOMI_ROCTX");
        roctx = v != nullptr && v[0] == '1' && gkomi_roctx_available();
    }
    bool active() const { return roctx || !loggers.empty(); }
};
inline logger_registry& registry()
{
    static logger_registry r;
    return r;
}
// "gkomi_csr_spmv_f64_i32(nullptr, ...)" -> "gkomi_csr_spmv_f64_i32"
inline std::string operation_name(const char* call)
{
    std::string s(call);
    const auto p = s.find('(');
    return p == std::string::npos ? s : s.substr(0, p);
}
struct operation_scope {
    explicit operation_scope(const char* call)
    {
        if (!registry().active()) return;
        name_ = operation_name(call);
        if (registry().roctx) gkomi_roctx_push(name_.c_str());
        for (const auto& l : registry().loggers) l.second->on_operation_launched(l.first, name_.c_str());
        armed_ = true;
    }
    ~operation_scope()
    {
        if (!armed_) return;
        for (const auto& l : registry().loggers) l.second->on_operation_completed(l.first, name_.c_str());
        if (registry().roctx) gkomi_roctx_pop();
    }
    std::string name_;
    bool armed_{false};
};
}  // namespace detail
#define GKOMI_CALL(expr)                                                   \
    do {                                                                   \
        ::gko::detail::operation_scope gkomi_scope_(#expr);                \
        ::gko::detail::check((expr), __FILE__, __LINE__, #expr);           \
    } while (0)

// ---- dim / version ------------------------------------------------------------
template <size_type N = 2>
struct dim {
    std::array<size_type, N> d{};
    dim() = default;
    dim(size_type s) { d.fill(s); }
    dim(size_type r, size_type c) { d[0] = r; d[1] = c; }
    size_type& operator[](size_type i) { return d[i]; }
    const size_type& operator[](size_type i) const { return d[i]; }
    explicit operator bool() const { return d[0] != 0 && d[1] != 0; }
    friend bool operator==(const dim& a, const dim& b) { return a.d == b.d; }
    friend bool operator!=(const dim& a, const dim& b) { return !(a == b); }
};
inline dim<2> transpose(const dim<2>& x) { return {x[1], x[0]}; }

class version_info {
public:
    static const version_info& get() { static version_info v; return v; }
    friend std::ostream& operator<<(std::ostream& os, const version_info&)
    {
        return os << "This is the MI355X-native hot-path backend with the Ginkgo 1.5.0 interface\n"
                  << "    running with core module 1.5.0 (hot path only)\n"
                  << "    the hip  module is   " << gkomi_version() << "\n"
                  << "    the reference/omp/cuda/dpcpp modules are not compiled";
    }
};

// ---- executors ------------------------------------------------------------------
class Executor : public std::enable_shared_from_this<Executor> {
public:
    virtual ~Executor() = default;
    virtual std::shared_ptr<Executor> get_master() noexcept = 0;
    virtual std::shared_ptr<const Executor> get_master() const noexcept = 0;
    virtual void synchronize() const = 0;
    virtual bool is_device() const noexcept = 0;
    template <typename T>
    T* alloc(size_type n) const { return static_cast<T*>(this->raw_alloc(n * sizeof(T))); }
    void free(void* p) const noexcept { this->raw_free(p); }
    template <typename T>
    void copy_from(const Executor* src_exec, size_type n, const T* src, T* dst) const
    {
        if (n == 0) return;
        const size_type bytes = n * sizeof(T);
        if (!src_exec->is_device() && !this->is_device()) {
            std::memcpy(dst, src, bytes);
        } else {
            const int kind = src_exec->is_device() ? (this->is_device() ? 2 : 1) : 0;
            GKOMI_CALL(gkomi_raw_copy(dst, src, bytes, kind));
        }
    }
    template <typename T>
    void copy(size_type n, const T* src, T* dst) const { this->copy_from(this, n, src, dst); }
    template <typename T>
    T copy_val_to_host(const T* ptr) const
    {
        T out{};
        this->get_master()->copy_from(this, 1, ptr, &out);
        return out;
    }
    // log::EnableLogging (include/ginkgo/core/log/logger.hpp:560-620)
    void add_logger(std::shared_ptr<const log::Logger> logger) const { detail::registry().loggers.emplace_back(this, std::move(logger)); }
    void remove_logger(const log::Logger* logger) const
    {
        auto& v = detail::registry().loggers;
        v.erase(std::remove_if(v.begin(), v.end(), [&](const std::pair<const Executor*, std::shared_ptr<const log::Logger>>& e) {
                    return e.first == this && e.second.get() == logger; }), v.end());
    }
protected:
    virtual void* raw_alloc(size_type bytes) const = 0;
    virtual void raw_free(void* p) const noexcept = 0;
};

class OmpExecutor : public Executor {
public:
    static std::shared_ptr<OmpExecutor> create() { return std::shared_ptr<OmpExecutor>(new OmpExecutor()); }
    std::shared_ptr<Executor> get_master() noexcept override { return this->shared_from_this(); }
    std::shared_ptr<const Executor> get_master() const noexcept override { return this->shared_from_this(); }
    void synchronize() const override {}
    bool is_device() const noexcept override { return false; }
protected:
    OmpExecutor() = default;
    void* raw_alloc(size_type bytes) const override
    {
        void* p = bytes ? std::malloc(bytes) : nullptr;
        if (bytes && !p) throw AllocationError(__FILE__, __LINE__, "host allocation failed");
        return p;
    }
    void raw_free(void* p) const noexcept override { std::free(p); }
};

class ReferenceExecutor : public OmpExecutor {
public:
    static std::shared_ptr<ReferenceExecutor> create() { return std::shared_ptr<ReferenceExecutor>(new ReferenceExecutor()); }
protected:
    ReferenceExecutor() = default;
};

enum class allocation_mode { device, unified_global, unified_host };

class HipExecutor : public Executor {
public:
    static std::shared_ptr<HipExecutor> create(int device_id, std::shared_ptr<Executor> master,
                                               bool device_reset = false,
                                               allocation_mode = allocation_mode::device)
    {
        (void)device_reset;
        if (device_id < 0 || device_id >= get_num_devices()) {
            throw HipError(__FILE__, __LINE__, "invalid device id " + std::to_string(device_id));
        }
        GKOMI_CALL(gkomi_set_device(device_id));
        auto e = std::shared_ptr<HipExecutor>(new HipExecutor(device_id, std::move(master)));
        int64_t prop[4] = {};
        GKOMI_CALL(gkomi_device_properties(device_id, prop));
        e->num_multiprocessor_ = static_cast<int>(prop[0]);
        e->warp_size_ = static_cast<int>(prop[1]);
        return e;
    }
    static int get_num_devices()
    {
        int n = 0;
        GKOMI_CALL(gkomi_get_num_devices(&n));
        return n;
    }
    std::shared_ptr<Executor> get_master() noexcept override { return master_; }
    std::shared_ptr<const Executor> get_master() const noexcept override { return master_; }
    void synchronize() const override { GKOMI_CALL(gkomi_synchronize(nullptr)); }
    bool is_device() const noexcept override { return true; }
    int get_device_id() const noexcept { return device_id_; }
    int get_num_multiprocessor() const noexcept { return num_multiprocessor_; }
    int get_warp_size() const noexcept { return warp_size_; }
    int get_num_warps_per_sm() const noexcept { return 4; }  // num_pu_per_cu on AMD
    int get_num_warps() const noexcept { return num_multiprocessor_ * 4; }
protected:
    HipExecutor(int id, std::shared_ptr<Executor> master) : device_id_(id), master_(std::move(master)) {}
    void* raw_alloc(size_type bytes) const override
    {
        void* p = nullptr;
        const int rc = gkomi_raw_alloc(bytes, &p);
        if (rc) throw AllocationError(__FILE__, __LINE__, std::string("hip: ") + gkomi_error_string(rc));
        return p;
    }
    void raw_free(void* p) const noexcept override
    {
        // like the reference: a failing free is fatal, never an exception
        if (gkomi_raw_free(p) != 0) { std::cerr << "Unrecoverable HIP error on hipFree\n"; std::exit(1); }
    }
private:
    int device_id_;
    std::shared_ptr<Executor> master_;
    int num_multiprocessor_{0};
    int warp_size_{64};
};

// backends outside this build: same factory signatures, NotCompiled on use
class CudaExecutor {
public:
    static std::shared_ptr<Executor> create(int, std::shared_ptr<Executor>, bool = false,
                                            allocation_mode = allocation_mode::device) { GKO_NOT_COMPILED(cuda); }
    static int get_num_devices() { return 0; }
};
class DpcppExecutor {
public:
    static std::shared_ptr<Executor> create(int, std::shared_ptr<Executor>, std::string = "all") { GKO_NOT_COMPILED(dpcpp); }
    static int get_num_devices(std::string = "all") { return 0; }
};

namespace detail {
inline void require_device(const std::shared_ptr<const Executor>& exec, const char* what)
{
    if (!exec->is_device()) {
        throw NotCompiled(__FILE__, __LINE__, std::string(what) +
                          ": only the hip (MI355X) kernels are compiled; reference/omp kernels are not part of this backend");
    }
}
}  // namespace detail

// ---- array ----------------------------------------------------------------------
template <typename T>
class array {
public:
    array() = default;
    explicit array(std::shared_ptr<const Executor> exec, size_type n = 0) : exec_(std::move(exec)) { resize_and_reset(n); }
    array(std::shared_ptr<const Executor> exec, std::initializer_list<T> init) : exec_(std::move(exec))
    {
        resize_and_reset(init.size());
        std::vector<T> tmp(init);
        auto host = exec_->get_master();
        exec_->copy_from(host.get(), tmp.size(), tmp.data(), data_);
    }
    template <typename It>
    array(std::shared_ptr<const Executor> exec, It b, It e) : exec_(std::move(exec))
    {
        std::vector<T> tmp(b, e);
        resize_and_reset(tmp.size());
        exec_->copy_from(exec_->get_master().get(), tmp.size(), tmp.data(), data_);
    }
    array(std::shared_ptr<const Executor> exec, const array& other) : exec_(std::move(exec)) { *this = other; }
    array(const array& other) : exec_(other.exec_) { *this = other; }
    array(array&& other) noexcept { *this = std::move(other); }
    ~array() { clear(); }
    array& operator=(const array& other)
    {
        if (this == &other) return *this;
        if (!exec_) exec_ = other.exec_;
        resize_and_reset(other.n_);
        if (n_) exec_->copy_from(other.exec_.get(), n_, other.data_, data_);
        return *this;
    }
    array& operator=(array&& other) noexcept
    {
        if (this == &other) return *this;
        if (exec_ && other.exec_ && exec_ != other.exec_) { *this = static_cast<const array&>(other); return *this; }
        clear();
        exec_ = other.exec_; data_ = other.data_; n_ = other.n_; owns_ = other.owns_;
        other.data_ = nullptr; other.n_ = 0;
        return *this;
    }
    static array view(std::shared_ptr<const Executor> exec, size_type n, T* data)
    {
        array a; a.exec_ = std::move(exec); a.data_ = data; a.n_ = n; a.owns_ = false; return a;
    }
    void resize_and_reset(size_type n)
    {
        if (n == n_) return;
        clear();
        if (n) data_ = exec_->template alloc<T>(n);
        n_ = n; owns_ = true;
    }
    void clear() noexcept
    {
        if (owns_ && data_ && exec_) exec_->free(data_);
        data_ = nullptr; n_ = 0;
    }
    void fill(T v)
    {
        std::vector<T> tmp(n_, v);
        exec_->copy_from(exec_->get_master().get(), n_, tmp.data(), data_);
    }
    void set_executor(std::shared_ptr<const Executor> exec)
    {
        if (exec == exec_) return;
        array tmp(exec, *this);  // copy of the data in the new memory space
        clear();
        exec_ = std::move(exec);
        data_ = tmp.data_; n_ = tmp.n_; owns_ = true;
        tmp.data_ = nullptr; tmp.n_ = 0;
    }
    T* get_data() noexcept { return data_; }
    const T* get_const_data() const noexcept { return data_; }
    size_type get_num_elems() const noexcept { return n_; }
    std::shared_ptr<const Executor> get_executor() const noexcept { return exec_; }
    std::vector<T> to_host() const
    {
        std::vector<T> out(n_);
        if (n_) exec_->get_master()->copy_from(exec_.get(), n_, data_, out.data());
        return out;
    }
private:
    std::shared_ptr<const Executor> exec_;
    T* data_{nullptr};
    size_type n_{0};
    bool owns_{true};
};
template <typename T>
array<T> make_array_view(std::shared_ptr<const Executor> exec, size_type n, T* data) { return array<T>::view(std::move(exec), n, data); }

// ---- pointer helpers --------------------------------------------------------------
template <typename T>
T* lend(const std::unique_ptr<T>& p) { return p.get(); }
template <typename T>
T* lend(const std::shared_ptr<T>& p) { return p.get(); }
template <typename T>
T* lend(T* p) { return p; }
template <typename T>
std::shared_ptr<T> share(std::unique_ptr<T>&& p) { return std::shared_ptr<T>(std::move(p)); }
template <typename T>
std::shared_ptr<T> share(std::shared_ptr<T> p) { return p; }
template <typename T>
std::unique_ptr<T> give(std::unique_ptr<T>&& p) { return std::move(p); }
// give(an lvalue): hands the object over, like the reference's std::move wrapper (utils_helper.hpp)
template <typename T>
std::unique_ptr<T> give(std::unique_ptr<T>& p) { return std::move(p); }
// gko::clone(exec, obj) (utils_helper.hpp): a copy of *obj on exec
template <typename Ptr>
auto clone(std::shared_ptr<const Executor> exec, const Ptr& p) -> decltype(p->clone(exec)) { return p->clone(std::move(exec)); }
template <typename Ptr>
auto clone(const Ptr& p) -> decltype(p->clone()) { return p->clone(); }
namespace detail {
// components::convert_precision<double <-> float> (core/components/precision_conversion_kernels.hpp:53)
inline int convert_precision(int64_t nrows, int64_t ncols, const double* in, int64_t in_stride, float* out, int64_t out_stride)
{
    return gkomi_dense_convert_f64_to_f32(nullptr, nrows, ncols, in, in_stride, out, out_stride);
}
inline int convert_precision(int64_t nrows, int64_t ncols, const float* in, int64_t in_stride, double* out, int64_t out_stride)
{
    return gkomi_dense_convert_f32_to_f64(nullptr, nrows, ncols, in, in_stride, out, out_stride);
}
}  // namespace detail
template <typename T, typename U>
T* as(U* p)
{
    auto r = dynamic_cast<T*>(p);
    if (!r) throw NotSupported(__FILE__, __LINE__, "object cannot be cast to the requested type");
    return r;
}

// ---- matrix_data + MatrixMarket I/O (include/ginkgo/core/base/mtx_io.hpp) -----------
template <typename V = double, typename I = int32>
struct matrix_data {
    struct nonzero_type {
        nonzero_type() = default;
        nonzero_type(I r, I c, V v) : row(r), column(c), value(v) {}
        I row{};
        I column{};
        V value{};
    };
    matrix_data() = default;
    explicit matrix_data(dim<2> size_) : size(size_) {}  // include/ginkgo/core/base/matrix_data.hpp:159 (no fill value: empty)
    dim<2> size;
    std::vector<nonzero_type> nonzeros;
    void ensure_row_major_order()
    {
        std::stable_sort(nonzeros.begin(), nonzeros.end(), [](const nonzero_type& a, const nonzero_type& b) {
            return std::tie(a.row, a.column) < std::tie(b.row, b.column);
        });
    }
    // include/ginkgo/core/base/matrix_data.hpp: remove_zeros / sum_duplicates
    void remove_zeros()
    {
        nonzeros.erase(std::remove_if(nonzeros.begin(), nonzeros.end(), [](const nonzero_type& e) { return e.value == V{}; }), nonzeros.end());
    }
    void sum_duplicates()
    {
        ensure_row_major_order();
        std::vector<nonzero_type> out;
        for (const auto& e : nonzeros) {
            if (out.empty() || out.back().row != e.row || out.back().column != e.column) out.push_back({e.row, e.column, V{}});
            out.back().value += e.value;
        }
        nonzeros = std::move(out);
    }
};

// ---- device_matrix_data (include/ginkgo/core/base/device_matrix_data.hpp:63-270) -------
// SoA triplets in the executor's memory; sort / de-duplicate / drop zeros run on
// the device (core/base/device_matrix_data.cpp:115-141 -> csrc/assembly.hip).
template <typename V = double, typename I = int32>
class device_matrix_data {
public:
    using value_type = V;
    using index_type = I;
    using host_type = matrix_data<V, I>;
    struct arrays { array<I> row_idxs; array<I> col_idxs; array<V> values; };
    explicit device_matrix_data(std::shared_ptr<const Executor> exec, dim<2> size = {}, size_type num_entries = 0)
        : size_(size), row_idxs_(exec, num_entries), col_idxs_(exec, num_entries), values_(exec, num_entries) {}
    device_matrix_data(std::shared_ptr<const Executor> exec, const device_matrix_data& data)
        : size_(data.size_), row_idxs_(exec, data.row_idxs_), col_idxs_(exec, data.col_idxs_), values_(exec, data.values_) {}
    device_matrix_data(dim<2> size, array<I> row_idxs, array<I> col_idxs, array<V> values)
        : size_(size), row_idxs_(std::move(row_idxs)), col_idxs_(std::move(col_idxs)), values_(std::move(values))
    {
        if (values_.get_num_elems() != row_idxs_.get_num_elems() || values_.get_num_elems() != col_idxs_.get_num_elems())
            throw BadDimension(__FILE__, __LINE__, "device_matrix_data: array sizes differ");
    }
    host_type copy_to_host() const
    {
        host_type result;
        result.size = size_;
        auto r = row_idxs_.to_host(); auto c = col_idxs_.to_host(); auto v = values_.to_host();
        result.nonzeros.resize(v.size());
        for (size_type i = 0; i < v.size(); ++i) result.nonzeros[i] = {r[i], c[i], v[i]};
        return result;
    }
    static device_matrix_data create_from_host(std::shared_ptr<const Executor> exec, const host_type& data)
    {
        std::vector<I> r(data.nonzeros.size()), c(data.nonzeros.size());
        std::vector<V> v(data.nonzeros.size());
        for (size_type i = 0; i < v.size(); ++i) { r[i] = data.nonzeros[i].row; c[i] = data.nonzeros[i].column; v[i] = data.nonzeros[i].value; }
        return device_matrix_data(data.size, array<I>(exec, r.begin(), r.end()), array<I>(exec, c.begin(), c.end()), array<V>(exec, v.begin(), v.end()));
    }
    void sort_row_major()
    {
        auto exec = device("components::sort_row_major");
        array<char> ws(exec, gkomi_matrix_data_workspace_bytes(get_num_elems()));
        GKOMI_CALL(gkomi_matrix_data_sort_row_major_f64_i32(nullptr, get_num_elems(), row_idxs_.get_data(), col_idxs_.get_data(), values_.get_data(),
                                                            ws.get_data(), ws.get_num_elems()));
    }
    void remove_zeros() { compact("components::remove_zeros", gkomi_matrix_data_remove_zeros_f64_i32); }
    void sum_duplicates()
    {
        sort_row_major();
        compact("components::sum_duplicates", gkomi_matrix_data_sum_duplicates_f64_i32);
    }
    std::shared_ptr<const Executor> get_executor() const { return values_.get_executor(); }
    dim<2> get_size() const { return size_; }
    size_type get_num_elems() const { return values_.get_num_elems(); }
    I* get_row_idxs() { return row_idxs_.get_data(); }
    const I* get_const_row_idxs() const { return row_idxs_.get_const_data(); }
    I* get_col_idxs() { return col_idxs_.get_data(); }
    const I* get_const_col_idxs() const { return col_idxs_.get_const_data(); }
    V* get_values() { return values_.get_data(); }
    const V* get_const_values() const { return values_.get_const_data(); }
    void resize_and_reset(size_type n) { row_idxs_.resize_and_reset(n); col_idxs_.resize_and_reset(n); values_.resize_and_reset(n); }
    void resize_and_reset(dim<2> new_size, size_type n) { size_ = new_size; resize_and_reset(n); }
    arrays empty_out()
    {
        arrays result{std::move(row_idxs_), std::move(col_idxs_), std::move(values_)};
        size_ = {};
        return result;
    }
private:
    std::shared_ptr<const Executor> device(const char* what) const
    {
        auto exec = get_executor();
        detail::require_device(exec, what);
        return exec;
    }
    template <typename Fn>
    void compact(const char* what, Fn kernel)
    {
        auto exec = device(what);
        const size_type n = get_num_elems();
        array<I> r(exec, n), c(exec, n);
        array<V> v(exec, n);
        array<char> ws(exec, gkomi_matrix_data_workspace_bytes(n));
        int64_t kept = 0;
        GKOMI_CALL(kernel(nullptr, n, row_idxs_.get_const_data(), col_idxs_.get_const_data(), values_.get_const_data(), r.get_data(), c.get_data(),
                          v.get_data(), ws.get_data(), ws.get_num_elems(), &kept));
        if (static_cast<size_type>(kept) == n) return;  // nothing removed: keep the arrays (no reallocation, as the reference)
        array<I> r2(exec, kept), c2(exec, kept);
        array<V> v2(exec, kept);
        if (kept) {
            exec->copy_from(exec.get(), kept, r.get_const_data(), r2.get_data());
            exec->copy_from(exec.get(), kept, c.get_const_data(), c2.get_data());
            exec->copy_from(exec.get(), kept, v.get_const_data(), v2.get_data());
        }
        row_idxs_ = std::move(r2); col_idxs_ = std::move(c2); values_ = std::move(v2);
    }
    dim<2> size_;
    array<I> row_idxs_;
    array<I> col_idxs_;
    array<V> values_;
};

template <typename V = double, typename I = int32>
matrix_data<V, I> read_raw(std::istream& is)
{
    std::string line;
    if (!std::getline(is, line)) throw StreamError(__FILE__, __LINE__, "empty MatrixMarket stream");
    std::istringstream hdr(line);
    std::string banner, object, layout, field, symmetry;
    hdr >> banner >> object >> layout >> field >> symmetry;
    std::transform(layout.begin(), layout.end(), layout.begin(), ::tolower);
    std::transform(field.begin(), field.end(), field.begin(), ::tolower);
    std::transform(symmetry.begin(), symmetry.end(), symmetry.begin(), ::tolower);
    if (banner != "%%MatrixMarket") throw StreamError(__FILE__, __LINE__, "not a MatrixMarket header");
    while (std::getline(is, line) && (line.empty() || line[0] == '%')) {}
    std::istringstream dims(line);
    matrix_data<V, I> data;
    if (layout == "array") {
        size_type r, c;
        dims >> r >> c;
        data.size = dim<2>(r, c);
        for (size_type j = 0; j < c; ++j) {
            for (size_type i = 0; i < r; ++i) {
                double v;
                if (!(is >> v)) throw StreamError(__FILE__, __LINE__, "truncated array data");
                if (v != 0.0) data.nonzeros.push_back({static_cast<I>(i), static_cast<I>(j), static_cast<V>(v)});
            }
        }
    } else {
        size_type r, c, nnz;
        dims >> r >> c >> nnz;
        data.size = dim<2>(r, c);
        for (size_type k = 0; k < nnz; ++k) {
            long long i, j;
            double v = 1.0;
            is >> i >> j;
            if (field != "pattern") is >> v;
            if (!is) throw StreamError(__FILE__, __LINE__, "truncated coordinate data");
            data.nonzeros.push_back({static_cast<I>(i - 1), static_cast<I>(j - 1), static_cast<V>(v)});
            if (symmetry == "symmetric" && i != j) {
                data.nonzeros.push_back({static_cast<I>(j - 1), static_cast<I>(i - 1), static_cast<V>(v)});
            }
        }
    }
    data.ensure_row_major_order();
    return data;
}

// ---- LinOp ------------------------------------------------------------------------
namespace matrix {
template <typename V>
class Dense;
}

class LinOp {
public:
    virtual ~LinOp() = default;
    // lin_op.hpp:158-224: validate, then apply_impl
    LinOp* apply(const LinOp* b, LinOp* x)
    {
        this->validate(b, x);
        this->apply_impl(b, x);
        return this;
    }
    const LinOp* apply(const LinOp* b, LinOp* x) const
    {
        this->validate(b, x);
        this->apply_impl(b, x);
        return this;
    }
    const LinOp* apply(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const
    {
        this->validate(b, x);
        if (alpha->get_size() != dim<2>(1, 1) || beta->get_size() != dim<2>(1, 1)) {
            throw DimensionMismatch(__FILE__, __LINE__, "alpha and beta must be 1x1");
        }
        this->apply_impl(alpha, b, beta, x);
        return this;
    }
    const dim<2>& get_size() const noexcept { return size_; }
    std::shared_ptr<const Executor> get_executor() const noexcept { return exec_; }
    // lin_op.hpp:255: does apply(b, x) read x?  false unless a solver says otherwise
    virtual bool apply_uses_initial_guess() const { return false; }
protected:
    LinOp(std::shared_ptr<const Executor> exec, const dim<2>& size = dim<2>{}) : exec_(std::move(exec)), size_(size) {}
    void set_size(const dim<2>& s) { size_ = s; }
    virtual void apply_impl(const LinOp* b, LinOp* x) const = 0;
    virtual void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const = 0;
    void validate(const LinOp* b, const LinOp* x) const
    {
        // GKO_ASSERT_CONFORMANT / EQUAL_ROWS / EQUAL_COLS (lin_op.hpp:323-345)
        if (size_[1] != b->get_size()[0] || size_[0] != x->get_size()[0] || b->get_size()[1] != x->get_size()[1]) {
            std::ostringstream os;
            os << "apply: operator " << size_[0] << "x" << size_[1] << ", b " << b->get_size()[0] << "x" << b->get_size()[1]
               << ", x " << x->get_size()[0] << "x" << x->get_size()[1];
            throw DimensionMismatch(__FILE__, __LINE__, os.str());
        }
    }
    std::shared_ptr<const Executor> exec_;
    dim<2> size_;
};

class LinOpFactory {
public:
    virtual ~LinOpFactory() = default;
    virtual std::unique_ptr<LinOp> generate_impl(std::shared_ptr<const LinOp> input) const = 0;
    std::shared_ptr<const Executor> get_executor() const noexcept { return exec_; }
protected:
    explicit LinOpFactory(std::shared_ptr<const Executor> exec) : exec_(std::move(exec)) {}
    std::shared_ptr<const Executor> exec_;
};

// include/ginkgo/core/base/lin_op.hpp:433-455 (real values: conj_transpose == transpose)
class Transposable {
public:
    virtual ~Transposable() = default;
    virtual std::unique_ptr<LinOp> transpose() const = 0;
    virtual std::unique_ptr<LinOp> conj_transpose() const { return this->transpose(); }
};

namespace detail {
// dense::simple_apply / apply and dense::transpose (gkomi_dense_gemm_f64, gkomi_dense_transpose_f64); double only:
// the reference executor arbitrates no float GEMM here
inline void dense_gemm(std::shared_ptr<const Executor> exec, int64_t m, int64_t n, int64_t k, const double* a, int64_t a_stride,
                       const double* b, int64_t b_stride, double* c, int64_t c_stride, const double* alpha, const double* beta)
{
    array<char> ws(exec, gkomi_dense_gemm_workspace_bytes(m, n, k, 0) + 8);
    GKOMI_CALL(gkomi_dense_gemm_f64(nullptr, m, n, k, a, a_stride, b, b_stride, c, c_stride, alpha, beta, 0, ws.get_data(), ws.get_num_elems()));
}
inline void dense_gemm(std::shared_ptr<const Executor>, int64_t, int64_t, int64_t, const float*, int64_t, const float*, int64_t, float*,
                       int64_t, const float*, const float*) { GKO_NOT_IMPLEMENTED; }
inline void dense_transpose(int64_t nrows, int64_t ncols, const double* in, int64_t in_stride, double* out, int64_t out_stride)
{
    GKOMI_CALL(gkomi_dense_transpose_f64(nullptr, nrows, ncols, in, in_stride, out, out_stride));
}
inline void dense_transpose(int64_t, int64_t, const float*, int64_t, float*, int64_t) { GKO_NOT_IMPLEMENTED; }
}  // namespace detail

// ---- matrix formats -----------------------------------------------------------------
namespace matrix {

template <typename V = double>
class Dense : public LinOp, public Transposable {
public:
    using value_type = V;
    static std::unique_ptr<Dense> create(std::shared_ptr<const Executor> exec, const dim<2>& size = dim<2>{}, size_type stride = 0)
    {
        return std::unique_ptr<Dense>(new Dense(std::move(exec), size, stride ? stride : size[1]));
    }
    // view over existing memory (Dense::create(exec, size, array view, stride))
    static std::unique_ptr<Dense> create(std::shared_ptr<const Executor> exec, const dim<2>& size, array<V> values, size_type stride)
    {
        auto d = std::unique_ptr<Dense>(new Dense(std::move(exec), dim<2>{}, 0));
        d->values_ = std::move(values);
        d->stride_ = stride;
        d->set_size(size);
        return d;
    }
    V* get_values() noexcept { return values_.get_data(); }
    const V* get_const_values() const noexcept { return values_.get_const_data(); }
    size_type get_stride() const noexcept { return stride_; }
    size_type get_num_stored_elements() const noexcept { return values_.get_num_elems(); }
    // host access only (like the reference: undefined on device memory)
    V& at(size_type r, size_type c = 0) { return values_.get_data()[r * stride_ + c]; }
    V at(size_type r, size_type c = 0) const { return values_.get_const_data()[r * stride_ + c]; }

    void fill(V v)
    {
        if (on_device()) GKOMI_CALL(gkomi_dense_fill_f64(nullptr, rows(), cols(), get_values(), stride_, v));
        else for (size_type i = 0; i < size_[0]; ++i) for (size_type j = 0; j < size_[1]; ++j) at(i, j) = v;
    }
    void copy_from(const Dense* other)
    {
        if (other->get_size() != size_ || other->get_stride() != stride_) {
            values_.resize_and_reset(other->get_size()[0] * other->get_stride());
            stride_ = other->get_stride();
            set_size(other->get_size());
        }
        exec_->copy_from(other->get_executor().get(), values_.get_num_elems(), other->get_const_values(), get_values());
    }
    std::unique_ptr<Dense> clone(std::shared_ptr<const Executor> exec = nullptr) const
    {
        auto d = Dense::create(exec ? exec : exec_, size_, stride_);
        d->copy_from(this);
        return d;
    }
    // Dense<double> <-> Dense<float> (core/matrix/dense.cpp convert_to(Dense<next_precision>*)): components::convert_precision
    template <typename W, typename = typename std::enable_if<!std::is_same<W, V>::value>::type>
    void convert_to(Dense<W>* result) const
    {
        kernel("components::convert_precision");
        if (result->get_size() != size_) {
            result->values_ = array<W>(result->get_executor(), size_[0] * size_[1]);
            result->stride_ = size_[1];
            result->set_size(size_);
        }
        GKOMI_CALL(::gko::detail::convert_precision(rows(), cols(), get_const_values(), stride_, result->get_values(), result->get_stride()));
    }
    template <typename W, typename = typename std::enable_if<!std::is_same<W, V>::value>::type>
    void move_to(Dense<W>* result) { convert_to(result); }
    void convert_to(Dense* result) const { result->copy_from(this); }
    void move_to(Dense* result) { result->copy_from(this); }
    void scale(const Dense* alpha) { kernel("dense::scale"); GKOMI_CALL(gkomi_dense_scale_f64(nullptr, rows(), cols(), alpha->get_const_values(), alpha->cols(), get_values(), stride_)); }
    void inv_scale(const Dense* alpha) { kernel("dense::inv_scale"); GKOMI_CALL(gkomi_dense_inv_scale_f64(nullptr, rows(), cols(), alpha->get_const_values(), alpha->cols(), get_values(), stride_)); }
    void add_scaled(const Dense* alpha, const Dense* b)
    {
        kernel("dense::add_scaled"); same_size(b);
        GKOMI_CALL(gkomi_dense_add_scaled_f64(nullptr, rows(), cols(), alpha->get_const_values(), alpha->cols(), b->get_const_values(), b->get_stride(), get_values(), stride_));
    }
    void sub_scaled(const Dense* alpha, const Dense* b)
    {
        kernel("dense::sub_scaled"); same_size(b);
        GKOMI_CALL(gkomi_dense_sub_scaled_f64(nullptr, rows(), cols(), alpha->get_const_values(), alpha->cols(), b->get_const_values(), b->get_stride(), get_values(), stride_));
    }
    void compute_dot(const Dense* b, Dense* result) const
    {
        kernel("dense::compute_dot"); same_size(b); result_size(result);
        array<char> tmp(exec_, gkomi_dense_reduction_workspace_bytes(rows(), cols()) + 8);
        GKOMI_CALL(gkomi_dense_compute_dot_f64(nullptr, rows(), cols(), get_const_values(), stride_, b->get_const_values(), b->get_stride(), result->get_values(), tmp.get_data(), tmp.get_num_elems()));
    }
    void compute_conj_dot(const Dense* b, Dense* result) const { compute_dot(b, result); }
    void compute_norm2(Dense* result) const
    {
        kernel("dense::compute_norm2"); result_size(result);
        array<char> tmp(exec_, gkomi_dense_reduction_workspace_bytes(rows(), cols()) + 8);
        GKOMI_CALL(gkomi_dense_compute_norm2_f64(nullptr, rows(), cols(), get_const_values(), stride_, result->get_values(), tmp.get_data(), tmp.get_num_elems()));
    }
    void read(const matrix_data<V, int32>& data)
    {
        values_.set_executor(exec_->get_master());
        values_.resize_and_reset(data.size[0] * data.size[1]);
        stride_ = data.size[1];
        set_size(data.size);
        std::fill_n(values_.get_data(), values_.get_num_elems(), V{});
        for (const auto& e : data.nonzeros) values_.get_data()[e.row * stride_ + e.column] = e.value;
        values_.set_executor(exec_);
    }
    void write(matrix_data<V, int32>& data) const
    {
        auto host = values_.to_host();
        data.size = size_;
        data.nonzeros.clear();
        for (size_type i = 0; i < size_[0]; ++i) for (size_type j = 0; j < size_[1]; ++j) {
            data.nonzeros.push_back({static_cast<int32>(i), static_cast<int32>(j), host[i * stride_ + j]});
        }
    }
    // core/matrix/dense.cpp:993-1030
    std::unique_ptr<LinOp> transpose() const override
    {
        auto t = Dense::create(exec_, dim<2>(size_[1], size_[0]));
        this->transpose(t.get());
        return std::unique_ptr<LinOp>(std::move(t));
    }
    std::unique_ptr<LinOp> conj_transpose() const override { return this->transpose(); }
    void transpose(Dense* output) const
    {
        kernel("dense::transpose");
        if (output->get_size() != dim<2>(size_[1], size_[0])) throw DimensionMismatch(__FILE__, __LINE__, "transpose: output must be #columns x #rows");
        ::gko::detail::dense_transpose(rows(), cols(), get_const_values(), stride_, output->get_values(), output->get_stride());
    }
    void conj_transpose(Dense* output) const { this->transpose(output); }
    int64_t rows() const { return static_cast<int64_t>(size_[0]); }
    int64_t cols() const { return static_cast<int64_t>(size_[1]); }
protected:
    Dense(std::shared_ptr<const Executor> exec, const dim<2>& size, size_type stride)
        : LinOp(exec, size), values_(exec, size[0] * stride), stride_(stride) {}
    bool on_device() const { return exec_->is_device(); }
    void kernel(const char* name) const { detail::require_device(exec_, name); }
    void same_size(const Dense* b) const { if (b->get_size() != size_) throw DimensionMismatch(__FILE__, __LINE__, "operands differ in size"); }
    void result_size(const Dense* r) const { if (r->get_size() != dim<2>(1, size_[1])) throw DimensionMismatch(__FILE__, __LINE__, "result must be 1 x #columns"); }
    // core/matrix/dense.cpp:88-114: dense::simple_apply / dense::apply, the reference's sums (include/gkomi.h)
    void apply_impl(const LinOp* b, LinOp* x) const override { gemm(nullptr, b, nullptr, x); }
    void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const override
    {
        gemm(as<const Dense>(alpha), b, as<const Dense>(beta), x);
    }
    void gemm(const Dense* alpha, const LinOp* b, const Dense* beta, LinOp* x) const
    {
        kernel("dense::apply");
        auto db = as<const Dense>(b);
        auto dx = as<Dense>(x);
        ::gko::detail::dense_gemm(exec_, rows(), dx->cols(), cols(), get_const_values(), stride_, db->get_const_values(), db->get_stride(),
                                  dx->get_values(), dx->get_stride(), alpha ? alpha->get_const_values() : nullptr,
                                  beta ? beta->get_const_values() : nullptr);
    }
    array<V> values_;
    size_type stride_;
    template <typename>
    friend class Dense;
};

namespace detail_fmt {
inline const Dense<double>* dense(const LinOp* op) { return as<const Dense<double>>(op); }
inline Dense<double>* dense(LinOp* op) { return as<Dense<double>>(op); }
}  // namespace detail_fmt

// gko::matrix::Identity (include/ginkgo/core/matrix/identity.hpp, core/matrix/identity.cpp:46-60): x = b, and as the
// operand of Csr::apply(alpha, I, beta, x) the mark of a sparse matrix sum
template <typename V = double>
class Identity : public LinOp {
public:
    using value_type = V;
    static std::unique_ptr<Identity> create(std::shared_ptr<const Executor> exec, size_type n = 0)
    {
        return std::unique_ptr<Identity>(new Identity(std::move(exec), n));
    }
protected:
    Identity(std::shared_ptr<const Executor> exec, size_type n) : LinOp(std::move(exec), dim<2>(n, n)) {}
    void apply_impl(const LinOp* b, LinOp* x) const override { as<Dense<V>>(x)->copy_from(as<const Dense<V>>(b)); }
    void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const override
    {
        auto dx = as<Dense<V>>(x);
        dx->scale(as<const Dense<V>>(beta));
        dx->add_scaled(as<const Dense<V>>(alpha), as<const Dense<V>>(b));
    }
};

template <typename V, typename I>
class Coo;
template <typename V, typename I>
class Ell;
template <typename V, typename I>
class Fbcsr;
template <typename V, typename I>
class Sellp;
template <typename V, typename I>
class Hybrid;
template <typename V, typename I>
class CsrBuilder;

namespace detail_abi {
// the C-ABI entry points of the two index types this backend instantiates for the SpMV path
// (GKO_INSTANTIATE_FOR_EACH_VALUE_AND_INDEX_TYPE, include/ginkgo/core/base/types.hpp:544-560: <double, int32> and
// <double, int64>; the other format / factorisation kernels exist for int32 only and do not compile for int64)
template <typename I>
struct csr_abi;
template <>
struct csr_abi<int32> {
    static constexpr auto spmv_srow = &gkomi_csr_spmv_srow_f64_i32;
    static constexpr auto make_srow = &gkomi_csr_make_srow_i32;
    static constexpr auto max_row_nnz = &gkomi_csr_max_row_nnz_i32;
    static constexpr auto idxs_to_ptrs = &gkomi_convert_idxs_to_ptrs_i32;
    // the column-pattern statistic of the strategy objects (GKOMI_CSR_COLBLOCK or 0): blocking, once per matrix
    static int gather_flags(int64_t ncols, int64_t nnz, const int32* col_idxs, double* scratch, int64_t* footprint)
    {
        int flags = 0;
        GKOMI_CALL(gkomi_csr_analyse_gather_i32(nullptr, ncols, nnz, col_idxs, scratch, &flags, footprint));
        return flags;
    }
    // the column-partitioned copy of the "gkomi_partitioned" strategy (gkomi_csr_colpart_*): nullptr = does not pay
    static gkomi_csr_colpart* colpart_create(std::shared_ptr<const Executor> exec, int64_t nrows, int64_t ncols, int64_t nnz, const int32* rp,
                                             const int32* ci, const double* v, array<char>& plan, int blocks)
    {
        if (blocks == 0 && gkomi_csr_colpart_blocks_for(nrows, ncols, nnz) == 0) return nullptr;
        plan = array<char>(exec, gkomi_csr_colpart_plan_bytes(nrows, nnz, blocks));
        gkomi_csr_colpart* h = nullptr;  // (0 blocks: the analysis times two block counts and keeps the faster)
        const int rc = gkomi_csr_colpart_create_f64_i32(nullptr, nrows, ncols, nnz, rp, ci, v, blocks, plan.get_data(), plan.get_num_elems(), &h);
        if (rc == GKOMI_ENOTSUPPORTED && blocks == 0) {  // timed against the matrix's own kernel: the copy does not pay
            plan = array<char>(exec, 0);
            return nullptr;
        }
        GKOMI_CALL(rc);
        return h;
    }
};
template <>
struct csr_abi<int64> {
    static constexpr auto spmv_srow = &gkomi_csr_spmv_srow_f64_i64;
    static constexpr auto make_srow = &gkomi_csr_make_srow_i64;
    static constexpr auto max_row_nnz = &gkomi_csr_max_row_nnz_i64;
    static constexpr auto idxs_to_ptrs = &gkomi_convert_idxs_to_ptrs_i64;
    static int gather_flags(int64_t, int64_t, const int64*, double*, int64_t* footprint)  // (column windows: int32 kernels only)
    {
        *footprint = 0;
        return 0;
    }
    static gkomi_csr_colpart* colpart_create(std::shared_ptr<const Executor>, int64_t, int64_t, int64_t, const int64*, const int64*, const double*,
                                             array<char>&, int)
    {
        return nullptr;
    }
};
}  // namespace detail_abi

template <typename V = double, typename I = int32>
class Csr : public LinOp {
    friend class CsrBuilder<V, I>;
public:
    using value_type = V;
    using index_type = I;
    using mat_data = matrix_data<V, I>;
    // kernel selection objects (include/ginkgo/core/matrix/csr.hpp:170-705)
    class strategy_type {
    public:
        explicit strategy_type(std::string name, int code, int partition_blocks = 0) : name_(std::move(name)), code_(code), partition_blocks_(partition_blocks) {}
        virtual ~strategy_type() = default;
        const std::string& get_name() const { return name_; }
        int get_code() const { return code_; }
        // gkomi_partitioned(blocks): the forced block count of the column-partitioned copy, 0 = the timed analysis decides
        int get_partition_blocks() const { return partition_blocks_; }
    private:
        std::string name_;
        int code_;
        int partition_blocks_;
    };
    struct classical : strategy_type { classical() : strategy_type("classical", GKOMI_CSR_VECTOR) {} };
    struct load_balance : strategy_type {
        load_balance(int64_t = 0) : strategy_type("load_balance", GKOMI_CSR_BALANCED) {}
        // include/ginkgo/core/matrix/csr.hpp:355-372: built from an executor (its warp count sized the reference's srow)
        template <typename Exec>
        load_balance(std::shared_ptr<Exec>) : load_balance(int64_t{0}) {}
    };
    struct merge_path : strategy_type { merge_path() : strategy_type("merge_path", GKOMI_CSR_STREAM) {} };
    struct automatical : strategy_type {
        automatical(int64_t = 0) : strategy_type("automatical", GKOMI_CSR_AUTO) {}
        template <typename Exec>
        automatical(std::shared_ptr<Exec>) : automatical(int64_t{0}) {}  // csr.hpp:571-588
    };
    // the vendor-library strategy (csr.hpp:299-330): no hipSPARSE behind this backend, the automatic choice serves it
    struct sparselib : strategy_type { sparselib() : strategy_type("sparselib", GKOMI_CSR_AUTO) {} };
    // An analysis-based strategy of this backend (the role hipSPARSE's analysis plays behind `sparselib` in the reference):
    // the matrix keeps a column-partitioned COPY (gkomi_csr_colpart_*, csrc/csr_colpart.hip) when its column pattern is
    // scattered and its shape fits, and applies one-column products through it (1.3-1.6 x on uniformly random / power-law
    // patterns of ~1 M columns; tolerance parity like load_balance); otherwise the automatic kernels.  The copy holds
    // values: it is re-gathered after get_values() (non-const) was asked for, and dropped and rebuilt after anything that
    // can change the pattern (get_col_idxs(), get_row_ptrs(), sort_by_column_index(), read, set_strategy, ...).
    // gkomi_partitioned() lets the analysis decide: it TIMES two block counts against the matrix's own kernel and may
    // decline, so whether a copy exists (and its summation association) can differ from run to run.
    // gkomi_partitioned(blocks), blocks in {2, 4, 8}, pins it: the copy is built with that many column blocks whatever
    // the shape, the column statistic or a timing say (reproducible runs, tests); an unusable count throws.
    struct gkomi_partitioned : strategy_type {
        explicit gkomi_partitioned(int blocks = 0) : strategy_type("gkomi_partitioned", GKOMI_CSR_AUTO, blocks) {}
    };
    struct cusparse : strategy_type { cusparse() : strategy_type("cusparse", GKOMI_CSR_AUTO) {} };

    static std::unique_ptr<Csr> create(std::shared_ptr<const Executor> exec, const dim<2>& size = dim<2>{}, size_type nnz = 0,
                                       std::shared_ptr<strategy_type> strategy = std::make_shared<automatical>())
    {
        return std::unique_ptr<Csr>(new Csr(std::move(exec), size, nnz, std::move(strategy)));
    }
    // include/ginkgo/core/matrix/csr.hpp:1036-1039: an empty matrix with a strategy
    static std::unique_ptr<Csr> create(std::shared_ptr<const Executor> exec, std::shared_ptr<strategy_type> strategy)
    {
        return std::unique_ptr<Csr>(new Csr(std::move(exec), dim<2>{}, 0, std::move(strategy)));
    }
    // The non-const getters tell the matrix that the array is about to change: what is cached from it (srow, the row and
    // column statistics, the column-partitioned copy) is rebuilt or re-gathered by the NEXT apply.  A pointer obtained
    // from them is therefore good for writing UNTIL THE NEXT APPLY; to write again after an apply, ask again.  (Writes
    // through a pointer saved across an apply are not seen by the caches.)
    V* get_values() noexcept { colpart_dirty_ = true; return values_.get_data(); }
    const V* get_const_values() const noexcept { return values_.get_const_data(); }
    I* get_col_idxs() noexcept { invalidate_srow(); return col_idxs_.get_data(); }  // the column statistic and the copy go with srow
    const I* get_const_col_idxs() const noexcept { return col_idxs_.get_const_data(); }
    I* get_row_ptrs() noexcept { invalidate_srow(); max_row_nnz_ = -1; return row_ptrs_.get_data(); }  // the caller may rewrite them
    const I* get_const_row_ptrs() const noexcept { return row_ptrs_.get_const_data(); }
    size_type get_num_stored_elements() const noexcept { return values_.get_num_elems(); }
    std::shared_ptr<strategy_type> get_strategy() const noexcept { return strategy_; }
    void set_strategy(std::shared_ptr<strategy_type> s) { strategy_ = std::move(s); invalidate_srow(); }  // the copy and the column statistic depend on it
    int64_t get_max_row_nnz() const noexcept { return max_row_nnz_; }

    // Csr::read(matrix_data) (core/matrix/csr.cpp:438-470)
    void read(const mat_data& data)
    {
        const size_type nnz = data.nonzeros.size();
        std::vector<I> rp(data.size[0] + 1, 0), ci(nnz);
        std::vector<V> v(nnz);
        for (size_type k = 0; k < nnz; ++k) {
            rp[data.nonzeros[k].row + 1]++;
            ci[k] = data.nonzeros[k].column;
            v[k] = data.nonzeros[k].value;
        }
        int64_t mx = 0;
        for (size_type r = 0; r < data.size[0]; ++r) { mx = std::max<int64_t>(mx, rp[r + 1]); rp[r + 1] += rp[r]; }
        max_row_nnz_ = mx;
        auto host = exec_->get_master();
        row_ptrs_ = array<I>(exec_, rp.begin(), rp.end());
        col_idxs_ = array<I>(exec_, ci.begin(), ci.end());
        values_ = array<V>(exec_, v.begin(), v.end());
        set_size(data.size);
        invalidate_srow();
    }
    // Csr::read(device_matrix_data) (core/matrix/csr.cpp:445-470): takes the
    // arrays over as they are (row-major order is the caller's job) and builds
    // row_ptrs with convert_idxs_to_ptrs on the device
    using device_mat_data = device_matrix_data<V, I>;
    void read(const device_mat_data& data) { this->read(device_mat_data{exec_, data}); }
    void read(device_mat_data&& data)
    {
        detail::require_device(exec_, "csr::convert_idxs_to_ptrs");
        const auto size = data.get_size();
        auto arrays = data.empty_out();
        arrays.row_idxs.set_executor(exec_); arrays.col_idxs.set_executor(exec_); arrays.values.set_executor(exec_);
        row_ptrs_.resize_and_reset(size[0] + 1);
        set_size(size);
        values_ = std::move(arrays.values);
        col_idxs_ = std::move(arrays.col_idxs);
        array<char> ws(exec_, gkomi_prefix_sum_workspace_bytes(size[0] + 1));
        GKOMI_CALL(detail_abi::csr_abi<I>::idxs_to_ptrs(nullptr, arrays.row_idxs.get_const_data(), arrays.row_idxs.get_num_elems(), size[0], row_ptrs_.get_data(),
                                                    ws.get_data(), ws.get_num_elems()));
        max_row_nnz_ = -1;
        invalidate_srow();
    }
    void write(mat_data& data) const
    {
        auto rp = row_ptrs_.to_host(); auto ci = col_idxs_.to_host(); auto v = values_.to_host();
        data.size = size_;
        data.nonzeros.clear();
        for (size_type r = 0; r < size_[0]; ++r) for (I k = rp[r]; k < rp[r + 1]; ++k) data.nonzeros.push_back({static_cast<I>(r), ci[k], v[k]});
    }
    // Csr<double, int32> <-> Csr<float, int32> (core/matrix/csr.cpp convert_to(Csr<next_precision>*)): the indices copied,
    // the values through components::convert_precision (nnz x 1), the strategy carried over
    template <typename W, typename = typename std::enable_if<!std::is_same<W, V>::value>::type>
    void convert_to(Csr<W, I>* result) const
    {
        static_assert(std::is_same<I, int32>::value, "precision conversion: int32 indices");
        detail::require_device(exec_, "components::convert_precision");
        const size_type nnz = get_num_stored_elements();
        auto rexec = result->get_executor();
        array<I> rp(rexec, size_[0] + 1), ci(rexec, nnz);
        array<W> v(rexec, nnz);
        exec_->copy(size_[0] + 1, get_const_row_ptrs(), rp.get_data());
        exec_->copy(nnz, get_const_col_idxs(), ci.get_data());
        GKOMI_CALL(::gko::detail::convert_precision(static_cast<int64_t>(nnz), 1, get_const_values(), 1, v.get_data(), 1));
        result->adopt(size_, std::move(rp), std::move(ci), std::move(v));
        result->set_strategy(std::make_shared<typename Csr<W, I>::strategy_type>(strategy_->get_name(), strategy_->get_code(), strategy_->get_partition_blocks()));
        result->max_row_nnz_ = max_row_nnz_;
    }
    template <typename W, typename = typename std::enable_if<!std::is_same<W, V>::value>::type>
    void move_to(Csr<W, I>* result) { convert_to(result); }
    void convert_to(Coo<V, I>* result) const;
    void convert_to(Ell<V, I>* result) const;
    void convert_to(Sellp<V, I>* result) const;
    void convert_to(Hybrid<V, I>* result) const;
    void convert_to(Fbcsr<V, I>* result) const;   // the block size is the target's (core/matrix/csr.cpp)
    std::unique_ptr<Csr> transpose() const
    {
        detail::require_device(exec_, "csr::transpose");
        auto t = Csr::create(exec_, gko::transpose(size_), get_num_stored_elements(), strategy_);
        array<char> ws(exec_, gkomi_csr_transpose_workspace_bytes(size_[1]));
        GKOMI_CALL(gkomi_csr_transpose_f64_i32(nullptr, size_[0], size_[1], get_num_stored_elements(), get_const_row_ptrs(), get_const_col_idxs(),
                                               get_const_values(), t->get_row_ptrs(), t->get_col_idxs(), t->get_values(), ws.get_data(), ws.get_num_elems()));
        t->max_row_nnz_ = -1;
        return t;
    }
    // Csr::compute_absolute (core/matrix/csr.cpp): the same pattern and strategy, |values|
    std::unique_ptr<Csr> compute_absolute() const
    {
        static_assert(std::is_same<V, double>::value && std::is_same<I, int32>::value, "compute_absolute: <double, int32> only");
        detail::require_device(exec_, "csr::compute_absolute");
        const size_type nnz = get_num_stored_elements();
        auto result = Csr::create(exec_, size_, nnz, strategy_);
        exec_->copy(size_[0] + 1, get_const_row_ptrs(), result->get_row_ptrs());
        exec_->copy(nnz, get_const_col_idxs(), result->get_col_idxs());
        GKOMI_CALL(gkomi_csr_compute_absolute_f64_i32(nullptr, static_cast<int64_t>(nnz), get_const_values(), result->get_values()));
        result->max_row_nnz_ = max_row_nnz_;
        return result;
    }
    // csr::sort_by_column_index / is_sorted_by_column_index (core/matrix/csr.cpp)
    void sort_by_column_index()
    {
        detail::require_device(exec_, "csr::sort_by_column_index");
        GKOMI_CALL(gkomi_csr_sort_by_column_index_f64_i32(nullptr, size_[0], get_const_row_ptrs(), get_col_idxs(), get_values()));
    }
    bool is_sorted_by_column_index() const
    {
        detail::require_device(exec_, "csr::is_sorted_by_column_index");
        array<char> ws(exec_, 8);
        int sorted = 1;
        GKOMI_CALL(gkomi_csr_is_sorted_by_column_index_i32(nullptr, size_[0], get_const_row_ptrs(), get_const_col_idxs(), ws.get_data(), ws.get_num_elems(), &sorted));
        return sorted != 0;
    }
    // arrays handed over by kernels that size their own outputs
    void adopt(const dim<2>& size, array<I> rp, array<I> ci, array<V> v)
    {
        row_ptrs_ = std::move(rp); col_idxs_ = std::move(ci); values_ = std::move(v); set_size(size); max_row_nnz_ = -1;
        invalidate_srow();
    }
protected:
    Csr(std::shared_ptr<const Executor> exec, const dim<2>& size, size_type nnz, std::shared_ptr<strategy_type> strategy)
        : LinOp(exec, size), values_(exec, nnz), col_idxs_(exec, nnz), row_ptrs_(exec, size[0] + 1), strategy_(std::move(strategy)) {}
    // the operand decides (core/matrix/csr.cpp:184-233): a Csr -> spgemm, alpha/Csr/beta -> advanced_spgemm with the old x
    // as D, alpha/Identity/beta -> spgeam with the old x as B, anything else -> spmv
    using sparse_kernels = std::integral_constant<bool, std::is_same<V, double>::value && std::is_same<I, int32>::value>;
    void apply_impl(const LinOp* b, LinOp* x) const override
    {
        if (auto b_csr = dynamic_cast<const Csr*>(b)) {
            spgemm_as(sparse_kernels{}, nullptr, b_csr, nullptr, as<Csr>(x));
        } else {
            spmv(nullptr, b, nullptr, x);
        }
    }
    void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const override
    {
        if (auto b_csr = dynamic_cast<const Csr*>(b)) {
            spgemm_as(sparse_kernels{}, alpha, b_csr, beta, as<Csr>(x));
        } else if (dynamic_cast<const Identity<V>*>(b)) {
            spgeam_as(sparse_kernels{}, alpha, beta, as<Csr>(x));
        } else {
            spmv(alpha, b, beta, x);
        }
    }
    void spgemm_as(std::false_type, const LinOp*, const Csr*, const LinOp*, Csr*) const { GKO_NOT_SUPPORTED("csr::spgemm: <double, int32> only"); }
    void spgeam_as(std::false_type, const LinOp*, const LinOp*, Csr*) const { GKO_NOT_SUPPORTED("csr::spgeam: <double, int32> only"); }
    // csr::spgemm / advanced_spgemm: count, read nnz(C) back, fill.  The reference clones x because its kernel writes
    // into x; here the result goes into fresh arrays that x adopts afterwards, so x's own arrays serve as D and no copy
    // is made (this == x and b == x are fine for the same reason).  adopt() drops srow, the row statistic and the
    // column-partitioned copy of x.
    void spgemm_as(std::true_type, const LinOp* alpha, const Csr* b, const LinOp* beta, Csr* x) const
    {
        detail::require_device(exec_, "csr::spgemm");
        const dim<2> size(size_[0], b->get_size()[1]);
        const double* al = alpha ? detail_fmt::dense(alpha)->get_const_values() : nullptr;
        const double* be = beta ? detail_fmt::dense(beta)->get_const_values() : nullptr;
        array<char> ws(exec_, gkomi_csr_spgemm_workspace_bytes(size[0], size[1]) + 8);
        array<I> rp(exec_, size[0] + 1);
        int64_t nnz = 0;
        auto call = [&](I* ci, V* v) {
            return gkomi_csr_spgemm_f64_i32(nullptr, size_[0], size_[1], get_num_stored_elements(), get_const_row_ptrs(), get_const_col_idxs(), get_const_values(),
                                            b->get_size()[0], b->get_size()[1], b->get_num_stored_elements(), b->get_const_row_ptrs(), b->get_const_col_idxs(),
                                            b->get_const_values(), al, be, x->get_size()[0], x->get_size()[1], alpha ? x->get_num_stored_elements() : 0,
                                            alpha ? x->get_const_row_ptrs() : nullptr, alpha ? x->get_const_col_idxs() : nullptr,
                                            alpha ? x->get_const_values() : nullptr, rp.get_data(), ci, v, &nnz, ws.get_data(), ws.get_num_elems());
        };
        GKOMI_CALL(call(nullptr, nullptr));
        array<I> ci(exec_, static_cast<size_type>(nnz));
        array<V> v(exec_, static_cast<size_type>(nnz));
        if (nnz > 0) GKOMI_CALL(call(ci.get_data(), v.get_data()));
        GKOMI_CALL(gkomi_synchronize(nullptr));  // the workspace goes away with this scope
        x->adopt(size, std::move(rp), std::move(ci), std::move(v));
    }
    // csr::spgeam: alpha * this + beta * x
    void spgeam_as(std::true_type, const LinOp* alpha, const LinOp* beta, Csr* x) const
    {
        detail::require_device(exec_, "csr::spgeam");
        const double* al = detail_fmt::dense(alpha)->get_const_values();
        const double* be = detail_fmt::dense(beta)->get_const_values();
        array<char> ws(exec_, gkomi_csr_spgeam_workspace_bytes(size_[0]) + 8);
        array<I> rp(exec_, size_[0] + 1);
        int64_t nnz = 0;
        auto call = [&](I* ci, V* v) {
            return gkomi_csr_spgeam_f64_i32(nullptr, size_[0], size_[1], al, get_num_stored_elements(), get_const_row_ptrs(), get_const_col_idxs(),
                                            get_const_values(), be, x->get_size()[0], x->get_size()[1], x->get_num_stored_elements(), x->get_const_row_ptrs(),
                                            x->get_const_col_idxs(), x->get_const_values(), rp.get_data(), ci, v, &nnz, ws.get_data(), ws.get_num_elems());
        };
        GKOMI_CALL(call(nullptr, nullptr));
        array<I> ci(exec_, static_cast<size_type>(nnz));
        array<V> v(exec_, static_cast<size_type>(nnz));
        if (nnz > 0) GKOMI_CALL(call(ci.get_data(), v.get_data()));
        GKOMI_CALL(gkomi_synchronize(nullptr));
        x->adopt(size_, std::move(rp), std::move(ci), std::move(v));
    }
    void spmv(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const { spmv_as(V{}, alpha, b, beta, x); }
    // <float, int32>: csr::spmv / advanced_spmv of the single-precision instantiation (gkomi_csr_spmv_f32_i32); no srow
    void spmv_as(float, const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const
    {
        detail::require_device(exec_, "csr::spmv");
        static_assert(!std::is_same<V, float>::value || std::is_same<I, int32>::value, "float: int32 indices");
        auto db = dynamic_cast<const Dense<float>*>(b);
        auto dx = dynamic_cast<Dense<float>*>(x);
        auto da = alpha ? dynamic_cast<const Dense<float>*>(alpha) : nullptr;
        auto dbeta = beta ? dynamic_cast<const Dense<float>*>(beta) : nullptr;
        if (!db || !dx || (alpha && !da) || (beta && !dbeta)) GKO_NOT_SUPPORTED("Csr<float>::apply takes Dense<float> operands");
        GKOMI_CALL(gkomi_csr_spmv_f32_i32(nullptr, size_[0], size_[1], db->get_size()[1], get_num_stored_elements(),
                                          reinterpret_cast<const int32_t*>(get_const_row_ptrs()), reinterpret_cast<const int32_t*>(get_const_col_idxs()),
                                          reinterpret_cast<const float*>(get_const_values()), db->get_const_values(), db->get_stride(), dx->get_values(),
                                          dx->get_stride(), da ? da->get_const_values() : nullptr, dbeta ? dbeta->get_const_values() : nullptr));
    }
    void spmv_as(double, const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const
    {
        detail::require_device(exec_, "csr::spmv");
        auto db = detail_fmt::dense(b); auto dx = detail_fmt::dense(x);
        make_srow();
        if (colpart_ && db->cols() == 1) {
            if (colpart_dirty_) {
                GKOMI_CALL(gkomi_csr_colpart_refresh_f64(nullptr, colpart_.get(), get_const_values()));
                colpart_dirty_ = false;
            }
            GKOMI_CALL(gkomi_csr_colpart_spmv_f64(nullptr, colpart_.get(), db->get_const_values(), db->get_stride(), dx->get_values(), dx->get_stride(),
                                                  alpha ? detail_fmt::dense(alpha)->get_const_values() : nullptr,
                                                  beta ? detail_fmt::dense(beta)->get_const_values() : nullptr));
            return;
        }
        GKOMI_CALL(detail_abi::csr_abi<I>::spmv_srow(nullptr, size_[0], size_[1], db->cols(), get_num_stored_elements(), get_const_row_ptrs(), get_const_col_idxs(),
                                                 get_const_values(), db->get_const_values(), db->get_stride(), dx->get_values(), dx->get_stride(),
                                                 alpha ? detail_fmt::dense(alpha)->get_const_values() : nullptr,
                                                 beta ? detail_fmt::dense(beta)->get_const_values() : nullptr, strategy_->get_code() | gather_flags_, max_row_nnz_,
                                                 get_num_srow_elements() ? get_const_srow() : nullptr, srow_tile_));
    }
public:
    // Csr::srow_ / make_srow (csr.hpp:1139-1157, 1265-1266): the tile start rows of the nonzero-split
    // kernel, rebuilt whenever row_ptrs may have changed (read / adopt / conversions reset it)
    const I* get_const_srow() const noexcept { return srow_.get_const_data(); }
    size_type get_num_srow_elements() const noexcept { return srow_.get_num_elems(); }
    int64_t get_srow_tile() const noexcept { return srow_tile_; }
    void make_srow() const
    {
        if (srow_valid_ || !exec_->is_device()) return;
        const int64_t nnz = static_cast<int64_t>(get_num_stored_elements());
        if (nnz >= 2 && max_row_nnz_ < 0) {  // row statistics of the strategy objects (csr.hpp:526-705)
            array<I> mx(exec_, 1);
            GKOMI_CALL(detail_abi::csr_abi<I>::max_row_nnz(nullptr, size_[0], get_const_row_ptrs(), mx.get_data()));
            max_row_nnz_ = exec_->copy_val_to_host(mx.get_const_data());
        }
        srow_tile_ = gkomi_csr_srow_tile_for(static_cast<int64_t>(get_num_stored_elements()));
        if (nnz >= 2) {
            srow_ = array<I>(exec_, static_cast<size_type>(gkomi_csr_srow_entries(nnz, srow_tile_)));
            GKOMI_CALL(detail_abi::csr_abi<I>::make_srow(nullptr, size_[0], nnz, get_const_row_ptrs(), srow_tile_, srow_.get_data(),
                                                     static_cast<int64_t>(srow_.get_num_elems())));
        } else {
            srow_ = array<I>(exec_, 0);
        }
        // ... and where the gathers of b go: matrices whose long rows select the load-balanced kernel get its column
        // windows when a tile's gathers overflow an XCD's L2 (gkomi_csr_analyse_gather_i32; acts on that kernel only)
        gather_flags_ = 0;
        gather_footprint_ = 0;
        const int code = strategy_->get_code() & 0xff;
        if (nnz >= 2 && (code == GKOMI_CSR_AUTO || code == GKOMI_CSR_BALANCED)) {
            array<double> scratch(exec_, 2);
            gather_flags_ = detail_abi::csr_abi<I>::gather_flags(static_cast<int64_t>(size_[1]), nnz, get_const_col_idxs(), scratch.get_data(), &gather_footprint_);
        }
        // the analysis of the gkomi_partitioned strategy: a scattered column pattern (the statistic above) on a shape that fits
        colpart_.reset();
        const int blocks = strategy_->get_partition_blocks();  // > 0: pinned, neither the statistic nor a timing is asked
        if (strategy_->get_name() == "gkomi_partitioned" && nnz >= 2 && (blocks > 0 || gather_footprint_ > (int64_t{3} << 20))) {  // gathers beyond an L2
            colpart_.reset(detail_abi::csr_abi<I>::colpart_create(exec_, static_cast<int64_t>(size_[0]), static_cast<int64_t>(size_[1]), nnz, get_const_row_ptrs(),
                                                                  get_const_col_idxs(), get_const_values(), colpart_plan_, blocks));
            colpart_dirty_ = false;
        }
        srow_valid_ = true;
    }
    bool has_partitioned_copy() const noexcept { return static_cast<bool>(colpart_); }
    void invalidate_srow() const { srow_valid_ = false; }
protected:
    array<V> values_;
    array<I> col_idxs_;
    array<I> row_ptrs_;
    std::shared_ptr<strategy_type> strategy_;
    mutable int64_t max_row_nnz_{-1};
    mutable array<I> srow_;
    mutable int64_t srow_tile_{0};
    mutable int gather_flags_{0};
    mutable int64_t gather_footprint_{0};
    mutable bool srow_valid_{false};
    struct colpart_deleter {
        void operator()(gkomi_csr_colpart* h) const { gkomi_csr_colpart_destroy(h); }
    };
    mutable std::unique_ptr<gkomi_csr_colpart, colpart_deleter> colpart_;
    mutable array<char> colpart_plan_;
    mutable bool colpart_dirty_{false};
    template <typename, typename>
    friend class Csr;
};

// core/matrix/csr_builder.hpp:47-83: intrusive access to a Csr's arrays for kernels that rebuild them
// (factorization::add_diagonal_elements); the srow is rebuilt when the builder goes away
template <typename V = double, typename I = int32>
class CsrBuilder {
public:
    array<I>& get_col_idx_array() { return matrix_->col_idxs_; }
    array<V>& get_value_array() { return matrix_->values_; }
    explicit CsrBuilder(Csr<V, I>* matrix) : matrix_{matrix} {}
    ~CsrBuilder()
    {
        matrix_->max_row_nnz_ = -1;
        matrix_->invalidate_srow();
    }
    CsrBuilder(const CsrBuilder&) = delete;
    CsrBuilder& operator=(const CsrBuilder&) = delete;
private:
    Csr<V, I>* matrix_;
};

template <typename V = double, typename I = int32>
class CooBuilder;

template <typename V = double, typename I = int32>
class Coo : public LinOp {
public:
    static std::unique_ptr<Coo> create(std::shared_ptr<const Executor> exec, const dim<2>& size = dim<2>{}, size_type nnz = 0) { return std::unique_ptr<Coo>(new Coo(std::move(exec), size, nnz)); }
    V* get_values() noexcept { return values_.get_data(); }
    const V* get_const_values() const noexcept { return values_.get_const_data(); }
    I* get_col_idxs() noexcept { return col_idxs_.get_data(); }
    const I* get_const_col_idxs() const noexcept { return col_idxs_.get_const_data(); }
    // handing out writable row indices forgets what is known about their order
    I* get_row_idxs() noexcept { sorted_state_ = -1; return row_idxs_.get_data(); }
    const I* get_const_row_idxs() const noexcept { return row_idxs_.get_const_data(); }
    size_type get_num_stored_elements() const noexcept { return values_.get_num_elems(); }
    void resize(const dim<2>& size, size_type nnz) { values_.resize_and_reset(nnz); col_idxs_.resize_and_reset(nnz); row_idxs_.resize_and_reset(nnz); set_size(size); sorted_state_ = -1; }
    // row indices non-decreasing (checked on the device once per set of indices):
    // apply / apply2 then run the atomic-free kernels of csrc/coo_spmv.hip
    bool is_sorted_by_row() const { return sorted_workspace(1) != nullptr; }
    // x += A b  (Coo::apply2, include/ginkgo/core/matrix/coo.hpp)
    void apply2(const LinOp* b, LinOp* x) const { validate(b, x); run2(nullptr, b, x); }
    void apply2(const LinOp* alpha, const LinOp* b, LinOp* x) const { validate(b, x); run2(alpha, b, x); }
protected:
    Coo(std::shared_ptr<const Executor> exec, const dim<2>& size, size_type nnz) : LinOp(exec, size), values_(exec, nnz), col_idxs_(exec, nnz), row_idxs_(exec, nnz), sorted_ws_(exec) {}
    // workspace of the sorted kernels, or nullptr when the rows are not sorted (or misaligned)
    void* sorted_workspace(size_type nrhs) const
    {
        if (!exec_->is_device() || sorted_state_ == 0) return nullptr;
        const size_type nnz = get_num_stored_elements();
        const size_type need = std::max<size_type>(gkomi_coo_sorted_workspace_bytes(nnz, nrhs), 16);
        if (sorted_ws_.get_num_elems() < need) sorted_ws_.resize_and_reset(need);
        if (sorted_state_ < 0) {
            int flag = 0;
            int64_t longest = 0;
            GKOMI_CALL(gkomi_coo_analyse_rows_i32(nullptr, nnz, get_const_row_idxs(), sorted_ws_.get_data(), sorted_ws_.get_num_elems(), &flag, &longest));
            max_row_nnz_ = longest;  // capped at 65: rows of up to 64 nonzeros take the one-launch kernel
            const bool aligned = reinterpret_cast<std::uintptr_t>(get_const_values()) % 16 == 0 && reinterpret_cast<std::uintptr_t>(get_const_row_idxs()) % 8 == 0 &&
                                 reinterpret_cast<std::uintptr_t>(get_const_col_idxs()) % 8 == 0;
            sorted_state_ = flag && aligned ? 1 : 0;
        }
        return sorted_state_ == 1 ? sorted_ws_.get_data() : nullptr;
    }
    void run2(const LinOp* alpha, const LinOp* b, LinOp* x) const
    {
        detail::require_device(exec_, "coo::spmv2");
        auto db = detail_fmt::dense(b); auto dx = detail_fmt::dense(x);
        auto al = alpha ? detail_fmt::dense(alpha)->get_const_values() : nullptr;
        if (void* ws = sorted_workspace(db->cols())) {
            GKOMI_CALL(gkomi_coo_spmv2_sorted_f64_i32(nullptr, size_[0], size_[1], db->cols(), get_num_stored_elements(), get_const_row_idxs(), get_const_col_idxs(),
                                                      get_const_values(), db->get_const_values(), db->get_stride(), dx->get_values(), dx->get_stride(), al, max_row_nnz_, ws,
                                                      sorted_ws_.get_num_elems()));
            return;
        }
        GKOMI_CALL(gkomi_coo_spmv2_f64_i32(nullptr, size_[0], size_[1], db->cols(), get_num_stored_elements(), get_const_row_idxs(), get_const_col_idxs(),
                                           get_const_values(), db->get_const_values(), db->get_stride(), dx->get_values(), dx->get_stride(), al));
    }
    void run(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const
    {
        detail::require_device(exec_, "coo::spmv");
        auto db = detail_fmt::dense(b); auto dx = detail_fmt::dense(x);
        auto al = alpha ? detail_fmt::dense(alpha)->get_const_values() : nullptr;
        auto be = beta ? detail_fmt::dense(beta)->get_const_values() : nullptr;
        if (void* ws = sorted_workspace(db->cols())) {
            GKOMI_CALL(gkomi_coo_spmv_sorted_f64_i32(nullptr, size_[0], size_[1], db->cols(), get_num_stored_elements(), get_const_row_idxs(), get_const_col_idxs(),
                                                     get_const_values(), db->get_const_values(), db->get_stride(), dx->get_values(), dx->get_stride(), al, be, max_row_nnz_, ws,
                                                     sorted_ws_.get_num_elems()));
            return;
        }
        GKOMI_CALL(gkomi_coo_spmv_f64_i32(nullptr, size_[0], size_[1], db->cols(), get_num_stored_elements(), get_const_row_idxs(), get_const_col_idxs(),
                                          get_const_values(), db->get_const_values(), db->get_stride(), dx->get_values(), dx->get_stride(), al, be));
    }
    void apply_impl(const LinOp* b, LinOp* x) const override { run(nullptr, b, nullptr, x); }
    void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const override { run(alpha, b, beta, x); }
    array<V> values_;
    array<I> col_idxs_;
    array<I> row_idxs_;
    mutable int sorted_state_{-1};   // -1 unknown, 0 not sorted, 1 sorted
    mutable int64_t max_row_nnz_{-1};
    mutable array<char> sorted_ws_;
    friend class CooBuilder<V, I>;
};

// core/matrix/coo_builder.hpp:47-86: intrusive access to a Coo's arrays for kernels that rebuild them
// (par_ilut_factorization::threshold_filter); what is known about the order of the rows is forgotten
template <typename V, typename I>
class CooBuilder {
public:
    array<I>& get_row_idx_array() { return matrix_->row_idxs_; }
    array<I>& get_col_idx_array() { return matrix_->col_idxs_; }
    array<V>& get_value_array() { return matrix_->values_; }
    explicit CooBuilder(Coo<V, I>* matrix) : matrix_{matrix} {}
    ~CooBuilder() { matrix_->sorted_state_ = -1; }
    CooBuilder(const CooBuilder&) = delete;
    CooBuilder& operator=(const CooBuilder&) = delete;
private:
    Coo<V, I>* matrix_;
};

template <typename V = double, typename I = int32>
class Ell : public LinOp {
public:
    static std::unique_ptr<Ell> create(std::shared_ptr<const Executor> exec, const dim<2>& size = dim<2>{}, size_type num_stored_per_row = 0, size_type stride = 0)
    {
        return std::unique_ptr<Ell>(new Ell(std::move(exec), size, num_stored_per_row, stride ? stride : size[0]));
    }
    V* get_values() noexcept { return values_.get_data(); }
    const V* get_const_values() const noexcept { return values_.get_const_data(); }
    I* get_col_idxs() noexcept { return col_idxs_.get_data(); }
    const I* get_const_col_idxs() const noexcept { return col_idxs_.get_const_data(); }
    size_type get_num_stored_elements_per_row() const noexcept { return k_; }
    size_type get_stride() const noexcept { return stride_; }
    size_type get_num_stored_elements() const noexcept { return values_.get_num_elems(); }
    void resize(const dim<2>& size, size_type k, size_type stride) { k_ = k; stride_ = stride; values_.resize_and_reset(k * stride); col_idxs_.resize_and_reset(k * stride); set_size(size); }
protected:
    Ell(std::shared_ptr<const Executor> exec, const dim<2>& size, size_type k, size_type stride) : LinOp(exec, size), values_(exec, k * stride), col_idxs_(exec, k * stride), k_(k), stride_(stride) {}
    void run(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const
    {
        detail::require_device(exec_, "ell::spmv");
        auto db = detail_fmt::dense(b); auto dx = detail_fmt::dense(x);
        GKOMI_CALL(gkomi_ell_spmv_f64_i32(nullptr, size_[0], size_[1], db->cols(), k_, stride_, get_const_col_idxs(), get_const_values(), db->get_const_values(), db->get_stride(),
                                          dx->get_values(), dx->get_stride(), alpha ? detail_fmt::dense(alpha)->get_const_values() : nullptr, beta ? detail_fmt::dense(beta)->get_const_values() : nullptr));
    }
    void apply_impl(const LinOp* b, LinOp* x) const override { run(nullptr, b, nullptr, x); }
    void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const override { run(alpha, b, beta, x); }
    array<V> values_;
    array<I> col_idxs_;
    size_type k_, stride_;
};

constexpr size_type default_slice_size = 64;
constexpr size_type default_stride_factor = 1;

template <typename V = double, typename I = int32>
class Sellp : public LinOp {
public:
    static std::unique_ptr<Sellp> create(std::shared_ptr<const Executor> exec, const dim<2>& size = dim<2>{}, size_type slice_size = default_slice_size,
                                         size_type stride_factor = default_stride_factor, size_type total_cols = 0)
    {
        return std::unique_ptr<Sellp>(new Sellp(std::move(exec), size, slice_size, stride_factor, total_cols));
    }
    const V* get_const_values() const noexcept { return values_.get_const_data(); }
    const I* get_const_col_idxs() const noexcept { return col_idxs_.get_const_data(); }
    const size_type* get_const_slice_sets() const noexcept { return slice_sets_.get_const_data(); }
    const size_type* get_const_slice_lengths() const noexcept { return slice_lengths_.get_const_data(); }
    size_type get_slice_size() const noexcept { return slice_size_; }
    size_type get_stride_factor() const noexcept { return stride_factor_; }
    size_type get_total_cols() const noexcept { return values_.get_num_elems() / slice_size_; }
    size_type get_num_stored_elements() const noexcept { return values_.get_num_elems(); }
    friend class Csr<V, I>;
protected:
    Sellp(std::shared_ptr<const Executor> exec, const dim<2>& size, size_type slice_size, size_type stride_factor, size_type total_cols)
        : LinOp(exec, size), values_(exec, slice_size * total_cols), col_idxs_(exec, slice_size * total_cols),
          slice_lengths_(exec, (size[0] + slice_size - 1) / slice_size), slice_sets_(exec, (size[0] + slice_size - 1) / slice_size + 1),
          slice_size_(slice_size), stride_factor_(stride_factor) {}
    void run(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const
    {
        detail::require_device(exec_, "sellp::spmv");
        auto db = detail_fmt::dense(b); auto dx = detail_fmt::dense(x);
        GKOMI_CALL(gkomi_sellp_spmv_f64_i32(nullptr, size_[0], size_[1], db->cols(), slice_size_, reinterpret_cast<const uint64_t*>(slice_sets_.get_const_data()),
                                            reinterpret_cast<const uint64_t*>(slice_lengths_.get_const_data()), get_const_col_idxs(), get_const_values(), db->get_const_values(), db->get_stride(),
                                            dx->get_values(), dx->get_stride(), alpha ? detail_fmt::dense(alpha)->get_const_values() : nullptr, beta ? detail_fmt::dense(beta)->get_const_values() : nullptr));
    }
    void apply_impl(const LinOp* b, LinOp* x) const override { run(nullptr, b, nullptr, x); }
    void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const override { run(alpha, b, beta, x); }
    array<V> values_;
    array<I> col_idxs_;
    array<size_type> slice_lengths_;
    array<size_type> slice_sets_;
    size_type slice_size_, stride_factor_;
};

template <typename V = double, typename I = int32>
class Hybrid : public LinOp {
public:
    // ELL-width strategies (include/ginkgo/core/matrix/hybrid.hpp:206-370)
    struct strategy_type { int kind; double percent; double ratio; int64_t num_columns; virtual ~strategy_type() = default;
        strategy_type(int k, double p, double r, int64_t c) : kind(k), percent(p), ratio(r), num_columns(c) {} };
    struct column_limit : strategy_type { explicit column_limit(size_type n = 0) : strategy_type(0, 0, 0, static_cast<int64_t>(n)) {} };
    struct imbalance_limit : strategy_type { explicit imbalance_limit(double p = 0.8) : strategy_type(1, p, 0, 0) {} };
    struct imbalance_bounded_limit : strategy_type { imbalance_bounded_limit(double p = 0.8, double r = 0.0001) : strategy_type(2, p, r, 0) {} };
    struct minimal_storage_limit : strategy_type { minimal_storage_limit() : strategy_type(3, 0, 0, 0) {} };
    struct automatic : strategy_type { automatic() : strategy_type(4, 0, 0, 0) {} };
    static std::unique_ptr<Hybrid> create(std::shared_ptr<const Executor> exec, std::shared_ptr<strategy_type> strategy = std::make_shared<automatic>())
    {
        return std::unique_ptr<Hybrid>(new Hybrid(std::move(exec), std::move(strategy)));
    }
    const Ell<V, I>* get_ell() const noexcept { return ell_.get(); }
    const Coo<V, I>* get_coo() const noexcept { return coo_.get(); }
    size_type get_ell_num_stored_elements_per_row() const noexcept { return ell_->get_num_stored_elements_per_row(); }
    size_type get_coo_num_stored_elements() const noexcept { return coo_->get_num_stored_elements(); }
    std::shared_ptr<strategy_type> get_strategy() const noexcept { return strategy_; }
    friend class Csr<V, I>;
protected:
    Hybrid(std::shared_ptr<const Executor> exec, std::shared_ptr<strategy_type> strategy)
        : LinOp(exec), ell_(Ell<V, I>::create(exec)), coo_(Coo<V, I>::create(exec)), strategy_(std::move(strategy)) {}
    // core/matrix/hybrid.cpp:133-159
    void apply_impl(const LinOp* b, LinOp* x) const override { ell_->apply(b, x); coo_->apply2(b, x); }
    void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const override { ell_->apply(alpha, b, beta, x); coo_->apply2(alpha, b, x); }
    std::unique_ptr<Ell<V, I>> ell_;
    std::unique_ptr<Coo<V, I>> coo_;
    std::shared_ptr<strategy_type> strategy_;
};

// include/ginkgo/core/matrix/fbcsr.hpp: fixed-block CSR, blocks column-major (csrc/fbcsr.hip)
template <typename V = double, typename I = int32>
class Fbcsr : public LinOp {
    static_assert(std::is_same<V, double>::value && std::is_same<I, int32>::value, "Fbcsr: <double, int32> only");
public:
    using mat_data = matrix_data<V, I>;
    // fbcsr.hpp: create(exec, block_size), create(exec, size, num_nonzeros, block_size)
    static std::unique_ptr<Fbcsr> create(std::shared_ptr<const Executor> exec, int block_size = 1)
    {
        return std::unique_ptr<Fbcsr>(new Fbcsr(std::move(exec), dim<2>{}, 0, block_size));
    }
    static std::unique_ptr<Fbcsr> create(std::shared_ptr<const Executor> exec, const dim<2>& size, size_type num_nonzeros, int block_size)
    {
        return std::unique_ptr<Fbcsr>(new Fbcsr(std::move(exec), size, num_nonzeros, block_size));
    }
    int get_block_size() const noexcept { return bs_; }
    void set_block_size(int block_size) { check_block_size(block_size, size_); bs_ = block_size; }
    I get_num_block_rows() const noexcept { return static_cast<I>(size_[0] / bs_); }
    I get_num_block_cols() const noexcept { return static_cast<I>(size_[1] / bs_); }
    size_type get_num_stored_blocks() const noexcept { return col_idxs_.get_num_elems(); }
    size_type get_num_stored_elements() const noexcept { return values_.get_num_elems(); }
    V* get_values() noexcept { return values_.get_data(); }
    const V* get_const_values() const noexcept { return values_.get_const_data(); }
    I* get_col_idxs() noexcept { return col_idxs_.get_data(); }
    const I* get_const_col_idxs() const noexcept { return col_idxs_.get_const_data(); }
    I* get_row_ptrs() noexcept { return row_ptrs_.get_data(); }
    const I* get_const_row_ptrs() const noexcept { return row_ptrs_.get_const_data(); }
    // Fbcsr::read(matrix_data) (core/matrix/fbcsr.cpp; fbcsr::fill_in_matrix_data is the loop of csr::convert_to_fbcsr):
    // row-major sorted, duplicate-free entries, dimensions divisible by the block size
    void read(const mat_data& data)
    {
        auto csr = Csr<V, I>::create(exec_);
        csr->read(data);
        csr->convert_to(this);
    }
    void convert_to(Csr<V, I>* result) const
    {
        detail::require_device(exec_, "fbcsr::convert_to_csr");
        const size_type nnz = get_num_stored_elements();
        array<I> rp(exec_, size_[0] + 1), ci(exec_, nnz);
        array<V> v(exec_, nnz);
        GKOMI_CALL(gkomi_fbcsr_convert_to_csr_i32(nullptr, get_num_block_rows(), bs_, get_num_stored_blocks(), get_const_row_ptrs(), get_const_col_idxs(), get_const_values(),
                                                  rp.get_data(), ci.get_data(), v.get_data()));
        result->adopt(size_, std::move(rp), std::move(ci), std::move(v));
    }
    void convert_to(Dense<V>* result) const
    {
        detail::require_device(exec_, "fbcsr::fill_in_dense");
        auto tmp = Dense<V>::create(exec_, size_);
        tmp->fill(V{});
        GKOMI_CALL(gkomi_fbcsr_fill_in_dense_f64_i32(nullptr, get_num_block_rows(), get_num_block_cols(), bs_, get_num_stored_blocks(), get_const_row_ptrs(), get_const_col_idxs(),
                                                     get_const_values(), tmp->get_values(), tmp->get_stride()));
        result->copy_from(tmp.get());
    }
    std::unique_ptr<Fbcsr> transpose() const
    {
        detail::require_device(exec_, "fbcsr::transpose");
        auto t = Fbcsr::create(exec_, gko::transpose(size_), get_num_stored_elements(), bs_);
        array<char> ws(exec_, gkomi_fbcsr_transpose_workspace_bytes(get_num_stored_blocks()) + 8);
        GKOMI_CALL(gkomi_fbcsr_transpose_f64_i32(nullptr, get_num_block_rows(), get_num_block_cols(), bs_, get_num_stored_blocks(), get_const_row_ptrs(), get_const_col_idxs(),
                                                 get_const_values(), t->get_row_ptrs(), t->get_col_idxs(), t->get_values(), ws.get_data(), ws.get_num_elems()));
        return t;
    }
    std::unique_ptr<Fbcsr> conj_transpose() const { return transpose(); }
    void sort_by_column_index()
    {
        detail::require_device(exec_, "fbcsr::sort_by_column_index");
        array<char> ws(exec_, gkomi_fbcsr_sort_workspace_bytes(get_num_stored_blocks(), bs_) + 8);
        GKOMI_CALL(gkomi_fbcsr_sort_by_column_index_f64_i32(nullptr, get_num_block_rows(), bs_, get_num_stored_blocks(), get_const_row_ptrs(), get_col_idxs(), get_values(),
                                                            ws.get_data(), ws.get_num_elems()));
    }
    bool is_sorted_by_column_index() const
    {
        detail::require_device(exec_, "fbcsr::is_sorted_by_column_index");
        array<char> ws(exec_, 8);
        int sorted = 1;
        GKOMI_CALL(gkomi_fbcsr_is_sorted_by_column_index_i32(nullptr, get_num_block_rows(), get_const_row_ptrs(), get_const_col_idxs(), ws.get_data(), ws.get_num_elems(), &sorted));
        return sorted != 0;
    }
    // the diagonal as an array of min(rows, cols) values, zero where no diagonal block is stored (the mirror has no
    // matrix::Diagonal; Csr's diagonal is read the same way, by the ABI call, where Jacobi needs it)
    array<V> extract_diagonal() const
    {
        detail::require_device(exec_, "fbcsr::extract_diagonal");
        array<V> diag(exec_, std::min(size_[0], size_[1]));
        diag.fill(V{});
        GKOMI_CALL(gkomi_fbcsr_extract_diagonal_f64_i32(nullptr, get_num_block_rows(), get_num_block_cols(), bs_, get_const_row_ptrs(), get_const_col_idxs(), get_const_values(),
                                                        diag.get_data()));
        return diag;
    }
    // arrays handed over by kernels that size their own outputs
    void adopt(const dim<2>& size, int block_size, array<I> rp, array<I> ci, array<V> v)
    {
        check_block_size(block_size, size);
        bs_ = block_size; row_ptrs_ = std::move(rp); col_idxs_ = std::move(ci); values_ = std::move(v); set_size(size);
    }
protected:
    static void check_block_size(int block_size, const dim<2>& size)
    {
        if (block_size < 1 || size[0] % block_size != 0 || size[1] % block_size != 0)
            throw BadDimension(__FILE__, __LINE__, "Fbcsr: the block size does not divide the size");
    }
    Fbcsr(std::shared_ptr<const Executor> exec, const dim<2>& size, size_type num_nonzeros, int block_size)
        : LinOp(exec, size), values_(exec, num_nonzeros), col_idxs_(exec, block_size > 0 ? num_nonzeros / (static_cast<size_type>(block_size) * block_size) : 0),
          row_ptrs_(exec, block_size > 0 ? size[0] / block_size + 1 : 1), bs_(block_size)
    {
        check_block_size(block_size, size);
        row_ptrs_.fill(I{});
    }
    void run(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const
    {
        detail::require_device(exec_, "fbcsr::spmv");
        auto db = detail_fmt::dense(b); auto dx = detail_fmt::dense(x);
        GKOMI_CALL(gkomi_fbcsr_spmv_f64_i32(nullptr, get_num_block_rows(), get_num_block_cols(), bs_, get_num_stored_blocks(), get_const_row_ptrs(), get_const_col_idxs(),
                                            get_const_values(), db->get_const_values(), db->get_stride(), db->cols(), dx->get_values(), dx->get_stride(),
                                            alpha ? detail_fmt::dense(alpha)->get_const_values() : nullptr, beta ? detail_fmt::dense(beta)->get_const_values() : nullptr));
    }
    void apply_impl(const LinOp* b, LinOp* x) const override { run(nullptr, b, nullptr, x); }
    void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const override { run(alpha, b, beta, x); }
    array<V> values_;
    array<I> col_idxs_;
    array<I> row_ptrs_;
    int bs_;
};

// conversions (core/matrix/csr.cpp:257-405)
template <typename V, typename I>
void Csr<V, I>::convert_to(Coo<V, I>* result) const
{
    detail::require_device(exec_, "csr::convert_to_coo");
    result->resize(size_, get_num_stored_elements());
    exec_->copy(get_num_stored_elements(), get_const_values(), result->get_values());
    exec_->copy(get_num_stored_elements(), get_const_col_idxs(), result->get_col_idxs());
    GKOMI_CALL(gkomi_convert_ptrs_to_idxs_i32(nullptr, get_const_row_ptrs(), size_[0], result->get_row_idxs()));
}
template <typename V, typename I>
void Csr<V, I>::convert_to(Ell<V, I>* result) const
{
    detail::require_device(exec_, "csr::convert_to_ell");
    array<I> mx(exec_, 1);
    GKOMI_CALL(gkomi_csr_max_row_nnz_i32(nullptr, size_[0], get_const_row_ptrs(), mx.get_data()));
    const size_type k = static_cast<size_type>(exec_->copy_val_to_host(mx.get_const_data()));
    result->resize(size_, k, size_[0]);
    GKOMI_CALL(gkomi_csr_convert_to_ell_f64_i32(nullptr, size_[0], get_const_row_ptrs(), get_const_col_idxs(), get_const_values(), k, size_[0], result->get_col_idxs(), result->get_values()));
}
template <typename V, typename I>
void Csr<V, I>::convert_to(Sellp<V, I>* result) const
{
    detail::require_device(exec_, "csr::convert_to_sellp");
    const size_type ss = result->slice_size_, sf = result->stride_factor_;
    const size_type nslices = (size_[0] + ss - 1) / ss;
    result->slice_sets_.resize_and_reset(nslices + 1);
    result->slice_lengths_.resize_and_reset(nslices);
    array<char> ws(exec_, gkomi_prefix_sum_workspace_bytes(nslices + 1) + 8);
    GKOMI_CALL(gkomi_sellp_compute_slice_sets_i32(nullptr, get_const_row_ptrs(), size_[0], ss, sf, reinterpret_cast<uint64_t*>(result->slice_sets_.get_data()),
                                                  reinterpret_cast<uint64_t*>(result->slice_lengths_.get_data()), ws.get_data(), ws.get_num_elems()));
    const size_type total = exec_->copy_val_to_host(result->slice_sets_.get_const_data() + nslices);
    result->values_.resize_and_reset(total * ss);
    result->col_idxs_.resize_and_reset(total * ss);
    result->set_size(size_);
    GKOMI_CALL(gkomi_csr_convert_to_sellp_f64_i32(nullptr, size_[0], get_const_row_ptrs(), get_const_col_idxs(), get_const_values(), ss,
                                                  reinterpret_cast<const uint64_t*>(result->slice_sets_.get_const_data()), reinterpret_cast<const uint64_t*>(result->slice_lengths_.get_const_data()),
                                                  result->col_idxs_.get_data(), result->values_.get_data()));
}
template <typename V, typename I>
void Csr<V, I>::convert_to(Hybrid<V, I>* result) const
{
    detail::require_device(exec_, "csr::convert_to_hybrid");
    const auto& st = *result->strategy_;
    int64_t ell_lim = 0;
    GKOMI_CALL(gkomi_hybrid_ell_width_i32(nullptr, get_const_row_ptrs(), size_[0], st.kind, st.percent, st.ratio, st.num_columns, &ell_lim));
    if (ell_lim > static_cast<int64_t>(size_[1])) ell_lim = size_[1];
    array<int64> crp(exec_, size_[0] + 1);
    array<char> ws(exec_, gkomi_prefix_sum_workspace_bytes(size_[0] + 1) + 8);
    GKOMI_CALL(gkomi_hybrid_compute_coo_row_ptrs_i32(nullptr, get_const_row_ptrs(), size_[0], ell_lim, crp.get_data(), ws.get_data(), ws.get_num_elems()));
    const size_type coo_nnz = static_cast<size_type>(exec_->copy_val_to_host(crp.get_const_data() + size_[0]));
    result->ell_->resize(size_, ell_lim, size_[0]);
    result->coo_->resize(size_, coo_nnz);
    result->set_size(size_);
    GKOMI_CALL(gkomi_csr_convert_to_hybrid_f64_i32(nullptr, size_[0], get_const_row_ptrs(), get_const_col_idxs(), get_const_values(), crp.get_const_data(), ell_lim, size_[0],
                                                   result->ell_->get_col_idxs(), result->ell_->get_values(), result->coo_->get_row_idxs(), result->coo_->get_col_idxs(), result->coo_->get_values()));
}

template <typename V, typename I>
void Csr<V, I>::convert_to(Fbcsr<V, I>* result) const
{
    detail::require_device(exec_, "csr::convert_to_fbcsr");
    const int bs = result->get_block_size();
    const size_type nnz = get_num_stored_elements();
    auto rexec = result->get_executor();
    array<char> ws(exec_, gkomi_csr_convert_to_fbcsr_workspace_bytes(nnz) + 8);
    array<I> rp(rexec, bs > 0 ? size_[0] / bs + 1 : 1);
    int64_t nbnz = 0;
    GKOMI_CALL(gkomi_csr_convert_to_fbcsr_i32(nullptr, size_[0], size_[1], bs, nnz, get_const_row_ptrs(), get_const_col_idxs(), get_const_values(), rp.get_data(), nullptr, nullptr,
                                              &nbnz, ws.get_data(), ws.get_num_elems()));
    array<I> ci(rexec, static_cast<size_type>(nbnz));
    array<V> v(rexec, static_cast<size_type>(nbnz) * bs * bs);
    if (nbnz > 0) {
        GKOMI_CALL(gkomi_csr_convert_to_fbcsr_i32(nullptr, size_[0], size_[1], bs, nnz, get_const_row_ptrs(), get_const_col_idxs(), get_const_values(), rp.get_data(), ci.get_data(),
                                                  v.get_data(), &nbnz, ws.get_data(), ws.get_num_elems()));
    }
    result->adopt(size_, bs, std::move(rp), std::move(ci), std::move(v));
}

}  // namespace matrix

// ---- binary matrix I/O (core/base/mtx_io.cpp:768-960): 32-byte header = magic
// "GINKGO" + value type (D/S) + index type (I/L), rows, cols, entries as uint64,
// then (row, column, value) records; complex files are refused ----------------------
namespace detail {
inline uint64 binary_magic(char value_bit, char index_bit)
{
    const char m[8] = {'G', 'I', 'N', 'K', 'G', 'O', value_bit, index_bit};
    uint64 v;
    std::memcpy(&v, m, 8);
    return v;
}
template <typename FV, typename FI, typename V, typename I>
matrix_data<V, I> read_binary_entries(std::istream& is, uint64 rows, uint64 cols, uint64 entries)
{
    if (rows > static_cast<uint64>(std::numeric_limits<I>::max()) || cols > static_cast<uint64>(std::numeric_limits<I>::max()))
        throw StreamError(__FILE__, __LINE__, "cannot read into this format, its index type would overflow");
    matrix_data<V, I> result;
    result.size = dim<2>(rows, cols);
    result.nonzeros.resize(entries);
    for (uint64 i = 0; i < entries; ++i) {
        char block[sizeof(FV) + 2 * sizeof(FI)];
        if (!is.read(block, sizeof(block))) throw StreamError(__FILE__, __LINE__, "failed reading entry " + std::to_string(i));
        FI row, column; FV value;
        std::memcpy(&row, block, sizeof(FI));
        std::memcpy(&column, block + sizeof(FI), sizeof(FI));
        std::memcpy(&value, block + 2 * sizeof(FI), sizeof(FV));
        result.nonzeros[i] = {static_cast<I>(row), static_cast<I>(column), static_cast<V>(value)};
    }
    result.ensure_row_major_order();
    return result;
}
}  // namespace detail

template <typename V = double, typename I = int32>
matrix_data<V, I> read_binary_raw(std::istream& is)
{
    char header[32];
    if (!is.read(header, 32)) throw StreamError(__FILE__, __LINE__, "failed reading header");
    uint64 magic, rows, cols, entries;
    std::memcpy(&magic, header, 8); std::memcpy(&rows, header + 8, 8); std::memcpy(&cols, header + 16, 8); std::memcpy(&entries, header + 24, 8);
    if (magic == detail::binary_magic('D', 'I')) return detail::read_binary_entries<double, int32, V, I>(is, rows, cols, entries);
    if (magic == detail::binary_magic('S', 'I')) return detail::read_binary_entries<float, int32, V, I>(is, rows, cols, entries);
    if (magic == detail::binary_magic('D', 'L')) return detail::read_binary_entries<double, int64, V, I>(is, rows, cols, entries);
    if (magic == detail::binary_magic('S', 'L')) return detail::read_binary_entries<float, int64, V, I>(is, rows, cols, entries);
    if (magic == detail::binary_magic('Z', 'I') || magic == detail::binary_magic('C', 'I') || magic == detail::binary_magic('Z', 'L') || magic == detail::binary_magic('C', 'L'))
        throw StreamError(__FILE__, __LINE__, "cannot read into this format, would assign complex to real");
    throw StreamError(__FILE__, __LINE__, "invalid header magic number '" + std::string(header, 8) + "'");
}
template <typename V = double, typename I = int32>
matrix_data<V, I> read_generic_raw(std::istream& is)
{
    const auto first = is.peek();
    if (!is) throw StreamError(__FILE__, __LINE__, "failed reading from stream");
    return first == '%' ? read_raw<V, I>(is) : read_binary_raw<V, I>(is);
}
template <typename V, typename I>
void write_binary_raw(std::ostream& os, const matrix_data<V, I>& data)
{
    static_assert(std::is_same<V, double>::value && std::is_same<I, int32>::value, "this mirror stores double / int32");
    const uint64 hdr[4] = {detail::binary_magic('D', 'I'), data.size[0], data.size[1], data.nonzeros.size()};
    os.write(reinterpret_cast<const char*>(hdr), 32);
    for (const auto& e : data.nonzeros) {
        char block[16];
        std::memcpy(block, &e.row, 4); std::memcpy(block + 4, &e.column, 4); std::memcpy(block + 8, &e.value, 8);
        os.write(block, 16);
    }
    if (!os) throw StreamError(__FILE__, __LINE__, "failed writing the matrix");
}

// ---- read / write / initialize ------------------------------------------------------
template <typename M, typename Stream>
std::unique_ptr<M> read_binary(Stream&& is, std::shared_ptr<const Executor> exec)
{
    auto data = read_binary_raw<double, int32>(is);
    auto m = M::create(std::move(exec));
    m->read(data);
    return m;
}
template <typename M, typename Stream>
std::unique_ptr<M> read_generic(Stream&& is, std::shared_ptr<const Executor> exec)
{
    auto data = read_generic_raw<double, int32>(is);
    auto m = M::create(std::move(exec));
    m->read(data);
    return m;
}
template <typename M>
void write_binary(std::ostream& os, const M* m)
{
    matrix_data<double, int32> data;
    m->write(data);
    write_binary_raw(os, data);
}
template <typename M, typename Stream>
std::unique_ptr<M> read(Stream&& is, std::shared_ptr<const Executor> exec)
{
    auto data = read_raw<double, int32>(is);
    auto m = M::create(std::move(exec));
    m->read(data);
    return m;
}
template <typename M>
void write(std::ostream& os, const M* m)
{
    matrix_data<double, int32> data;
    m->write(data);
    // Dense is written in array layout, sparse formats in coordinate layout
    if (std::is_same<M, matrix::Dense<double>>::value) {
        os << "%%MatrixMarket matrix array real general\n" << data.size[0] << " " << data.size[1] << "\n";
        std::vector<double> colmajor(data.size[0] * data.size[1]);
        for (const auto& e : data.nonzeros) colmajor[e.column * data.size[0] + e.row] = e.value;
        for (double v : colmajor) os << v << "\n";
    } else {
        os << "%%MatrixMarket matrix coordinate real general\n" << data.size[0] << " " << data.size[1] << " " << data.nonzeros.size() << "\n";
        for (const auto& e : data.nonzeros) os << e.row + 1 << " " << e.column + 1 << " " << e.value << "\n";
    }
}
template <typename M>
std::unique_ptr<M> initialize(size_type stride, std::initializer_list<typename M::value_type> vals, std::shared_ptr<const Executor> exec)
{
    auto host = exec->get_master();
    auto tmp = matrix::Dense<double>::create(host, dim<2>(vals.size(), 1), stride);
    size_type i = 0;
    for (auto v : vals) tmp->at(i++, 0) = v;
    auto m = M::create(exec, dim<2>(vals.size(), 1), stride);
    m->copy_from(tmp.get());
    return m;
}
template <typename M>
std::unique_ptr<M> initialize(std::initializer_list<typename M::value_type> vals, std::shared_ptr<const Executor> exec) { return initialize<M>(1, vals, std::move(exec)); }
template <typename M>
std::unique_ptr<M> initialize(std::initializer_list<std::initializer_list<typename M::value_type>> vals, std::shared_ptr<const Executor> exec)
{
    const size_type r = vals.size(), c = r ? vals.begin()->size() : 0;
    auto tmp = matrix::Dense<double>::create(exec->get_master(), dim<2>(r, c));
    size_type i = 0;
    for (const auto& row : vals) { size_type j = 0; for (auto v : row) tmp->at(i, j++) = v; ++i; }
    auto m = M::create(exec, dim<2>(r, c));
    m->copy_from(tmp.get());
    return m;
}

// ---- stopping criteria (include/ginkgo/core/stop/*.hpp) ---------------------------------
namespace stop {
enum class mode { absolute, initial_resnorm, rhs_norm };
struct criterion_settings {
    int64_t max_iters{std::numeric_limits<int64_t>::max() / 4};
    double reduction_factor{-1.0};  // < 0: no residual criterion
    mode baseline{mode::rhs_norm};
    bool implicit{false};           // ImplicitResidualNorm: sqrt of the solver's implicit r.z instead of ||r||
};
class CriterionFactory {
public:
    virtual ~CriterionFactory() = default;
    virtual void contribute(criterion_settings& s) const = 0;
};
template <typename Concrete>
struct builder_base {
    std::shared_ptr<const CriterionFactory> on(std::shared_ptr<const Executor>) const { return std::make_shared<Concrete>(static_cast<const Concrete&>(*this)); }
};
class Iteration : public CriterionFactory, public builder_base<Iteration> {
public:
    static Iteration build() { return {}; }
    Iteration& with_max_iters(size_type n) { max_iters_ = n; return *this; }
    void contribute(criterion_settings& s) const override { s.max_iters = std::min<int64_t>(s.max_iters, static_cast<int64_t>(max_iters_)); }
private:
    size_type max_iters_{0};
};
template <typename V = double>
class ResidualNorm : public CriterionFactory, public builder_base<ResidualNorm<V>> {
public:
    static ResidualNorm build() { return {}; }
    ResidualNorm& with_reduction_factor(V f) { factor_ = f; return *this; }
    ResidualNorm& with_baseline(mode m) { baseline_ = m; return *this; }
    void contribute(criterion_settings& s) const override { s.reduction_factor = factor_; s.baseline = baseline_; }
private:
    V factor_{static_cast<V>(1e-15)};  // residual_norm.hpp:65
    mode baseline_{mode::rhs_norm};
};
// stop::ImplicitResidualNorm (include/ginkgo/core/stop/residual_norm.hpp:193-244; kernel
// stop::implicit_residual_norm): the criterion on sqrt(|r.z|), the quantity Cg / Fcg carry anyway.
// With the Identity preconditioner that IS ||r||, and the native drivers evaluate it as such; with
// another preconditioner the solvers refuse it (their drivers evaluate ResidualNorm).
template <typename V = double>
class ImplicitResidualNorm : public CriterionFactory, public builder_base<ImplicitResidualNorm<V>> {
public:
    static ImplicitResidualNorm build() { return {}; }
    ImplicitResidualNorm& with_reduction_factor(V f) { factor_ = f; return *this; }
    ImplicitResidualNorm& with_baseline(mode m) { baseline_ = m; return *this; }
    void contribute(criterion_settings& s) const override { s.reduction_factor = factor_; s.baseline = baseline_; s.implicit = true; }
private:
    V factor_{static_cast<V>(1e-15)};
    mode baseline_{mode::rhs_norm};
};
// stop::Combined (include/ginkgo/core/stop/combined.hpp): stops when ANY of its criteria does,
// which is how the drivers treat a list of criteria anyway (Iteration is asked first)
class Combined : public CriterionFactory, public builder_base<Combined> {
public:
    static Combined build() { return {}; }
    template <typename... Criteria>
    Combined& with_criteria(Criteria&&... c)
    {
        criteria_ = {std::shared_ptr<const CriterionFactory>(std::forward<Criteria>(c))...};
        return *this;
    }
    Combined& with_criteria(std::vector<std::shared_ptr<const CriterionFactory>> c) { criteria_ = std::move(c); return *this; }
    void contribute(criterion_settings& s) const override { for (const auto& c : criteria_) if (c) c->contribute(s); }
private:
    std::vector<std::shared_ptr<const CriterionFactory>> criteria_;
};
// stop::combine (combined.hpp:130-160)
template <typename FactoryContainer>
std::shared_ptr<const CriterionFactory> combine(FactoryContainer&& factories)
{
    if (factories.size() == 1) return factories[0];
    auto exec = std::shared_ptr<const Executor>();
    return Combined::build().with_criteria(std::vector<std::shared_ptr<const CriterionFactory>>(factories.begin(), factories.end())).on(exec);
}
}  // namespace stop

namespace detail {
// A system whose solve is a collective: implemented by experimental::distributed::Matrix
// (distributed.hpp); the solvers hand such a system to its own driver.
struct distributed_system {
    virtual ~distributed_system() = default;
    virtual void cg_solve(const LinOp* b, LinOp* x, const stop::criterion_settings& settings, const LinOp* precond, int64_t* iters,
                          bool* converged) const = 0;
};
}  // namespace detail

// ---- preconditioners -----------------------------------------------------------------
namespace detail {
// a preconditioner the library has a callback of its own for (gkomi_jacobi_apply_cb, gkomi_ilu_apply_cb): it hands
// the native drivers that callback and its record instead of an opaque LinOp::apply
struct native_preconditioner {
    virtual ~native_preconditioner() = default;
    // false: not in this configuration (the caller wraps LinOp::apply)
    virtual bool native_callback(gkomi_apply_fn& fn, void*& ctx, size_type nrhs) const = 0;
};
// a LinOp as a gkomi_apply_fn for the native solver drivers
struct linop_callback {
    const LinOp* op;
    std::shared_ptr<const Executor> exec;
    size_type n, nrhs;
    static int call(void* ctx, gkomi_stream_t, const double* in, double* out)
    {
        auto* c = static_cast<linop_callback*>(ctx);
        try {
            auto vin = matrix::Dense<double>::create(c->exec, dim<2>(c->n, c->nrhs), array<double>::view(c->exec, c->n * c->nrhs, const_cast<double*>(in)), c->nrhs);
            auto vout = matrix::Dense<double>::create(c->exec, dim<2>(c->n, c->nrhs), array<double>::view(c->exec, c->n * c->nrhs, out), c->nrhs);
            c->op->apply(vin.get(), vout.get());
        } catch (const std::exception&) {
            return GKOMI_EINVAL;
        }
        return 0;
    }
};
// any LinOp as a gkomi_matrix_apply_fn: the system matrix of the *_solve_op_f64
// drivers (Ell, Sellp, Coo, Hybrid, ... -- config 4 of BASELINE.json)
struct matrix_callback {
    const LinOp* op;
    std::shared_ptr<const Executor> exec;
    size_type n;
    static int call(void* ctx, gkomi_stream_t, int64_t nrhs, const double* alpha, const double* b, int64_t b_stride, const double* beta, double* c, int64_t c_stride)
    {
        auto* m = static_cast<matrix_callback*>(ctx);
        try {
            const size_type k = static_cast<size_type>(nrhs);
            auto vb = matrix::Dense<double>::create(m->exec, dim<2>(m->n, k), array<double>::view(m->exec, m->n * b_stride, const_cast<double*>(b)), b_stride);
            auto vc = matrix::Dense<double>::create(m->exec, dim<2>(m->n, k), array<double>::view(m->exec, m->n * c_stride, c), c_stride);
            if (alpha == nullptr) {
                m->op->apply(vb.get(), vc.get());
            } else {
                auto va = matrix::Dense<double>::create(m->exec, dim<2>(1, 1), array<double>::view(m->exec, 1, const_cast<double*>(alpha)), 1);
                auto vbeta = matrix::Dense<double>::create(m->exec, dim<2>(1, 1), array<double>::view(m->exec, 1, const_cast<double*>(beta)), 1);
                m->op->apply(va.get(), vb.get(), vbeta.get(), vc.get());
            }
        } catch (const std::exception&) {
            return GKOMI_EINVAL;
        }
        return 0;
    }
};
// A Csr as the record of gkomi_csr_matrix_apply_cb (and of gkomi_isai_apply_cb): the matrix travels with its srow and
// its row statistic, so the drivers run the kernel Csr::apply runs, also inside their fused SpMV + dot launches
inline void fill_csr_ctx(const matrix::Csr<double, int32>* c, gkomi_csr_ctx& csr)
{
    c->make_srow();
    csr.nrows = static_cast<int64_t>(c->get_size()[0]);
    csr.ncols = static_cast<int64_t>(c->get_size()[1]);
    csr.nnz = static_cast<int64_t>(c->get_num_stored_elements());
    csr.row_ptrs = c->get_const_row_ptrs();
    csr.col_idxs = c->get_const_col_idxs();
    csr.vals = c->get_const_values();
    csr.strategy = c->get_strategy()->get_code();
    csr.max_row_nnz_hint = c->get_max_row_nnz();
    csr.srow = c->get_num_srow_elements() ? c->get_const_srow() : nullptr;
    csr.srow_tile = c->get_num_srow_elements() ? c->get_srow_tile() : 0;
}
// The system matrix of a solver as (gkomi_matrix_apply_fn, context): Ell and
// Sellp go by the library's own callbacks + records, which the fused drivers
// recognise (SpMV with the dot-product epilogue, csrc/formats.hip), Fbcsr and Dense
// by their own callbacks + records (no epilogue: the drivers follow them with their
// partials kernel); every other LinOp goes through matrix_callback.
struct system_callback {
    matrix_callback generic;
    gkomi_csr_ctx csr{};
    gkomi_ell_ctx ell{};
    gkomi_sellp_ctx sellp{};
    gkomi_fbcsr_ctx fbcsr{};
    gkomi_dense_ctx dense{};
    gkomi_matrix_apply_fn fn;
    void* ctx;
    system_callback(const LinOp* A, std::shared_ptr<const Executor> exec, size_type n)
        : generic{A, std::move(exec), n}, fn(&matrix_callback::call), ctx(&generic)
    {
        if (auto c = dynamic_cast<const matrix::Csr<double, int32>*>(A)) {
            fill_csr_ctx(c, csr);
            fn = &gkomi_csr_matrix_apply_cb;
            ctx = &csr;
        } else if (auto e = dynamic_cast<const matrix::Ell<double, int32>*>(A)) {
            ell.nrows = static_cast<int64_t>(e->get_size()[0]);
            ell.ncols = static_cast<int64_t>(e->get_size()[1]);
            ell.num_stored_per_row = static_cast<int64_t>(e->get_num_stored_elements_per_row());
            ell.stride = static_cast<int64_t>(e->get_stride());
            ell.col_idxs = e->get_const_col_idxs();
            ell.vals = e->get_const_values();
            fn = &gkomi_ell_matrix_apply_cb;
            ctx = &ell;
        } else if (auto sp = dynamic_cast<const matrix::Sellp<double, int32>*>(A)) {
            sellp.nrows = static_cast<int64_t>(sp->get_size()[0]);
            sellp.ncols = static_cast<int64_t>(sp->get_size()[1]);
            sellp.slice_size = static_cast<int64_t>(sp->get_slice_size());
            sellp.slice_sets = reinterpret_cast<const uint64_t*>(sp->get_const_slice_sets());
            sellp.slice_lengths = reinterpret_cast<const uint64_t*>(sp->get_const_slice_lengths());
            sellp.col_idxs = sp->get_const_col_idxs();
            sellp.vals = sp->get_const_values();
            fn = &gkomi_sellp_matrix_apply_cb;
            ctx = &sellp;
        } else if (auto fb = dynamic_cast<const matrix::Fbcsr<double, int32>*>(A)) {
            fbcsr.nbrows = fb->get_num_block_rows();
            fbcsr.nbcols = fb->get_num_block_cols();
            fbcsr.bs = fb->get_block_size();
            fbcsr.nbnz = static_cast<int64_t>(fb->get_num_stored_blocks());
            fbcsr.row_ptrs = fb->get_const_row_ptrs();
            fbcsr.col_idxs = fb->get_const_col_idxs();
            fbcsr.vals = fb->get_const_values();
            fn = &gkomi_fbcsr_matrix_apply_cb;
            ctx = &fbcsr;
        } else if (auto d = dynamic_cast<const matrix::Dense<double>*>(A)) {
            // ordered (mode 1): the reference's bits for any number of right-hand sides, and no workspace
            dense.nrows = d->rows();
            dense.ncols = d->cols();
            dense.stride = static_cast<int64_t>(d->get_stride());
            dense.vals = d->get_const_values();
            dense.mode = 1;
            fn = &gkomi_dense_matrix_apply_cb;
            ctx = &dense;
        }
    }
    system_callback(const system_callback&) = delete;
    system_callback& operator=(const system_callback&) = delete;
};
}  // namespace detail

// include/ginkgo/core/base/types.hpp:257-400
class precision_reduction {
public:
    using storage_type = uint8;
    constexpr precision_reduction() noexcept : data_{0} {}
    constexpr precision_reduction(storage_type preserving, storage_type nonpreserving) noexcept
        : data_(static_cast<storage_type>((preserving << 4) | nonpreserving)) {}
    constexpr operator storage_type() const noexcept { return data_; }
    constexpr storage_type get_preserving() const noexcept { return data_ >> 4; }
    constexpr storage_type get_nonpreserving() const noexcept { return data_ & 0xf; }
    constexpr static precision_reduction autodetect() noexcept { return from_bits(0xff); }
    constexpr static precision_reduction from_bits(storage_type b) noexcept { precision_reduction p; p.data_ = b; return p; }
private:
    storage_type data_;
};

namespace preconditioner {
// include/ginkgo/core/preconditioner/jacobi.hpp:62-167
template <typename IndexType>
struct block_interleaved_storage_scheme {
    block_interleaved_storage_scheme() = default;
    block_interleaved_storage_scheme(IndexType block_offset_, IndexType group_offset_, uint32 group_power_)
        : block_offset{block_offset_}, group_offset{group_offset_}, group_power{group_power_} {}
    IndexType block_offset{};
    IndexType group_offset{};
    uint32 group_power{};
    IndexType get_group_size() const noexcept { return IndexType{1} << group_power; }
    size_type compute_storage_space(size_type num_blocks) const noexcept
    {
        return (num_blocks + 1 == size_type{0}) ? size_type{0} : ((num_blocks + get_group_size() - 1) / get_group_size()) * group_offset;
    }
    IndexType get_group_offset(IndexType block_id) const noexcept { return group_offset * (block_id >> group_power); }
    IndexType get_block_offset(IndexType block_id) const noexcept { return block_offset * (block_id & (get_group_size() - 1)); }
    IndexType get_global_block_offset(IndexType block_id) const noexcept { return get_group_offset(block_id) + get_block_offset(block_id); }
    IndexType get_stride() const noexcept { return block_offset << group_power; }
};

template <typename V = double, typename I = int32>
class Jacobi : public LinOp, public Transposable, public ::gko::detail::native_preconditioner {
public:
    class Factory : public LinOpFactory {
    public:
        Factory& with_max_block_size(uint32 n) { max_block_size_ = n; return *this; }
        // storage_optimization (jacobi.hpp:262-330): one precision for all blocks
        // (autodetect() = adaptive) or a list repeated over the blocks
        Factory& with_storage_optimization(precision_reduction p) { storage_.assign(1, p); adaptive_ = true; return *this; }
        Factory& with_storage_optimization(const std::vector<precision_reduction>& p) { storage_ = p; adaptive_ = !p.empty(); return *this; }
        Factory& with_accuracy(double a) { accuracy_ = a; return *this; }
        // jacobi.hpp:338-349: 0 = the executor's default = the wavefront size (64 on HIP), the only
        // stride the kernels of this backend lay the blocks out for
        Factory& with_max_block_stride(uint32 s)
        {
            if (s != 0 && s != 64) GKO_NOT_SUPPORTED("max_block_stride: 0 or 64 (the HIP wavefront size)");
            return *this;
        }
        std::shared_ptr<Factory> on(std::shared_ptr<const Executor> exec) const { auto f = std::make_shared<Factory>(*this); f->exec_ = std::move(exec); return f; }
        std::unique_ptr<Jacobi> generate(std::shared_ptr<const LinOp> A) const
        {
            return std::unique_ptr<Jacobi>(new Jacobi(this->exec_, max_block_size_, adaptive_ ? &storage_ : nullptr, accuracy_, std::move(A)));
        }
        std::unique_ptr<LinOp> generate_impl(std::shared_ptr<const LinOp> A) const override { return generate(std::move(A)); }
        Factory() : LinOpFactory(nullptr) {}
    private:
        uint32 max_block_size_{32};  // jacobi.hpp:338-349
        std::vector<precision_reduction> storage_;
        bool adaptive_{false};
        double accuracy_{1e-1};      // jacobi.hpp:332-336
    };
    static Factory build() { return Factory{}; }
    size_type get_num_blocks() const noexcept { return num_blocks_; }
    uint32 get_max_block_size() const noexcept { return max_block_size_; }
    // per-block storage precisions actually used / condition numbers (adaptive storage only)
    std::vector<precision_reduction> get_block_precisions() const
    {
        std::vector<precision_reduction> out;
        for (auto b : precisions_.to_host()) out.push_back(precision_reduction::from_bits(b));
        return out;
    }
    std::vector<double> get_conditioning() const { return conditioning_.to_host(); }
    // jacobi.hpp:557-609: the scheme of max_block_stride = 64
    block_interleaved_storage_scheme<I> get_storage_scheme() const
    {
        int64_t o[4] = {};
        GKOMI_CALL(gkomi_jacobi_storage_scheme(static_cast<int>(max_block_size_), o));
        return {static_cast<I>(o[0]), static_cast<I>(o[1]), static_cast<uint32>(o[2])};
    }
    const V* get_blocks() const noexcept { return blocks_.get_const_data(); }
    size_type get_num_stored_elements() const noexcept { return blocks_.get_num_elems(); }
    const I* get_const_block_pointers() const noexcept { return block_ptrs_.get_const_data(); }
    // Jacobi::transpose (core/preconditioner/jacobi.cpp): same blocks structure,
    // every stored block transposed in its storage precision (jacobi::transpose_jacobi)
    std::unique_ptr<LinOp> transpose() const override
    {
        std::unique_ptr<Jacobi> t(new Jacobi(*this));
        if (max_block_size_ > 1 && num_blocks_ > 0) {
            t->blocks_ = array<V>(exec_, blocks_.get_num_elems());
            GKOMI_CALL(gkomi_jacobi_transpose_f64_i32(nullptr, num_blocks_, max_block_size_, block_ptrs_.get_const_data(),
                                                      precisions_.get_num_elems() > 0 ? precisions_.get_const_data() : nullptr, blocks_.get_const_data(),
                                                      t->blocks_.get_data()));
        }  // scalar Jacobi: a diagonal is its own transpose
        return std::unique_ptr<LinOp>(t.release());
    }
protected:
    Jacobi(const Jacobi&) = default;
    Jacobi(std::shared_ptr<const Executor> exec, uint32 max_bs, const std::vector<precision_reduction>* storage, double accuracy, std::shared_ptr<const LinOp> A)
        : LinOp(exec, A->get_size()), max_block_size_(max_bs), block_ptrs_(exec), blocks_(exec), precisions_(exec), conditioning_(exec)
    {
        ::gko::detail::require_device(exec_, "jacobi::generate");
        if (max_bs < 1 || max_bs > 32) GKO_NOT_SUPPORTED("max_block_size must be in [1, 32]");
        auto csr = as<const matrix::Csr<V, I>>(A.get());
        const size_type n = size_[0];
        if (max_bs == 1) {
            array<V> diag(exec_, n);
            blocks_.resize_and_reset(n);
            GKOMI_CALL(gkomi_csr_extract_diagonal_f64_i32(nullptr, n, csr->get_const_row_ptrs(), csr->get_const_col_idxs(), csr->get_const_values(), diag.get_data()));
            GKOMI_CALL(gkomi_jacobi_invert_diagonal_f64(nullptr, n, diag.get_const_data(), blocks_.get_data()));
            num_blocks_ = n;
            return;
        }
        block_ptrs_.resize_and_reset(n + 1);
        array<int64> nb(exec_, 1);
        array<char> ws(exec_, gkomi_jacobi_find_blocks_workspace_bytes(n));
        int64_t host_nb = 0;
        GKOMI_CALL(gkomi_jacobi_find_blocks_i32(nullptr, n, csr->get_const_row_ptrs(), csr->get_const_col_idxs(), max_bs, block_ptrs_.get_data(), nb.get_data(), ws.get_data(), ws.get_num_elems(), &host_nb));
        num_blocks_ = static_cast<size_type>(host_nb);
        blocks_.resize_and_reset(gkomi_jacobi_storage_elements(max_bs, host_nb));
        if (storage == nullptr) {
            GKOMI_CALL(gkomi_jacobi_generate_f64_i32(nullptr, n, csr->get_const_row_ptrs(), csr->get_const_col_idxs(), csr->get_const_values(), host_nb, max_bs, block_ptrs_.get_const_data(), nullptr, blocks_.get_data()));
            return;
        }
        // jacobi::initialize_precisions (jacobi_kernels.cpp:485-493): the list repeats over the blocks
        std::vector<uint8> req(num_blocks_);
        for (size_type i = 0; i < num_blocks_; ++i) req[i] = (*storage)[i % storage->size()];
        precisions_ = array<uint8>(exec_, req.begin(), req.end());
        conditioning_.resize_and_reset(num_blocks_);
        GKOMI_CALL(gkomi_jacobi_generate_adaptive_f64_i32(nullptr, n, csr->get_const_row_ptrs(), csr->get_const_col_idxs(), csr->get_const_values(), host_nb, max_bs,
                                                          block_ptrs_.get_const_data(), accuracy, conditioning_.get_data(), precisions_.get_data(), blocks_.get_data()));
    }
    void run(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const
    {
        auto db = matrix::detail_fmt::dense(b); auto dx = matrix::detail_fmt::dense(x);
        const double* a = alpha ? matrix::detail_fmt::dense(alpha)->get_const_values() : nullptr;
        const double* be = beta ? matrix::detail_fmt::dense(beta)->get_const_values() : nullptr;
        if (max_block_size_ == 1) {
            GKOMI_CALL(gkomi_jacobi_scalar_apply_f64(nullptr, size_[0], db->cols(), blocks_.get_const_data(), a, db->get_const_values(), db->get_stride(), be, dx->get_values(), dx->get_stride()));
        } else if (precisions_.get_num_elems() > 0) {
            GKOMI_CALL(gkomi_jacobi_apply_adaptive_f64_i32(nullptr, num_blocks_, max_block_size_, block_ptrs_.get_const_data(), precisions_.get_const_data(), blocks_.get_const_data(),
                                                           db->cols(), a, db->get_const_values(), db->get_stride(), be, dx->get_values(), dx->get_stride()));
        } else {
            GKOMI_CALL(gkomi_jacobi_apply_f64_i32(nullptr, num_blocks_, max_block_size_, block_ptrs_.get_const_data(), blocks_.get_const_data(), db->cols(), a, db->get_const_values(), db->get_stride(), be, dx->get_values(), dx->get_stride()));
        }
    }
    void apply_impl(const LinOp* b, LinOp* x) const override { run(nullptr, b, nullptr, x); }
    void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const override { run(alpha, b, beta, x); }
public:
    // this preconditioner as the record of the library's own callback (gkomi_jacobi_apply_cb): the native drivers
    // then see a block-Jacobi, not an opaque operator (the fused CG lets its apply carry r.z and r.r).  The record
    // lives in the object: one solve at a time per preconditioner object and column count.
    bool native_callback(gkomi_apply_fn& fn, void*& ctx, size_type nrhs) const override
    {
        if (!std::is_same<V, double>::value || !std::is_same<I, int32>::value) return false;
        gkomi_jacobi_ctx& c = record_;
        c.n = static_cast<int64_t>(size_[0]);
        c.nrhs = static_cast<int64_t>(nrhs);
        c.num_blocks = static_cast<int64_t>(num_blocks_);
        c.max_block_size = static_cast<int32_t>(max_block_size_);
        c.pad_ = 0;
        c.block_ptrs = max_block_size_ == 1 ? nullptr : block_ptrs_.get_const_data();
        c.blocks = blocks_.get_const_data();
        c.block_precisions = precisions_.get_num_elems() > 0 ? precisions_.get_const_data() : nullptr;
        fn = &gkomi_jacobi_apply_cb;
        ctx = &record_;
        return true;
    }
private:
    mutable gkomi_jacobi_ctx record_{};
    uint32 max_block_size_;
    size_type num_blocks_{0};
    array<I> block_ptrs_;
    array<V> blocks_;
    array<uint8> precisions_;
    array<double> conditioning_;
};
}  // namespace preconditioner

namespace detail {
// The preconditioner of a native solver driver as (gkomi_apply_fn, context): a preconditioner::Jacobi or Ilu
// <double, int32> goes by the library's own callback + record (native_preconditioner), any other LinOp by linop_callback.
struct precond_callback {
    linop_callback generic;
    gkomi_apply_fn fn = nullptr;
    void* ctx = nullptr;
    precond_callback(const LinOp* op, std::shared_ptr<const Executor> exec, size_type n, size_type nrhs) : generic{op, std::move(exec), n, nrhs}
    {
        if (op == nullptr) return;
        if (auto native = dynamic_cast<const native_preconditioner*>(op)) {
            if (native->native_callback(fn, ctx, nrhs)) return;
        }
        fn = &linop_callback::call;
        ctx = &generic;
    }
    precond_callback(const precond_callback&) = delete;
    precond_callback& operator=(const precond_callback&) = delete;
};
}  // namespace detail

// ---- solvers ------------------------------------------------------------------------------
namespace solver {
// include/ginkgo/core/solver/solver_base.hpp:57-72, 93-124
enum class initial_guess_mode { zero, rhs, provided };
class ApplyWithInitialGuess {
public:
    virtual ~ApplyWithInitialGuess() = default;
    virtual void apply_with_initial_guess(const LinOp* b, LinOp* x, initial_guess_mode guess) const = 0;
    initial_guess_mode get_default_initial_guess() const noexcept { return guess_; }
protected:
    void set_default_initial_guess(initial_guess_mode guess) { guess_ = guess; }
    // prepare_initial_guess (solver_base.hpp:130-150)
    static void prepare_initial_guess(const LinOp* b, LinOp* x, initial_guess_mode guess)
    {
        if (guess == initial_guess_mode::zero) {
            matrix::detail_fmt::dense(x)->fill(0.0);
        } else if (guess == initial_guess_mode::rhs) {
            matrix::detail_fmt::dense(x)->copy_from(matrix::detail_fmt::dense(b));
        }
    }
private:
    initial_guess_mode guess_{initial_guess_mode::provided};
};
namespace detail {
// GKOMI_MG_FUSED=0 / 1 forces the three-call sequence / the fused Jacobi sweep of a multigrid smoother at every size
// (A/B runs); otherwise fused up to the last size at which it was measured through this mirror to be at least as fast:
// the row "409600 | 2045440" of the mirror's table in profiles/multigrid_probe_reading.md; on the next row, 2946048
// nonzeros, it loses, so the crossover lies between the two.  Either way the same bits.
inline bool multigrid_fused(size_type nnz)
{
    const char* e = std::getenv("GKOMI_MG_FUSED");
    if (e != nullptr && (e[0] == '0' || e[0] == '1') && e[1] == 0) return e[0] == '1';
    return nnz <= 2045440;
}
template <typename Solver>
class factory_base : public LinOpFactory {
public:
    factory_base() : LinOpFactory(nullptr) {}
    template <typename... Criteria>
    typename Solver::Factory& with_criteria(Criteria&&... c)
    {
        criteria_ = {std::shared_ptr<const stop::CriterionFactory>(std::forward<Criteria>(c))...};
        return static_cast<typename Solver::Factory&>(*this);
    }
    typename Solver::Factory& with_preconditioner(std::shared_ptr<const LinOpFactory> f) { precond_factory_ = std::move(f); return static_cast<typename Solver::Factory&>(*this); }
    typename Solver::Factory& with_generated_preconditioner(std::shared_ptr<const LinOp> p) { precond_ = std::move(p); return static_cast<typename Solver::Factory&>(*this); }
    std::shared_ptr<typename Solver::Factory> on(std::shared_ptr<const Executor> exec) const
    {
        auto f = std::make_shared<typename Solver::Factory>(static_cast<const typename Solver::Factory&>(*this));
        f->exec_ = std::move(exec);
        return f;
    }
    std::unique_ptr<Solver> generate(std::shared_ptr<const LinOp> A) const { return std::unique_ptr<Solver>(new Solver(static_cast<const typename Solver::Factory*>(this), std::move(A))); }
    template <typename M>
    std::unique_ptr<Solver> generate(std::unique_ptr<M>&& A) const { return generate(std::shared_ptr<const LinOp>(std::move(A))); }
    std::unique_ptr<LinOp> generate_impl(std::shared_ptr<const LinOp> A) const override { return generate(std::move(A)); }
    stop::criterion_settings settings() const
    {
        stop::criterion_settings s;
        for (const auto& c : criteria_) c->contribute(s);
        if (s.reduction_factor < 0) s.reduction_factor = 0.0;  // Iteration only
        if (s.implicit && (precond_ || precond_factory_)) {
            GKO_NOT_SUPPORTED("ImplicitResidualNorm with a preconditioner: the native drivers evaluate ResidualNorm (identical without one)");
        }
        return s;
    }
    std::vector<std::shared_ptr<const stop::CriterionFactory>> criteria_;
    std::shared_ptr<const LinOpFactory> precond_factory_;
    std::shared_ptr<const LinOp> precond_;
};

inline int baseline_code(stop::mode m) { return m == stop::mode::rhs_norm ? 0 : (m == stop::mode::initial_resnorm ? 1 : 2); }

// What Cg, Bicgstab / Fcg / Cgs, Idr, Bicg, Ir and Gmres share: the system matrix, the generated or given preconditioner,
// the stop settings, the outcome of the last apply, the advanced apply and the frame of a plain apply.  A derived class
// adds the parameters of its Factory, its workspace size and its one driver call.
template <typename Derived>
class iterative_solver : public LinOp {
public:
    // a solver with factory parameters of its own declares its own Factory and build()
    class Factory : public factory_base<Derived> {};
    static Factory build() { return Factory{}; }
    std::shared_ptr<const LinOp> get_system_matrix() const { return A_; }
    std::shared_ptr<const LinOp> get_preconditioner() const { return precond_; }
    // filled by the last apply
    int64_t get_last_iteration_count() const noexcept { return last_iters_; }
    bool has_converged() const noexcept { return last_converged_; }
    // what the criteria of the factory amount to (the role of get_stop_criterion_factory())
    const stop::criterion_settings& get_stop_settings() const noexcept { return settings_; }
protected:
    template <typename F>
    iterative_solver(const F* f, std::shared_ptr<const LinOp> A) : LinOp(f->get_executor(), gko::transpose(A->get_size())), A_(std::move(A)), settings_(f->settings())
    {
        if (size_[0] != size_[1]) throw DimensionMismatch(__FILE__, __LINE__, "the solver needs a square system matrix");
        precond_ = f->precond_ ? f->precond_ : (f->precond_factory_ ? std::shared_ptr<const LinOp>(f->precond_factory_->generate_impl(A_)) : nullptr);
    }
    using LinOp::apply_impl;
    // x = alpha * solve(b) + beta * x  (core/solver/cg.cpp:196-210)
    void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const override
    {
        auto dx = matrix::detail_fmt::dense(x);
        auto x_clone = dx->clone();
        this->apply_impl(b, x_clone.get());
        dx->scale(matrix::detail_fmt::dense(beta));
        dx->add_scaled(matrix::detail_fmt::dense(alpha), x_clone.get());
    }
    // the first two entries of a driver's info record
    void report(const double* info) const
    {
        last_iters_ = static_cast<int64_t>(info[0]);
        last_converged_ = info[1] != 0.0;
    }
    // The operands of a plain apply on the device: b and x as contiguous Dense<double>, their sizes, the info record.
    struct operands {
        const iterative_solver& solver;
        const matrix::Dense<double>* db;
        matrix::Dense<double>* dx;
        int64_t n, nrhs;
        std::vector<double> info;
        operands(const iterative_solver& s, const LinOp* b, LinOp* x) : solver(s)
        {
            ::gko::detail::require_device(s.exec_, "solver::apply");
            db = matrix::detail_fmt::dense(b);
            dx = matrix::detail_fmt::dense(x);
            n = s.size_[0];
            nrhs = db->cols();
            if (db->get_stride() != static_cast<size_type>(nrhs) || dx->get_stride() != static_cast<size_type>(nrhs)) GKO_NOT_SUPPORTED("solver vectors must be contiguous (stride == #columns)");
            info.assign(2 + 2 * nrhs, 0.0);
        }
        void report() const { solver.report(info.data()); }
    };
    // ... and the two callbacks of the *_solve_op_f64 drivers: the preconditioner (detail::precond_callback) and the
    // system matrix, a Csr as its record with srow and row statistic (detail::system_callback)
    struct frame : operands {
        ::gko::detail::precond_callback precond;
        ::gko::detail::system_callback system;
        frame(const iterative_solver& s, const LinOp* b, LinOp* x)
            : operands(s, b, x), precond(s.precond_.get(), s.exec_, static_cast<size_type>(this->n), static_cast<size_type>(this->nrhs)),
              system(s.A_.get(), s.exec_, static_cast<size_type>(this->n))
        {}
    };
    std::shared_ptr<const LinOp> A_;
    std::shared_ptr<const LinOp> precond_;
    stop::criterion_settings settings_;
    mutable int64_t last_iters_{-1};
    mutable bool last_converged_{false};
};
}  // namespace detail

template <typename V = double>
class Cg : public detail::iterative_solver<Cg<V>> {
    using base = detail::iterative_solver<Cg<V>>;
protected:
    friend class detail::factory_base<Cg>;
    Cg(const typename base::Factory* f, std::shared_ptr<const LinOp> A) : base(f, std::move(A)) {}
    using base::apply_impl;
    void apply_impl(const LinOp* b, LinOp* x) const override { solve_as(V{}, b, x); }
    // Cg<float>: the single-precision instantiation -- the reference's kernel sequence on the _f32 kernels (gkomi_cg_solve_f32):
    // a Csr<float, int32> system matrix, Dense<float> vectors with one column, no preconditioner, Iteration + ResidualNorm
    void solve_as(float, const LinOp* b, LinOp* x) const
    {
        const auto& exec = this->exec_;
        const auto& st = this->settings_;
        ::gko::detail::require_device(exec, "cg::apply");
        auto A = dynamic_cast<const matrix::Csr<float, int32>*>(this->A_.get());
        auto db = dynamic_cast<const matrix::Dense<float>*>(b);
        auto dx = dynamic_cast<matrix::Dense<float>*>(x);
        auto db64 = A ? dynamic_cast<const matrix::Dense<double>*>(b) : nullptr;
        auto dx64 = A ? dynamic_cast<matrix::Dense<double>*>(x) : nullptr;
        if (db64 && dx64) {
            // Dense<double> operands: through temporary float copies (precision_dispatch, precision_dispatch.hpp:73-96)
            auto bf = matrix::Dense<float>::create(exec, db64->get_size());
            auto xf = matrix::Dense<float>::create(exec, dx64->get_size());
            db64->convert_to(bf.get());
            dx64->convert_to(xf.get());
            solve_as(float{}, bf.get(), xf.get());
            xf->convert_to(dx64);
            return;
        }
        if (!A || !db || !dx || this->precond_ || st.implicit || db->get_size()[1] != 1 || db->get_stride() != 1 || dx->get_stride() != 1) {
            GKO_NOT_SUPPORTED("Cg<float>: Csr<float, int32> system, Dense<float> vectors of one contiguous column, Iteration + ResidualNorm, no preconditioner");
        }
        const int64_t n = this->size_[0];
        array<char> ws(exec, gkomi_cg_workspace_bytes_f32(n));
        double info[4] = {};
        GKOMI_CALL(gkomi_cg_solve_f32(nullptr, n, static_cast<int64_t>(A->get_num_stored_elements()), A->get_const_row_ptrs(), A->get_const_col_idxs(),
                                      A->get_const_values(), db->get_const_values(), dx->get_values(), st.max_iters,
                                      static_cast<float>(st.reduction_factor), detail::baseline_code(st.baseline), ws.get_data(),
                                      ws.get_num_elems(), info));
        this->report(info);
    }
    void solve_as(double, const LinOp* b, LinOp* x) const
    {
        const auto& st = this->settings_;
        if (auto ds = dynamic_cast<const ::gko::detail::distributed_system*>(this->A_.get())) {
            // experimental::distributed::Matrix + Vectors: the row-partitioned driver
            ds->cg_solve(b, x, st, this->precond_.get(), &this->last_iters_, &this->last_converged_);
            return;
        }
        typename base::frame f(*this, b, x);
        array<char> ws(this->exec_, gkomi_cg_workspace_bytes(f.n, f.nrhs));
        if (f.nrhs == 1) {  // the fused loop; Ell / Sellp with the dot in the SpMV's epilogue
            GKOMI_CALL(gkomi_cg_solve_fused_op_f64(nullptr, f.n, f.system.fn, f.system.ctx, f.precond.fn, f.precond.ctx, f.db->get_const_values(), f.dx->get_values(),
                                                   st.max_iters, st.reduction_factor, detail::baseline_code(st.baseline), 8, ws.get_data(), ws.get_num_elems(), f.info.data()));
        } else {
            GKOMI_CALL(gkomi_cg_solve_op_f64(nullptr, f.n, f.nrhs, f.system.fn, f.system.ctx, f.precond.fn, f.precond.ctx, f.db->get_const_values(), f.dx->get_values(),
                                             st.max_iters, st.reduction_factor, detail::baseline_code(st.baseline), ws.get_data(), ws.get_num_elems(), f.info.data()));
        }
        f.report();
    }
};

// Bicgstab / Fcg / Cgs (include/ginkgo/core/solver/{bicgstab,fcg,cgs}.hpp): same factory parameters as Cg, native
// drivers of csrc/krylov.hip -- the fused one for one right-hand side, the reference kernel sequence otherwise
namespace detail {
using krylov_fused_op_driver = int (*)(gkomi_stream_t, int64_t, gkomi_matrix_apply_fn, void*, gkomi_apply_fn, void*, const double*, double*, int64_t, double, int, int64_t,
                                       void*, size_t, double*);
using krylov_op_driver = int (*)(gkomi_stream_t, int64_t, int64_t, gkomi_matrix_apply_fn, void*, gkomi_apply_fn, void*, const double*, double*, int64_t, double, int, int64_t,
                                 void*, size_t, double*);
template <typename Derived, krylov_fused_op_driver FusedOpDriver, krylov_op_driver OpDriver>
class krylov_solver : public iterative_solver<Derived> {
protected:
    using base = iterative_solver<Derived>;
    template <typename F>
    krylov_solver(const F* f, std::shared_ptr<const LinOp> A) : base(f, std::move(A)) {}
    using base::apply_impl;
    void apply_impl(const LinOp* b, LinOp* x) const override
    {
        const auto& st = this->settings_;
        typename base::frame f(*this, b, x);
        array<char> ws(this->exec_, gkomi_krylov_workspace_bytes(f.n, f.nrhs));
        if (f.nrhs == 1) {
            GKOMI_CALL(FusedOpDriver(nullptr, f.n, f.system.fn, f.system.ctx, f.precond.fn, f.precond.ctx, f.db->get_const_values(), f.dx->get_values(), st.max_iters,
                                     st.reduction_factor, baseline_code(st.baseline), 8, ws.get_data(), ws.get_num_elems(), f.info.data()));
        } else {
            GKOMI_CALL(OpDriver(nullptr, f.n, f.nrhs, f.system.fn, f.system.ctx, f.precond.fn, f.precond.ctx, f.db->get_const_values(), f.dx->get_values(), st.max_iters,
                                st.reduction_factor, baseline_code(st.baseline), 8, ws.get_data(), ws.get_num_elems(), f.info.data()));
        }
        f.report();
    }
};
}  // namespace detail

#define GKOMI_KRYLOV_SOLVER(Name, fused_op_driver, op_driver)                                      \
    template <typename V = double>                                                                 \
    class Name : public detail::krylov_solver<Name<V>, fused_op_driver, op_driver> {               \
        using base = detail::krylov_solver<Name<V>, fused_op_driver, op_driver>;                   \
        friend class detail::factory_base<Name>;                                                   \
        Name(const typename base::Factory* f, std::shared_ptr<const LinOp> A) : base(f, std::move(A)) {} \
    }
GKOMI_KRYLOV_SOLVER(Bicgstab, gkomi_bicgstab_solve_fused_op_f64, gkomi_bicgstab_solve_op_f64);
GKOMI_KRYLOV_SOLVER(Fcg, gkomi_fcg_solve_fused_op_f64, gkomi_fcg_solve_op_f64);
GKOMI_KRYLOV_SOLVER(Cgs, gkomi_cgs_solve_fused_op_f64, gkomi_cgs_solve_op_f64);
#undef GKOMI_KRYLOV_SOLVER

// Idr (include/ginkgo/core/solver/idr.hpp): IDR(s) with a real subspace, native drivers of csrc/idr.hip (the fused
// one for a single right-hand side and s <= 8).  P is filled on the host: std::normal_distribution<>(0, 1) over
// std::default_random_engine(15) when deterministic, as core/solver/idr.cpp:159-164 does, seeded from
// std::random_device otherwise; the device orthonormalises its rows.  get_last_iteration_count() counts outer
// iterations (s + 1 applies of the system matrix each).
template <typename V = double>
class Idr : public detail::iterative_solver<Idr<V>> {
    using base = detail::iterative_solver<Idr<V>>;
public:
    class Factory : public detail::factory_base<Idr> {
    public:
        Factory& with_subspace_dim(size_type s) { subspace_dim_ = s; return *this; }
        Factory& with_kappa(V k) { kappa_ = k; return *this; }
        Factory& with_deterministic(bool d) { deterministic_ = d; return *this; }
        Factory& with_complex_subspace(bool c)
        {
            if (c) GKO_NOT_SUPPORTED("Idr: complex subspace (this backend is fp64 only)");
            return *this;
        }
        size_type subspace_dim_{2};  // idr.hpp: defaults 2, 0.7, false
        V kappa_{0.7};
        bool deterministic_{false};
    };
    static Factory build() { return Factory{}; }
    size_type get_subspace_dim() const noexcept { return subspace_dim_; }
    V get_kappa() const noexcept { return kappa_; }
    bool get_deterministic() const noexcept { return deterministic_; }
    bool get_complex_subspace() const noexcept { return false; }
protected:
    friend class detail::factory_base<Idr>;
    Idr(const Factory* f, std::shared_ptr<const LinOp> A) : base(f, std::move(A)), subspace_dim_(f->subspace_dim_), kappa_(f->kappa_), deterministic_(f->deterministic_)
    {
        static_assert(std::is_same<V, double>::value, "Idr: fp64 only");
    }
    using base::apply_impl;
    void apply_impl(const LinOp* b, LinOp* x) const override
    {
        const auto& exec = this->exec_;
        const auto& st = this->settings_;
        typename base::frame f(*this, b, x);
        const int64_t s = static_cast<int64_t>(subspace_dim_);
        std::vector<double> host_p(static_cast<size_t>(s * f.n));
        std::default_random_engine engine(deterministic_ ? 15u : std::random_device{}());
        std::normal_distribution<> dist(0.0, 1.0);
        for (auto& v : host_p) v = dist(engine);
        array<double> p(exec, host_p.size());
        exec->copy_from(exec->get_master().get(), host_p.size(), host_p.data(), p.get_data());
        array<char> ws(exec, gkomi_idr_workspace_bytes(f.n, f.nrhs, s));
        auto driver = f.nrhs == 1 && s <= 8 ? &gkomi_idr_solve_fused_op_f64 : &gkomi_idr_solve_op_f64;
        GKOMI_CALL(driver(nullptr, f.n, f.nrhs, f.system.fn, f.system.ctx, f.precond.fn, f.precond.ctx, s, kappa_, p.get_data(), f.db->get_const_values(), f.dx->get_values(),
                          st.max_iters, st.reduction_factor, detail::baseline_code(st.baseline), 8, ws.get_data(), ws.get_num_elems(), f.info.data()));
        f.report();
    }
    size_type subspace_dim_;
    V kappa_;
    bool deterministic_;
};

// Bicg (include/ginkgo/core/solver/bicg.hpp): the transposed system matrix is
// built once at generate (the reference rebuilds it in every apply), and so is
// the transposed preconditioner (bicg.cpp:169-171 asks the preconditioner for its
// Transposable interface: Jacobi here).
template <typename V = double>
class Bicg : public detail::iterative_solver<Bicg<V>> {
    using base = detail::iterative_solver<Bicg<V>>;
protected:
    friend class detail::factory_base<Bicg>;
    Bicg(const typename base::Factory* f, std::shared_ptr<const LinOp> A) : base(f, std::move(A))
    {
        if (this->precond_) {
            auto tr = dynamic_cast<const Transposable*>(this->precond_.get());
            if (tr == nullptr) GKO_NOT_SUPPORTED("Bicg: the preconditioner must be Transposable");
            precond_t_ = std::shared_ptr<const LinOp>(tr->conj_transpose());
        }
        if (auto csr = dynamic_cast<const matrix::Csr<V, int32>*>(this->A_.get())) {
            At_ = csr->transpose();
        } else {
            // any other Transposable system matrix (a Dense): both go to the driver as operators
            auto tr = dynamic_cast<const Transposable*>(this->A_.get());
            if (tr == nullptr) GKO_NOT_SUPPORTED("Bicg: the system matrix must be Transposable");
            At_op_ = std::shared_ptr<const LinOp>(tr->conj_transpose());
        }
    }
    using base::apply_impl;
    void apply_impl(const LinOp* b, LinOp* x) const override
    {
        const auto& st = this->settings_;
        const bool pre = this->precond_ != nullptr;
        typename base::operands f(*this, b, x);
        array<char> ws(this->exec_, gkomi_krylov_workspace_bytes(f.n, f.nrhs));
        ::gko::detail::linop_callback cb{this->precond_.get(), this->exec_, static_cast<size_type>(f.n), static_cast<size_type>(f.nrhs)};
        ::gko::detail::linop_callback cbt{precond_t_.get(), this->exec_, static_cast<size_type>(f.n), static_cast<size_type>(f.nrhs)};
        auto pfn = pre ? &::gko::detail::linop_callback::call : nullptr;
        if (At_op_) {
            ::gko::detail::system_callback sys{this->A_.get(), this->exec_, static_cast<size_type>(f.n)};
            ::gko::detail::system_callback sys_t{At_op_.get(), this->exec_, static_cast<size_type>(f.n)};
            GKOMI_CALL(gkomi_bicg_solve_op_f64(nullptr, f.n, f.nrhs, sys.fn, sys.ctx, sys_t.fn, sys_t.ctx, pfn, pre ? &cb : nullptr, pfn, pre ? &cbt : nullptr,
                                               f.db->get_const_values(), f.dx->get_values(), st.max_iters, st.reduction_factor,
                                               detail::baseline_code(st.baseline), 8, ws.get_data(), ws.get_num_elems(), f.info.data()));
            f.report();
            return;
        }
        auto csr = as<const matrix::Csr<V, int32>>(this->A_.get());
        GKOMI_CALL(gkomi_bicg_solve_f64_i32(nullptr, f.n, f.nrhs, csr->get_num_stored_elements(), csr->get_const_row_ptrs(), csr->get_const_col_idxs(), csr->get_const_values(),
                                            At_->get_const_row_ptrs(), At_->get_const_col_idxs(), At_->get_const_values(), csr->get_strategy()->get_code(), csr->get_max_row_nnz(),
                                            pfn, pre ? &cb : nullptr, pfn, pre ? &cbt : nullptr, f.db->get_const_values(), f.dx->get_values(), st.max_iters, st.reduction_factor,
                                            detail::baseline_code(st.baseline), 8, ws.get_data(), ws.get_num_elems(), f.info.data()));
        f.report();
    }
    std::shared_ptr<const LinOp> precond_t_;
    std::unique_ptr<matrix::Csr<V, int32>> At_;
    std::shared_ptr<const LinOp> At_op_;
};

// Ir (include/ginkgo/core/solver/ir.hpp): x += relaxation_factor * solver(b - A x);
// without an inner solver it is the Richardson iteration.  The inner solver sits in the
// preconditioner slot of the common base and factory: with_solver / with_generated_solver
// are with_preconditioner / with_generated_preconditioner, get_solver() is get_preconditioner().
template <typename V = double>
class Ir : public detail::iterative_solver<Ir<V>>, public ApplyWithInitialGuess {
    using base = detail::iterative_solver<Ir<V>>;
public:
    class Factory : public detail::factory_base<Ir> {
    public:
        Factory& with_relaxation_factor(V r) { relaxation_factor_ = r; return *this; }
        Factory& with_default_initial_guess(initial_guess_mode g) { guess_ = g; return *this; }
        initial_guess_mode guess_{initial_guess_mode::provided};
        Factory& with_solver(std::shared_ptr<const LinOpFactory> f) { this->precond_factory_ = std::move(f); return *this; }
        Factory& with_generated_solver(std::shared_ptr<const LinOp> p) { this->precond_ = std::move(p); return *this; }
        V relaxation_factor_{1.0};
    };
    static Factory build() { return Factory{}; }
    std::shared_ptr<const LinOp> get_solver() const { return this->precond_; }
    // inner iterations of the last apply, summed over its inner solves: known when it ran as the native
    // mixed-precision driver (-1 otherwise)
    int64_t get_last_inner_iteration_count() const noexcept { return last_inner_iters_; }
    // ir.hpp:105-109
    bool apply_uses_initial_guess() const override { return this->get_default_initial_guess() == initial_guess_mode::provided; }
    V get_relaxation_factor() const noexcept { return relaxation_factor_; }
    // Ir::apply_with_initial_guess (core/solver/ir.cpp:170-183).  Ir<double> over a generated scalar Jacobi with an
    // Iteration-only criterion on a Csr<double, int32> and one unit-stride column -- the smoother build_smoother makes --
    // runs as gkomi_multigrid_jacobi_sweeps_f64_i32 where detail::multigrid_fused says so, else as copy + advanced SpMV
    // + scalar_apply: the same bits; both run on buffers this solver keeps and add no synchronisation.  Anything else:
    // the guess is prepared and the plain apply runs.
    void apply_with_initial_guess(const LinOp* b, LinOp* x, initial_guess_mode guess) const override
    {
        if (jacobi_sweeps_as(V{}, b, x, guess)) return;
        prepare_initial_guess(b, x, guess);
        this->apply_impl(b, x);
    }
protected:
    friend class detail::factory_base<Ir>;
    Ir(const Factory* f, std::shared_ptr<const LinOp> A) : base(f, std::move(A)), relaxation_factor_(f->relaxation_factor_)
    {
        this->set_default_initial_guess(f->guess_);
    }
    bool jacobi_sweeps_as(float, const LinOp*, LinOp*, initial_guess_mode) const { return false; }
    bool jacobi_sweeps_as(double, const LinOp* b, LinOp* x, initial_guess_mode guess) const
    {
        const auto& st = this->settings_;
        auto jac = dynamic_cast<const preconditioner::Jacobi<double, int32>*>(this->precond_.get());
        auto A = dynamic_cast<const matrix::Csr<double, int32>*>(this->A_.get());
        auto db = dynamic_cast<const matrix::Dense<double>*>(b);
        auto dx = dynamic_cast<matrix::Dense<double>*>(x);
        if (!jac || jac->get_max_block_size() != 1 || !A || !db || !dx || st.implicit || st.reduction_factor != 0.0) return false;
        if (db->get_size()[1] != 1 || db->get_stride() != 1 || dx->get_stride() != 1) return false;
        ::gko::detail::require_device(this->exec_, "ir::apply");
        const int64_t n = this->size_[0];
        const bool zero = guess == initial_guess_mode::zero;
        if (guess == initial_guess_mode::rhs) dx->copy_from(db);
        // The sweep buffer, r and the three scalars are sized on the first call and kept (as Multigrid keeps its level
        // vectors), so a call only queues work on the stream: no allocation, no upload, no synchronisation.
        if (detail::multigrid_fused(A->get_num_stored_elements())) {
            const size_type need = gkomi_multigrid_jacobi_sweeps_workspace_bytes(n) + 8;
            if (sweep_ws_.get_num_elems() < need) sweep_ws_ = array<char>(this->exec_, need);
            GKOMI_CALL(gkomi_multigrid_jacobi_sweeps_f64_i32(nullptr, n, 1, A->get_num_stored_elements(), A->get_const_row_ptrs(), A->get_const_col_idxs(),
                                                             A->get_const_values(), jac->get_blocks(), relaxation_factor_, db->get_const_values(),
                                                             dx->get_values(), st.max_iters, zero ? 1 : 0, sweep_ws_.get_data(), sweep_ws_.get_num_elems()));
        } else {
            if (!sweep_r_) {
                sweep_one_ = initialize<matrix::Dense<double>>({1.0}, this->exec_);
                sweep_neg_one_ = initialize<matrix::Dense<double>>({-1.0}, this->exec_);
                sweep_relax_ = initialize<matrix::Dense<double>>({relaxation_factor_}, this->exec_);
                sweep_r_ = matrix::Dense<double>::create(this->exec_, dim<2>(n, 1));
            }
            auto r = sweep_r_.get();
            if (zero) dx->fill(0.0);
            for (int64_t it = 0; it < st.max_iters; ++it) {
                const matrix::Dense<double>* src = db;
                if (!(it == 0 && zero)) {
                    r->copy_from(db);
                    A->apply(sweep_neg_one_.get(), dx, sweep_one_.get(), r);
                    src = r;
                }
                jac->apply(sweep_relax_.get(), src, sweep_one_.get(), dx);
            }
        }
        this->last_iters_ = st.max_iters;
        this->last_converged_ = false;
        return true;
    }
    // Ir<double> over a generated Cg<float> on a Csr<float, int32> (the float copy of the Csr<double, int32> system),
    // both with Iteration + ResidualNorm, no inner preconditioner, one column: mixed-precision iterative refinement as one
    // native driver (gkomi_ir_mixed_solve_f64_i32).  false: not this configuration, the general path runs.
    bool mixed_as(float, const LinOp*, LinOp*) const { return false; }
    bool mixed_as(double, const LinOp* b, LinOp* x) const
    {
        const auto& st = this->settings_;
        auto inner = dynamic_cast<const Cg<float>*>(this->precond_.get());
        if (!inner || inner->get_preconditioner() || st.implicit || st.reduction_factor < 0) return false;
        const auto& is = inner->get_stop_settings();
        if (is.implicit || is.reduction_factor < 0) return false;
        auto A = dynamic_cast<const matrix::Csr<double, int32>*>(this->A_.get());
        auto Af = dynamic_cast<const matrix::Csr<float, int32>*>(inner->get_system_matrix().get());
        auto db = dynamic_cast<const matrix::Dense<double>*>(b);
        auto dx = dynamic_cast<matrix::Dense<double>*>(x);
        if (!A || !Af || !db || !dx || db->get_size()[1] != 1 || db->get_stride() != 1 || dx->get_stride() != 1) return false;
        if (Af->get_size() != A->get_size() || Af->get_num_stored_elements() != A->get_num_stored_elements()) return false;
        ::gko::detail::require_device(this->exec_, "ir::apply");
        const int64_t n = this->size_[0];
        array<char> ws(this->exec_, gkomi_ir_mixed_workspace_bytes(n));
        double info[6] = {};
        GKOMI_CALL(gkomi_ir_mixed_solve_f64_i32(nullptr, n, 1, A->get_num_stored_elements(), A->get_const_row_ptrs(), A->get_const_col_idxs(),
                                                A->get_const_values(), Af->get_const_values(), A->get_strategy()->get_code(), A->get_max_row_nnz(),
                                                db->get_const_values(), dx->get_values(), st.max_iters, st.reduction_factor,
                                                detail::baseline_code(st.baseline), is.max_iters, is.reduction_factor,
                                                detail::baseline_code(is.baseline), relaxation_factor_, ws.get_data(), ws.get_num_elems(), info));
        this->report(info);
        last_inner_iters_ = static_cast<int64_t>(info[4]);
        return true;
    }
    using base::apply_impl;
    void apply_impl(const LinOp* b, LinOp* x) const override
    {
        last_inner_iters_ = -1;
        if (mixed_as(V{}, b, x)) return;
        const auto& st = this->settings_;
        const LinOp* inner = this->precond_.get();
        typename base::operands f(*this, b, x);
        auto csr = as<const matrix::Csr<V, int32>>(this->A_.get());
        array<char> ws(this->exec_, gkomi_krylov_workspace_bytes(f.n, f.nrhs));
        ::gko::detail::linop_callback cb{inner, this->exec_, static_cast<size_type>(f.n), static_cast<size_type>(f.nrhs)};
        GKOMI_CALL(gkomi_ir_solve_f64_i32(nullptr, f.n, f.nrhs, csr->get_num_stored_elements(), csr->get_const_row_ptrs(), csr->get_const_col_idxs(), csr->get_const_values(),
                                          csr->get_strategy()->get_code(), csr->get_max_row_nnz(), inner ? &::gko::detail::linop_callback::call : nullptr, inner ? &cb : nullptr,
                                          relaxation_factor_, f.db->get_const_values(), f.dx->get_values(), st.max_iters, st.reduction_factor,
                                          detail::baseline_code(st.baseline), ws.get_data(), ws.get_num_elems(), f.info.data()));
        f.report();
    }
    V relaxation_factor_;
    mutable int64_t last_inner_iters_{-1};
    // state of jacobi_sweeps_as, allocated on its first call and reused
    mutable array<char> sweep_ws_;
    mutable std::unique_ptr<matrix::Dense<double>> sweep_r_, sweep_one_, sweep_neg_one_, sweep_relax_;
};

template <typename V = double>
class Gmres: public detail::iterative_solver<Gmres<V>> {
    using base = detail::iterative_solver<Gmres<V>>;
public:
    class Factory : public detail::factory_base<Gmres> {
    public:
        Factory& with_krylov_dim(size_type d) { krylov_dim_ = d; return *this; }
        size_type krylov_dim_{100};  // gmres.hpp:57,161
    };
    static Factory build() { return Factory{}; }
    size_type get_krylov_dim() const noexcept { return krylov_dim_; }
protected:
    friend class detail::factory_base<Gmres>;
    Gmres(const Factory* f, std::shared_ptr<const LinOp> A) : base(f, std::move(A)), krylov_dim_(f->krylov_dim_) {}
    using base::apply_impl;
    void apply_impl(const LinOp* b, LinOp* x) const override
    {
        const auto& st = this->settings_;
        typename base::frame f(*this, b, x);
        array<char> ws(this->exec_, gkomi_gmres_workspace_bytes(f.n, f.nrhs, krylov_dim_));
        GKOMI_CALL(gkomi_gmres_solve_op_f64(nullptr, f.n, f.nrhs, f.system.fn, f.system.ctx, f.precond.fn, f.precond.ctx, f.db->get_const_values(), f.dx->get_values(), krylov_dim_,
                                            st.max_iters, st.reduction_factor, detail::baseline_code(st.baseline), ws.get_data(), ws.get_num_elems(), f.info.data()));
        f.report();
    }
    size_type krylov_dim_;
};

// CbGmres (include/ginkgo/core/solver/cb_gmres.hpp): GMRES with a compressed Krylov basis.  The enumerators follow
// cb_gmres.hpp:88-95 and are the `storage` codes of gkomi_cb_gmres_*; for double: double, float, half, int64, int32, int16.
namespace cb_gmres {
enum class storage_precision { keep, reduce1, reduce2, integer, ireduce1, ireduce2 };
}  // namespace cb_gmres

template <typename V = double>
class CbGmres : public detail::iterative_solver<CbGmres<V>> {
    using base = detail::iterative_solver<CbGmres<V>>;
    static_assert(std::is_same<V, double>::value, "CbGmres: double only");
public:
    class Factory : public detail::factory_base<CbGmres> {
    public:
        Factory& with_krylov_dim(size_type d) { krylov_dim_ = d; return *this; }
        Factory& with_storage_precision(cb_gmres::storage_precision p) { storage_precision_ = p; return *this; }
        size_type krylov_dim_{100};  // cb_gmres.hpp:186, 161-162
        cb_gmres::storage_precision storage_precision_{cb_gmres::storage_precision::reduce1};
    };
    static Factory build() { return Factory{}; }
    size_type get_krylov_dim() const noexcept { return krylov_dim_; }
    cb_gmres::storage_precision get_storage_precision() const noexcept { return storage_precision_; }
    // how often the last apply checked a detected convergence by a forced restart (cb_gmres.cpp:315-383)
    int64_t get_last_forced_resets() const noexcept { return last_forced_resets_; }
protected:
    friend class detail::factory_base<CbGmres>;
    CbGmres(const Factory* f, std::shared_ptr<const LinOp> A)
        : base(f, std::move(A)), krylov_dim_(f->krylov_dim_), storage_precision_(f->storage_precision_) {}
    using base::apply_impl;
    void apply_impl(const LinOp* b, LinOp* x) const override
    {
        const auto& st = this->settings_;
        typename base::frame f(*this, b, x);
        const int storage = static_cast<int>(storage_precision_);
        f.info.assign(3 + 2 * f.nrhs, 0.0);  // this driver's record ends with the number of forced resets
        array<char> ws(this->exec_, gkomi_cb_gmres_workspace_bytes(f.n, f.nrhs, krylov_dim_, storage));
        GKOMI_CALL(gkomi_cb_gmres_solve_op_f64(nullptr, f.n, f.nrhs, f.system.fn, f.system.ctx, f.precond.fn, f.precond.ctx, f.db->get_const_values(), f.dx->get_values(),
                                               krylov_dim_, storage, st.max_iters, st.reduction_factor, detail::baseline_code(st.baseline), ws.get_data(), ws.get_num_elems(),
                                               f.info.data()));
        last_forced_resets_ = static_cast<int64_t>(f.info[2 + 2 * f.nrhs]);
        f.report();
    }
    size_type krylov_dim_;
    cb_gmres::storage_precision storage_precision_;
    mutable int64_t last_forced_resets_{0};
};

// LowerTrs / UpperTrs (include/ginkgo/core/solver/triangular.hpp)
template <bool Lower, typename V = double, typename I = int32>
class Trs : public LinOp {
public:
    class Factory : public LinOpFactory {
    public:
        Factory() : LinOpFactory(nullptr) {}
        Factory& with_unit_diagonal(bool u) { unit_ = u; return *this; }
        Factory& with_num_rhs(size_type) { return *this; }
        std::shared_ptr<Factory> on(std::shared_ptr<const Executor> exec) const { auto f = std::make_shared<Factory>(*this); f->exec_ = std::move(exec); return f; }
        std::unique_ptr<Trs> generate(std::shared_ptr<const LinOp> A) const { return std::unique_ptr<Trs>(new Trs(this->exec_, unit_, std::move(A))); }
        std::unique_ptr<LinOp> generate_impl(std::shared_ptr<const LinOp> A) const override { return generate(std::move(A)); }
        bool unit_{false};
    };
    static Factory build() { return Factory{}; }
protected:
public:
    // what generate() found: dependency levels of the factor and whether the level-scheduled solve is used
    int64_t get_num_levels() const noexcept { return nlevels_; }
    bool uses_level_schedule() const noexcept { return planned_; }
    bool uses_brick_plan() const noexcept { return bricks_ != nullptr; }
    bool has_unit_diagonal() const noexcept { return unit_; }
    // what gkomi_ilu_ctx carries of an analysed factor: its brick plan, else its level plan, else nothing
    void fill_callback_record(void*& level_plan, int64_t& nslices, int64_t& entries, int64_t& max_deps, gkomi_trs_bricks*& bricks, void*& bricks_plan) const
    {
        level_plan = nullptr; bricks = nullptr; bricks_plan = nullptr; nslices = 0; entries = 0; max_deps = -1;
        if (bricks_ != nullptr) {
            bricks = bricks_;
            bricks_plan = const_cast<char*>(plan_.get_const_data());
        } else if (planned_) {
            level_plan = const_cast<char*>(plan_.get_const_data());
            nslices = nslices_; entries = entries_; max_deps = max_deps_;
        }
    }
    ~Trs() override { gkomi_trs_bricks_destroy(bricks_); }
    // a solve that gave up (spin bound) left NaNs in x; sticky until the next generate
    bool has_overrun() const
    {
        int flag = 0;
        if (bricks_ != nullptr) GKOMI_CALL(gkomi_trs_bricks_check_overrun(nullptr, plan_.get_const_data(), &flag));
        else if (planned_) GKOMI_CALL(gkomi_trs_plan_check_overrun(nullptr, plan_.get_const_data(), &flag));
        else GKOMI_CALL(gkomi_trs_check_overrun(nullptr, ws_.get_const_data(), &flag));
        return flag != 0;
    }
protected:
    // LowerTrs / UpperTrs::generate (core/solver/lower_trs.cpp generate -> lower_trs::generate): the
    // dependency-level analysis of the factor, kept for every apply (the reference's SolveStruct)
    Trs(std::shared_ptr<const Executor> exec, bool unit, std::shared_ptr<const LinOp> A)
        : LinOp(exec, A->get_size()), unit_(unit), A_(std::move(A)), ws_(exec, gkomi_trs_workspace_bytes()), plan_(exec)
    {
        if (!exec_->is_device()) return;
        ws_.fill(0);
        auto csr = as<const matrix::Csr<V, I>>(A_.get());
        const int64_t n = static_cast<int64_t>(size_[0]);
        // factors of grid problems (many levels, stencil-shaped): the brick plan -- bricks solved out of LDS,
        // about one LDS step per level instead of one memory hand-off (csrc/trs_bricks.hip).  Its analysis runs
        // on the device and says itself how many levels the factor has if its box geometry holds, so a factor
        // that takes the brick plan never pays for the level analysis (generate on the 108^3 ILU: 55 -> 7 ms).
        if (n >= 2) {
            const int err = gkomi_trs_bricks_create_i32(nullptr, n, csr->get_const_row_ptrs(), csr->get_const_col_idxs(), Lower ? 1 : 0, 0, 0, 0, &bricks_);
            if (err != GKOMI_SUCCESS && err != GKOMI_ENOTSUPPORTED) GKOMI_CALL(err);
            if (bricks_ != nullptr) {
                int64_t info[8] = {};
                GKOMI_CALL(gkomi_trs_bricks_info(bricks_, info));
                const int64_t levels = gkomi_trs_bricks_levels_estimate(bricks_);
                if (gkomi_trs_prefer_bricks(n, levels, info[1]) != 0) {  // the cost model of profiles/r02_trs_bricks.md (+ the single-workgroup solve of small factors)
                    nlevels_ = levels;
                    plan_.resize_and_reset(gkomi_trs_bricks_plan_bytes(bricks_));
                    GKOMI_CALL(gkomi_trs_bricks_numeric_f64_i32(nullptr, bricks_, csr->get_const_row_ptrs(), csr->get_const_col_idxs(), csr->get_const_values(), plan_.get_data(),
                                                                plan_.get_num_elems()));
                    return;
                }
                gkomi_trs_bricks_destroy(bricks_);
                bricks_ = nullptr;
            }
        }
        array<char> symbolic(exec_, gkomi_trs_symbolic_workspace_bytes(n));
        int64_t out[4] = {};
        GKOMI_CALL(gkomi_trs_analyse_symbolic_i32(nullptr, n, csr->get_const_row_ptrs(), csr->get_const_col_idxs(), Lower ? 1 : 0, symbolic.get_data(),
                                                  symbolic.get_num_elems(), out));
        nslices_ = out[0]; entries_ = out[1]; nlevels_ = out[2]; max_deps_ = out[3];
        // wide levels: level-scheduled; chains and narrow bands: the analysis-free kernel's in-workgroup hand-offs
        planned_ = gkomi_trs_use_plan(n, nlevels_, max_deps_) != 0;
        if (planned_) {
            plan_.resize_and_reset(gkomi_trs_plan_bytes(nslices_, entries_));
            GKOMI_CALL(gkomi_trs_analyse_numeric_f64_i32(nullptr, n, csr->get_const_row_ptrs(), csr->get_const_col_idxs(), csr->get_const_values(), Lower ? 1 : 0,
                                                         symbolic.get_const_data(), nslices_, entries_, nlevels_, plan_.get_data(), plan_.get_num_elems()));
            GKOMI_CALL(gkomi_synchronize(nullptr));  // `symbolic` goes out of scope
        }
    }
    void apply_impl(const LinOp* b, LinOp* x) const override
    {
        ::gko::detail::require_device(exec_, "trs::solve");
        auto csr = as<const matrix::Csr<V, I>>(A_.get());
        auto db = matrix::detail_fmt::dense(b); auto dx = matrix::detail_fmt::dense(x);
        if (bricks_ != nullptr) {
            GKOMI_CALL(gkomi_trs_bricks_solve_f64(nullptr, bricks_, const_cast<char*>(plan_.get_const_data()), db->cols(), unit_ ? 1 : 0, db->get_const_values(), db->get_stride(),
                                                  dx->get_values(), dx->get_stride()));
            return;
        }
        if (planned_) {
            GKOMI_CALL(gkomi_trs_solve_plan_f64(nullptr, size_[0], db->cols(), const_cast<char*>(plan_.get_const_data()), nslices_, entries_, max_deps_, unit_ ? 1 : 0,
                                                db->get_const_values(), db->get_stride(), dx->get_values(), dx->get_stride()));
            return;
        }
        auto fn = Lower ? gkomi_lower_trs_solve_f64_i32 : gkomi_upper_trs_solve_f64_i32;
        GKOMI_CALL(fn(nullptr, size_[0], db->cols(), csr->get_const_row_ptrs(), csr->get_const_col_idxs(), csr->get_const_values(), unit_ ? 1 : 0, db->get_const_values(), db->get_stride(),
                      dx->get_values(), dx->get_stride(), const_cast<char*>(ws_.get_const_data()), ws_.get_num_elems()));
    }
    void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const override
    {
        auto dx = matrix::detail_fmt::dense(x);
        auto x_clone = dx->clone();
        this->apply_impl(b, x_clone.get());
        dx->scale(matrix::detail_fmt::dense(beta));
        dx->add_scaled(matrix::detail_fmt::dense(alpha), x_clone.get());
    }
    bool unit_;
    std::shared_ptr<const LinOp> A_;
    array<char> ws_;
    array<char> plan_;
    int64_t nslices_{0}, entries_{0}, nlevels_{0}, max_deps_{-1};
    bool planned_{false};
    gkomi_trs_bricks* bricks_{nullptr};  // host-side analysis; its device plan lives in plan_
};
template <typename V = double, typename I = int32>
using LowerTrs = Trs<true, V, I>;
template <typename V = double, typename I = int32>
using UpperTrs = Trs<false, V, I>;
}  // namespace solver

// ---- the factorizations: ParIlu, Ilu, Ic, ParIlut, ParIc, ParIct ---------------------------------------------------
// (core/factorization/par_ilu.cpp:74-163, ilu.cpp:67-124, ic.cpp:67-120, par_ilut.cpp:190-344, par_ic.cpp:70-145,
// par_ict.cpp:174-292)
namespace factorization {
// The pieces of a generate chain, each once.  A helper that is handed its workspace launches and returns: the caller
// keeps the workspace alive and hoists it out of its loop.  A helper that owns its workspace ends in a blocking read of
// a count, or synchronizes before the workspace leaves scope.
namespace detail {
using ::gko::detail::require_device;

// a square CSR matrix as its three arrays
template <typename V, typename I>
struct csr_arrays {
    array<I> rp, ci;
    array<V> v;
    csr_arrays() = default;
    csr_arrays(const std::shared_ptr<const Executor>& exec, size_type n, size_type nnz = 0) : rp(exec, n + 1), ci(exec, nnz), v(exec, nnz) {}
    int64_t nnz() const { return static_cast<int64_t>(v.get_num_elems()); }
    // fresh col_idxs and vals of nnz entries under the row pointers there are
    void resize(size_type nnz)
    {
        ci = array<I>(rp.get_executor(), nnz);
        v = array<V>(rp.get_executor(), nnz);
    }
    std::shared_ptr<matrix::Csr<V, I>> to_csr(std::shared_ptr<typename matrix::Csr<V, I>::strategy_type> strategy = nullptr) &&
    {
        const size_type n = rp.get_num_elems() - 1;
        std::shared_ptr<matrix::Csr<V, I>> m = matrix::Csr<V, I>::create(rp.get_executor());
        m->adopt(dim<2>(n, n), std::move(rp), std::move(ci), std::move(v));
        if (strategy) m->set_strategy(std::move(strategy));
        return m;
    }
};

// what the kernels read of a csr_arrays or a matrix::Csr
template <typename V, typename I>
struct csr_view {
    csr_view(const csr_arrays<V, I>& m) : n(m.rp.get_num_elems() - 1), nnz(m.nnz()), rp(m.rp.get_const_data()), ci(m.ci.get_const_data()), v(m.v.get_const_data()) {}
    csr_view(const matrix::Csr<V, I>* m)
        : n(m->get_size()[0]), nnz(static_cast<int64_t>(m->get_num_stored_elements())), rp(m->get_const_row_ptrs()), ci(m->get_const_col_idxs()), v(m->get_const_values())
    {}
    size_type n;
    int64_t nnz;
    const I* rp;
    const I* ci;
    const V* v;
};

// the matrix a generate reads: a Csr on the device, square, its rows sorted by column index where asked
template <typename V, typename I>
struct source {
    source(const std::shared_ptr<const Executor>& exec, const LinOp* A, const char* kernel, const std::string& who, bool sort)
    {
        static_assert(std::is_same<V, double>::value && std::is_same<I, int32>::value, "the factorizations are <double, int32>");
        require_device(exec, kernel);
        mtx = as<const matrix::Csr<V, I>>(A);
        n = mtx->get_size()[0];
        if (n != mtx->get_size()[1]) throw DimensionMismatch(__FILE__, __LINE__, who + " needs a square matrix");
        if (sort && !mtx->is_sorted_by_column_index()) {
            matrix_data<V, I> d;
            mtx->write(d);
            sorted_ = matrix::Csr<V, I>::create(exec);
            sorted_->read(d);
            sorted_->sort_by_column_index();
            mtx = sorted_.get();
        }
    }
    const matrix::Csr<V, I>* mtx;
    size_type n;
private:
    std::unique_ptr<matrix::Csr<V, I>> sorted_;
};

// factorization::add_diagonal_elements on a copy; ws: gkomi_factorization_workspace_bytes(n)
template <typename V, typename I>
csr_arrays<V, I> with_diagonal(const std::shared_ptr<const Executor>& exec, const matrix::Csr<V, I>* src, array<char>& ws)
{
    const size_type n = src->get_size()[0], nnz = src->get_num_stored_elements();
    csr_arrays<V, I> w(exec, n);
    exec->copy(n + 1, src->get_const_row_ptrs(), w.rp.get_data());
    int64_t missing = 0;
    GKOMI_CALL(gkomi_factorization_count_missing_diagonal_i32(nullptr, n, n, w.rp.get_const_data(), src->get_const_col_idxs(), ws.get_data(), ws.get_num_elems(), &missing));
    w.resize(nnz + missing);
    if (missing) {
        GKOMI_CALL(gkomi_factorization_add_diagonal_elements_f64_i32(nullptr, n, n, w.rp.get_data(), src->get_const_col_idxs(), src->get_const_values(), w.ci.get_data(), w.v.get_data(), ws.get_const_data()));
    } else {
        exec->copy(nnz, src->get_const_col_idxs(), w.ci.get_data());
        exec->copy(nnz, src->get_const_values(), w.v.get_data());
    }
    return w;
}

// factorization::initialize_row_ptrs_l_u + initialize_l_u: (L with a unit diagonal, U)
template <typename V, typename I>
std::pair<csr_arrays<V, I>, csr_arrays<V, I>> split_l_u(const std::shared_ptr<const Executor>& exec, csr_view<V, I> a)
{
    const size_type n = a.n;
    csr_arrays<V, I> l(exec, n), u(exec, n);
    {   // the scan's workspace goes while the stream is idle behind the blocking reads, not behind the launch below
        array<char> sws(exec, gkomi_prefix_sum_workspace_bytes(n + 1) + 8);
        GKOMI_CALL(gkomi_factorization_initialize_row_ptrs_l_u_i32(nullptr, n, a.rp, a.ci, l.rp.get_data(), u.rp.get_data(), sws.get_data(), sws.get_num_elems()));
        const size_type lnnz = exec->copy_val_to_host(l.rp.get_const_data() + n), unnz = exec->copy_val_to_host(u.rp.get_const_data() + n);
        l.resize(lnnz);
        u.resize(unnz);
    }
    GKOMI_CALL(gkomi_factorization_initialize_l_u_f64_i32(nullptr, n, a.rp, a.ci, a.v, l.rp.get_const_data(), l.ci.get_data(), l.v.get_data(), u.rp.get_const_data(), u.ci.get_data(), u.v.get_data()));
    return {std::move(l), std::move(u)};
}

// factorization::initialize_row_ptrs_l + initialize_l; diag_sqrt: the root of the diagonal is stored
template <typename V, typename I>
csr_arrays<V, I> split_l(const std::shared_ptr<const Executor>& exec, csr_view<V, I> a, bool diag_sqrt)
{
    const size_type n = a.n;
    csr_arrays<V, I> l(exec, n);
    {   // as in split_l_u
        array<char> sws(exec, gkomi_prefix_sum_workspace_bytes(n + 1) + 8);
        GKOMI_CALL(gkomi_factorization_initialize_row_ptrs_l_i32(nullptr, n, a.rp, a.ci, l.rp.get_data(), sws.get_data(), sws.get_num_elems()));
        l.resize(exec->copy_val_to_host(l.rp.get_const_data() + n));
    }
    GKOMI_CALL(gkomi_factorization_initialize_l_f64_i32(nullptr, n, a.rp, a.ci, a.v, l.rp.get_const_data(), l.ci.get_data(), l.v.get_data(), diag_sqrt ? 1 : 0));
    return l;
}

// out = m^T into arrays of m's sizes; ws: gkomi_csr_transpose_workspace_bytes(n)
template <typename V, typename I>
void transpose_into(csr_view<V, I> m, csr_arrays<V, I>& out, array<char>& ws)
{
    GKOMI_CALL(gkomi_csr_transpose_f64_i32(nullptr, m.n, m.n, m.nnz, m.rp, m.ci, m.v, out.rp.get_data(), out.ci.get_data(), out.v.get_data(), ws.get_data(), ws.get_num_elems()));
}

// m^T; without a workspace of the caller's it brings its own and waits for the transpose
template <typename V, typename I>
csr_arrays<V, I> transposed(const std::shared_ptr<const Executor>& exec, csr_view<V, I> m, array<char>* ws = nullptr)
{
    csr_arrays<V, I> out(exec, m.n, m.nnz);
    if (ws != nullptr) {
        transpose_into(m, out, *ws);
    } else {
        array<char> own(exec, gkomi_csr_transpose_workspace_bytes(m.n));
        transpose_into(m, out, own);
        exec->synchronize();  // the workspace leaves scope
    }
    return out;
}

// csr::spgemm a b, count then fill; ws: gkomi_csr_spgemm_workspace_bytes(n, n)
template <typename V, typename I>
csr_arrays<V, I> spgemm(const std::shared_ptr<const Executor>& exec, csr_view<V, I> a, csr_view<V, I> b, array<char>& ws)
{
    const size_type n = a.n;
    csr_arrays<V, I> c(exec, n);
    int64_t nnz = 0;
    auto call = [&] {
        GKOMI_CALL(gkomi_csr_spgemm_f64_i32(nullptr, n, n, a.nnz, a.rp, a.ci, a.v, n, n, b.nnz, b.rp, b.ci, b.v, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, c.rp.get_data(), c.ci.get_data(),
                                            c.v.get_data(), &nnz, ws.get_data(), ws.get_num_elems()));
    };
    call();
    c.resize(nnz);
    if (nnz > 0) call();
    return c;
}

// par_ilut_factorization::threshold_filter: the reference executor's keeps |v| >= threshold || col == row whatever its `lower` flag says
template <typename V, typename I>
csr_arrays<V, I> filtered(const std::shared_ptr<const Executor>& exec, csr_view<V, I> m, double threshold)
{
    csr_arrays<V, I> out(exec, m.n);
    array<char> ws(exec, gkomi_par_ilut_filter_workspace_bytes(m.n));
    int64_t nnz = 0;
    auto call = [&] {
        GKOMI_CALL(gkomi_par_ilut_threshold_filter_f64_i32(nullptr, m.n, m.rp, m.ci, m.v, threshold, out.rp.get_data(), out.ci.get_data(), out.v.get_data(), nullptr, &nnz, ws.get_data(), ws.get_num_elems()));
    };
    call();
    out.resize(nnz);
    call();
    return out;
}

// the magnitude of a rank among the values of a candidate factor: the sampled selection of threshold_filter_approx or
// the exact threshold_select, 0 without a launch for n == 0.  One workspace for the thresholds of one iteration.
template <typename V>
class threshold {
public:
    threshold(const std::shared_ptr<const Executor>& exec, size_type n, bool approximate, int64_t max_nnz)
        : skip_(n == 0), approximate_(approximate), ws_(exec, skip_ ? 0 : (approximate ? gkomi_par_ilut_approx_workspace_bytes() : gkomi_par_ilut_select_workspace_bytes(max_nnz)))
    {}
    double operator()(const array<V>& vals, int64_t rank)
    {
        double t = 0.0;
        if (skip_) return t;
        auto select = approximate_ ? gkomi_par_ilut_threshold_approx_f64 : gkomi_par_ilut_threshold_select_f64;
        GKOMI_CALL(select(nullptr, static_cast<int64_t>(vals.get_num_elems()), vals.get_const_data(), rank, ws_.get_data(), ws_.get_num_elems(), &t));
        return t;
    }
private:
    bool skip_, approximate_;
    array<char> ws_;
};

// on(), generate() and the executor of a factorization's Factory; the class itself keeps build(), its with_* and getters
template <typename Fact>
class factory_base {
public:
    std::shared_ptr<typename Fact::Factory> on(std::shared_ptr<const Executor> exec) const
    {
        auto f = std::make_shared<typename Fact::Factory>(static_cast<const typename Fact::Factory&>(*this));
        f->exec_ = std::move(exec);
        return f;
    }
    std::unique_ptr<Fact> generate(std::shared_ptr<const LinOp> A) const { return std::unique_ptr<Fact>(new Fact(static_cast<const typename Fact::Factory&>(*this), std::move(A))); }
    std::shared_ptr<const Executor> exec_;
};

// the working copy both exact chains factorize: sorted unless skipped, explicit diagonal, then gkomi_ilu_analyse_i32
// + the numeric phase in place
template <typename V, typename I>
csr_arrays<V, I> exact_factorized(const std::shared_ptr<const Executor>& exec, const LinOp* A, bool skip_sorting, bool ic, const char* who)
{
    source<V, I> src(exec, A, who, who, !skip_sorting);
    const size_type n = src.n;
    array<char> fws(exec, gkomi_factorization_workspace_bytes(n));
    auto w = with_diagonal(exec, src.mtx, fws);
    array<char> aws(exec, gkomi_ilu_analysis_workspace_bytes(n));
    int64_t info[6] = {};
    GKOMI_CALL(gkomi_ilu_analyse_i32(nullptr, n, w.rp.get_const_data(), w.ci.get_const_data(), aws.get_data(), aws.get_num_elems(), info));
    auto compute = ic ? gkomi_ic_compute_f64_i32 : gkomi_ilu_compute_lu_f64_i32;
    GKOMI_CALL(compute(nullptr, n, w.rp.get_const_data(), w.ci.get_const_data(), w.v.get_data(), aws.get_const_data(), aws.get_num_elems()));
    exec->synchronize();  // the workspaces leave scope
    return w;
}
}  // namespace detail

template <typename V = double, typename I = int32>
class ParIlu {
public:
    using matrix_type = matrix::Csr<V, I>;
    class Factory : public detail::factory_base<ParIlu> {
    public:
        Factory& with_iterations(size_type n) { iterations_ = n; return *this; }
        Factory& with_skip_sorting(bool) { return *this; }
        size_type iterations_{0};
    };
    static Factory build() { return Factory{}; }
    std::shared_ptr<const matrix_type> get_l_factor() const { return l_; }
    std::shared_ptr<const matrix_type> get_u_factor() const { return u_; }
protected:
    friend class detail::factory_base<ParIlu>;
    ParIlu(const Factory& f, std::shared_ptr<const LinOp> A)
    {
        const auto& exec = f.exec_;
        detail::source<V, I> src(exec, A.get(), "par_ilu_factorization", "ParIlu", false);
        const size_type n = src.n;
        array<char> fws(exec, gkomi_factorization_workspace_bytes(n)), tws(exec, gkomi_csr_transpose_workspace_bytes(n));
        auto w = detail::with_diagonal(exec, src.mtx, fws);
        auto lu = detail::split_l_u<V, I>(exec, w);
        auto& l = lu.first; auto& u = lu.second;
        auto ut = detail::transposed<V, I>(exec, u, &tws);
        array<I> rows(exec, w.nnz());
        GKOMI_CALL(gkomi_convert_ptrs_to_idxs_i32(nullptr, w.rp.get_const_data(), n, rows.get_data()));
        GKOMI_CALL(gkomi_par_ilu_compute_l_u_factors_f64_i32(nullptr, f.iterations_, w.nnz(), rows.get_const_data(), w.ci.get_const_data(), w.v.get_const_data(), l.rp.get_const_data(), l.ci.get_const_data(), l.v.get_data(),
                                                             ut.rp.get_const_data(), ut.ci.get_const_data(), ut.v.get_data()));
        detail::transpose_into<V, I>(ut, u, tws);
        l_ = std::move(l).to_csr(); u_ = std::move(u).to_csr();
    }
    std::shared_ptr<matrix_type> l_, u_;
};

template <typename V = double, typename I = int32>
class Ilu {
public:
    using matrix_type = matrix::Csr<V, I>;
    class Factory : public detail::factory_base<Ilu> {
    public:
        Factory& with_skip_sorting(bool skip) { skip_sorting_ = skip; return *this; }
        Factory& with_l_strategy(std::shared_ptr<typename matrix_type::strategy_type> s) { l_strategy_ = std::move(s); return *this; }
        Factory& with_u_strategy(std::shared_ptr<typename matrix_type::strategy_type> s) { u_strategy_ = std::move(s); return *this; }
        bool skip_sorting_{false};
        std::shared_ptr<typename matrix_type::strategy_type> l_strategy_, u_strategy_;
    };
    static Factory build() { return Factory{}; }
    std::shared_ptr<const matrix_type> get_l_factor() const { return l_; }
    std::shared_ptr<const matrix_type> get_u_factor() const { return u_; }
protected:
    friend class detail::factory_base<Ilu>;
    Ilu(const Factory& f, std::shared_ptr<const LinOp> A)
    {
        auto w = detail::exact_factorized<V, I>(f.exec_, A.get(), f.skip_sorting_, false, "ilu_factorization");
        auto lu = detail::split_l_u<V, I>(f.exec_, w);
        l_ = std::move(lu.first).to_csr(f.l_strategy_); u_ = std::move(lu.second).to_csr(f.u_strategy_);
    }
    std::shared_ptr<matrix_type> l_, u_;
};

template <typename V = double, typename I = int32>
class Ic {
public:
    using matrix_type = matrix::Csr<V, I>;
    class Factory : public detail::factory_base<Ic> {
    public:
        Factory& with_skip_sorting(bool skip) { skip_sorting_ = skip; return *this; }
        Factory& with_both_factors(bool both) { both_factors_ = both; return *this; }
        Factory& with_l_strategy(std::shared_ptr<typename matrix_type::strategy_type> s) { l_strategy_ = std::move(s); return *this; }
        bool skip_sorting_{false}, both_factors_{true};
        std::shared_ptr<typename matrix_type::strategy_type> l_strategy_;
    };
    static Factory build() { return Factory{}; }
    std::shared_ptr<const matrix_type> get_l_factor() const { return l_; }
    // nullptr when generated with_both_factors(false)
    std::shared_ptr<const matrix_type> get_lt_factor() const { return lt_; }
protected:
    friend class detail::factory_base<Ic>;
    Ic(const Factory& f, std::shared_ptr<const LinOp> A)
    {
        auto w = detail::exact_factorized<V, I>(f.exec_, A.get(), f.skip_sorting_, true, "ic_factorization");
        l_ = detail::split_l<V, I>(f.exec_, w, false).to_csr(f.l_strategy_);
        if (f.both_factors_) lt_ = l_->transpose();
    }
    std::shared_ptr<matrix_type> l_, lt_;
};

// ParIlut, the threshold ILU.  The factors are the reference executor's, bit for bit: its sweep is sequential and in
// place, so its result is determined by the pattern, and the device reproduces it with a level schedule (csrc/par_ilut.hip).
template <typename V = double, typename I = int32>
class ParIlut {
public:
    using matrix_type = matrix::Csr<V, I>;
    class Factory : public detail::factory_base<ParIlut> {
    public:
        Factory& with_iterations(size_type n) { iterations_ = n; return *this; }
        Factory& with_skip_sorting(bool skip) { skip_sorting_ = skip; return *this; }
        Factory& with_approximate_select(bool approximate) { approximate_select_ = approximate; return *this; }
        // the reference executor's sample is deterministic either way; so is this one
        Factory& with_deterministic_sample(bool deterministic) { deterministic_sample_ = deterministic; return *this; }
        Factory& with_fill_in_limit(double limit) { fill_in_limit_ = limit; return *this; }
        Factory& with_l_strategy(std::shared_ptr<typename matrix_type::strategy_type> s) { l_strategy_ = std::move(s); return *this; }
        Factory& with_u_strategy(std::shared_ptr<typename matrix_type::strategy_type> s) { u_strategy_ = std::move(s); return *this; }
        size_type iterations_{5};
        bool skip_sorting_{false}, approximate_select_{true}, deterministic_sample_{false};
        double fill_in_limit_{2.0};
        std::shared_ptr<typename matrix_type::strategy_type> l_strategy_, u_strategy_;
    };
    static Factory build() { return Factory{}; }
    std::shared_ptr<const matrix_type> get_l_factor() const { return l_; }
    std::shared_ptr<const matrix_type> get_u_factor() const { return u_; }
protected:
    friend class detail::factory_base<ParIlut>;
    using factor = detail::csr_arrays<V, I>;
    using view = detail::csr_view<V, I>;
    // compute_l_u_factors in place; ut: the CSC copy of u whose values are brought up to date, or nullptr
    static void sweep(const std::shared_ptr<const Executor>& exec, view a, factor& l, factor& u, factor* ut)
    {
        const size_type n = a.n;
        array<char> ws(exec, gkomi_par_ilut_sweep_workspace_bytes(n, l.nnz(), u.nnz()));
        int64_t info[6] = {};
        GKOMI_CALL(gkomi_par_ilut_analyse_i32(nullptr, n, l.nnz(), l.rp.get_const_data(), l.ci.get_const_data(), u.nnz(), u.rp.get_const_data(), u.ci.get_const_data(), ws.get_data(), ws.get_num_elems(), info));
        GKOMI_CALL(gkomi_par_ilut_compute_l_u_factors_f64_i32(nullptr, n, a.rp, a.ci, a.v, l.nnz(), l.rp.get_const_data(), l.ci.get_const_data(), l.v.get_data(), u.nnz(), u.rp.get_const_data(),
                                                              u.ci.get_const_data(), u.v.get_data(), ut ? ut->rp.get_const_data() : nullptr, ut ? ut->ci.get_const_data() : nullptr,
                                                              ut ? ut->v.get_data() : nullptr, ws.get_const_data(), ws.get_num_elems()));
        exec->synchronize();  // the workspace leaves scope
    }
    ParIlut(const Factory& f, std::shared_ptr<const LinOp> A)
    {
        const auto& exec = f.exec_;
        detail::source<V, I> src(exec, A.get(), "par_ilut_factorization", "ParIlut", !f.skip_sorting_);
        // GKO_ASSERT_EQ(parameters_.fill_in_limit > 0.0, true)
        if (!(f.fill_in_limit_ > 0.0)) throw ValueMismatch(__FILE__, __LINE__, "ParIlut needs fill_in_limit > 0");
        const size_type n = src.n;
        const view a(src.mtx);
        auto lu0 = detail::split_l_u<V, I>(exec, a);
        factor l = std::move(lu0.first), u = std::move(lu0.second);
        const int64_t l_nnz_limit = static_cast<I>(l.nnz() * f.fill_in_limit_), u_nnz_limit = static_cast<I>(u.nnz() * f.fill_in_limit_);
        array<char> gws(exec, gkomi_csr_spgemm_workspace_bytes(n, n)), cws(exec, gkomi_par_ilut_add_candidates_workspace_bytes(n));
        array<char> tws(exec, gkomi_csr_transpose_workspace_bytes(n));
        for (size_type it = 0; it < f.iterations_; ++it) {
            auto lu = detail::spgemm<V, I>(exec, l, u, gws);
            // the candidates L', U'
            factor l_new(exec, n), u_new(exec, n);
            int64_t l_new_nnz = 0, u_new_nnz = 0;
            auto add_candidates = [&] {
                GKOMI_CALL(gkomi_par_ilut_add_candidates_f64_i32(nullptr, n, lu.rp.get_const_data(), lu.ci.get_const_data(), lu.v.get_const_data(), a.rp, a.ci, a.v, l.rp.get_const_data(), l.ci.get_const_data(),
                                                                 l.v.get_const_data(), u.rp.get_const_data(), u.ci.get_const_data(), u.v.get_const_data(), l_new.rp.get_data(), l_new.ci.get_data(), l_new.v.get_data(),
                                                                 u_new.rp.get_data(), u_new.ci.get_data(), u_new.v.get_data(), &l_new_nnz, &u_new_nnz, cws.get_data(), cws.get_num_elems()));
            };
            add_candidates();
            l_new.resize(l_new_nnz);
            u_new.resize(u_new_nnz);
            if (n > 0) add_candidates();
            // U' by columns only where the order of its values matters: the approximate selection samples it
            factor u_new_csc;
            if (f.approximate_select_) u_new_csc = detail::transposed<V, I>(exec, u_new, &tws);
            sweep(exec, a, l_new, u_new, f.approximate_select_ ? &u_new_csc : nullptr);
            const int64_t l_rank = std::max<int64_t>(0, l_new_nnz - l_nnz_limit - 1), u_rank = std::max<int64_t>(0, u_new_nnz - u_nnz_limit - 1);
            detail::threshold<V> select(exec, n, f.approximate_select_, std::max(l_new_nnz, u_new_nnz));
            const double l_threshold = select(l_new.v, l_rank), u_threshold = select(f.approximate_select_ ? u_new_csc.v : u_new.v, u_rank);
            l = detail::filtered<V, I>(exec, l_new, l_threshold);
            u = detail::filtered<V, I>(exec, u_new, u_threshold);
            sweep(exec, a, l, u, nullptr);
        }
        l_ = std::move(l).to_csr(f.l_strategy_); u_ = std::move(u).to_csr(f.u_strategy_);
    }
    std::shared_ptr<matrix_type> l_, u_;
};

template <typename V = double, typename I = int32>
class ParIc {
public:
    using matrix_type = matrix::Csr<V, I>;
    class Factory : public detail::factory_base<ParIc> {
    public:
        Factory& with_iterations(size_type n) { iterations_ = n; return *this; }
        Factory& with_skip_sorting(bool) { return *this; }
        Factory& with_both_factors(bool) { return *this; }
        size_type iterations_{0};
    };
    static Factory build() { return Factory{}; }
    std::shared_ptr<const matrix_type> get_l_factor() const { return l_; }
    std::shared_ptr<const matrix_type> get_lt_factor() const { return lt_; }
protected:
    friend class detail::factory_base<ParIc>;
    ParIc(const Factory& f, std::shared_ptr<const LinOp> A)
    {
        const auto& exec = f.exec_;
        detail::source<V, I> src(exec, A.get(), "par_ic_factorization", "ParIc", false);
        const size_type n = src.n;
        array<char> fws(exec, gkomi_factorization_workspace_bytes(n));
        auto w = detail::with_diagonal(exec, src.mtx, fws);
        auto l = detail::split_l<V, I>(exec, w, false);
        array<I> rows(exec, l.nnz());
        array<V> a_vals(exec, l.v);  // the COO copy of the lower triangle (par_ic.cpp:121-131)
        GKOMI_CALL(gkomi_convert_ptrs_to_idxs_i32(nullptr, l.rp.get_const_data(), n, rows.get_data()));
        GKOMI_CALL(gkomi_par_ic_init_factor_f64_i32(nullptr, n, l.rp.get_const_data(), l.ci.get_const_data(), l.v.get_data()));
        GKOMI_CALL(gkomi_par_ic_compute_factor_f64_i32(nullptr, f.iterations_, l.nnz(), rows.get_const_data(), a_vals.get_const_data(), l.rp.get_const_data(), l.ci.get_const_data(), l.v.get_data()));
        l_ = std::move(l).to_csr();
        lt_ = l_->transpose();
    }
    std::shared_ptr<matrix_type> l_, lt_;
};

// ParIct, the threshold IC.  The factor is the reference executor's, bit for bit: its sweep is sequential and in place,
// so its result is determined by the pattern, and the device reproduces it with a level schedule (csrc/par_ict.hip).
// Selection and filter are those of ParIlut.
template <typename V = double, typename I = int32>
class ParIct {
public:
    using matrix_type = matrix::Csr<V, I>;
    class Factory : public detail::factory_base<ParIct> {
    public:
        Factory& with_iterations(size_type n) { iterations_ = n; return *this; }
        Factory& with_skip_sorting(bool skip) { skip_sorting_ = skip; return *this; }
        Factory& with_approximate_select(bool approximate) { approximate_select_ = approximate; return *this; }
        // the reference executor's sample is deterministic either way; so is this one
        Factory& with_deterministic_sample(bool deterministic) { deterministic_sample_ = deterministic; return *this; }
        Factory& with_fill_in_limit(double limit) { fill_in_limit_ = limit; return *this; }
        Factory& with_l_strategy(std::shared_ptr<typename matrix_type::strategy_type> s) { l_strategy_ = std::move(s); return *this; }
        Factory& with_lt_strategy(std::shared_ptr<typename matrix_type::strategy_type> s) { lt_strategy_ = std::move(s); return *this; }
        size_type iterations_{5};
        bool skip_sorting_{false}, approximate_select_{true}, deterministic_sample_{false};
        double fill_in_limit_{2.0};
        std::shared_ptr<typename matrix_type::strategy_type> l_strategy_, lt_strategy_;
    };
    static Factory build() { return Factory{}; }
    std::shared_ptr<const matrix_type> get_l_factor() const { return l_; }
    std::shared_ptr<const matrix_type> get_lt_factor() const { return lt_; }
protected:
    friend class detail::factory_base<ParIct>;
    using factor = detail::csr_arrays<V, I>;
    using view = detail::csr_view<V, I>;
    // compute_factor in place
    static void sweep(const std::shared_ptr<const Executor>& exec, view a, factor& l)
    {
        const size_type n = a.n;
        array<char> ws(exec, gkomi_par_ict_sweep_workspace_bytes(n, l.nnz()));
        int64_t info[6] = {};
        GKOMI_CALL(gkomi_par_ict_analyse_i32(nullptr, n, l.nnz(), l.rp.get_const_data(), l.ci.get_const_data(), ws.get_data(), ws.get_num_elems(), info));
        GKOMI_CALL(gkomi_par_ict_compute_factor_f64_i32(nullptr, n, a.rp, a.ci, a.v, l.nnz(), l.rp.get_const_data(), l.ci.get_const_data(), l.v.get_data(), ws.get_const_data(), ws.get_num_elems()));
        exec->synchronize();  // the workspace leaves scope
    }
    ParIct(const Factory& f, std::shared_ptr<const LinOp> A)
    {
        const auto& exec = f.exec_;
        detail::source<V, I> src(exec, A.get(), "par_ict_factorization", "ParIct", !f.skip_sorting_);
        // GKO_ASSERT_EQ(parameters_.fill_in_limit > 0.0, true)
        if (!(f.fill_in_limit_ > 0.0)) throw ValueMismatch(__FILE__, __LINE__, "ParIct needs fill_in_limit > 0");
        const size_type n = src.n;
        const view a(src.mtx);
        factor l = detail::split_l<V, I>(exec, a, true);
        const int64_t l_nnz_limit = static_cast<I>(l.nnz() * f.fill_in_limit_);
        array<char> gws(exec, gkomi_csr_spgemm_workspace_bytes(n, n)), cws(exec, gkomi_par_ict_add_candidates_workspace_bytes(n));
        factor lt = detail::transposed<V, I>(exec, l);
        for (size_type it = 0; it < f.iterations_; ++it) {
            auto llh = detail::spgemm<V, I>(exec, l, lt, gws);
            // the candidates L'
            factor l_new(exec, n);
            int64_t l_new_nnz = 0;
            auto add_candidates = [&] {
                GKOMI_CALL(gkomi_par_ict_add_candidates_f64_i32(nullptr, n, llh.rp.get_const_data(), llh.ci.get_const_data(), llh.v.get_const_data(), a.rp, a.ci, a.v, l.rp.get_const_data(), l.ci.get_const_data(),
                                                                l.v.get_const_data(), l_new.rp.get_data(), l_new.ci.get_data(), l_new.v.get_data(), &l_new_nnz, cws.get_data(), cws.get_num_elems()));
            };
            add_candidates();
            l_new.resize(l_new_nnz);
            if (n > 0) add_candidates();
            sweep(exec, a, l_new);
            const int64_t rank = std::max<int64_t>(0, l_new_nnz - l_nnz_limit - 1);
            l = detail::filtered<V, I>(exec, l_new, detail::threshold<V>(exec, n, f.approximate_select_, l_new_nnz)(l_new.v, rank));
            sweep(exec, a, l);
            lt = detail::transposed<V, I>(exec, l);
        }
        l_ = std::move(l).to_csr(f.l_strategy_); lt_ = std::move(lt).to_csr(f.lt_strategy_);
    }
    std::shared_ptr<matrix_type> l_, lt_;
};
}  // namespace factorization

// ---- preconditioner::Ilu and Ic (include/ginkgo/core/preconditioner/ilu.hpp:265-305, ic.hpp) -------------------------
// ---- Composition (include/ginkgo/core/base/composition.hpp): what SpdIsai needs of it and no more -- create from
// operators, get_operators(), and the apply through intermediates: x = op[0] (op[1] (... op[k-1] b)).
template <typename V = double>
class Composition : public LinOp {
public:
    template <typename... Rest>
    static std::unique_ptr<Composition> create(std::shared_ptr<const LinOp> first, Rest&&... rest)
    {
        std::unique_ptr<Composition> c(new Composition(first->get_executor()));
        c->add(std::move(first));
        int each[] = {0, (c->add(std::shared_ptr<const LinOp>(std::forward<Rest>(rest))), 0)...};
        (void)each;
        return c;
    }
    const std::vector<std::shared_ptr<const LinOp>>& get_operators() const noexcept { return operators_; }
protected:
    explicit Composition(std::shared_ptr<const Executor> exec) : LinOp(std::move(exec)) {}
    void add(std::shared_ptr<const LinOp> op)
    {
        if (!operators_.empty() && operators_.back()->get_size()[1] != op->get_size()[0]) {
            throw DimensionMismatch(__FILE__, __LINE__, "Composition: the operators do not conform");
        }
        operators_.push_back(std::move(op));
        this->set_size(dim<2>(operators_.front()->get_size()[0], operators_.back()->get_size()[1]));
    }
    void apply_impl(const LinOp* b, LinOp* x) const override
    {
        std::vector<std::unique_ptr<matrix::Dense<V>>> mids;
        const LinOp* in = b;
        for (size_type k = operators_.size(); k-- > 1;) {
            mids.push_back(matrix::Dense<V>::create(exec_, dim<2>(operators_[k]->get_size()[0], b->get_size()[1])));
            operators_[k]->apply(in, mids.back().get());
            in = mids.back().get();
        }
        operators_[0]->apply(in, x);
    }
    void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const override
    {
        auto dx = matrix::detail_fmt::dense(x);
        auto x_clone = dx->clone();
        this->apply_impl(b, x_clone.get());
        dx->scale(matrix::detail_fmt::dense(beta));
        dx->add_scaled(matrix::detail_fmt::dense(alpha), x_clone.get());
    }
    std::vector<std::shared_ptr<const LinOp>> operators_;
};

namespace preconditioner {
// ---- Isai (include/ginkgo/core/preconditioner/isai.hpp, core/preconditioner/isai.cpp:87-265) --------------------------
// The incomplete sparse approximate inverse of a triangular, general or spd matrix on the sparsity pattern of one of
// its powers, generated on the device by the gkomi_isai_* kernels with the reference executor's results; every apply is
// one CSR SpMV (two for spd).  <double, int32>.
enum struct isai_type { lower, upper, general, spd };

namespace detail {
using ::gko::detail::fill_csr_ctx;
// the record of gkomi_isai_apply_cb over one or two inverses; mid: n x nrhs scratch for two
inline void fill_isai_ctx(gkomi_isai_ctx& r, size_type n, size_type nrhs, const matrix::Csr<double, int32>* first, const matrix::Csr<double, int32>* second, double* mid)
{
    r = gkomi_isai_ctx{};
    r.n = static_cast<int64_t>(n);
    r.nrhs = static_cast<int64_t>(nrhs);
    r.num_matrices = second != nullptr ? 2 : 1;
    fill_csr_ctx(first, r.first);
    if (second != nullptr) fill_csr_ctx(second, r.second);
    r.intermediate = mid;
}
}  // namespace detail

template <isai_type Type, typename V = double, typename I = int32>
class Isai : public LinOp, public Transposable, public ::gko::detail::native_preconditioner {
    template <isai_type, typename, typename>
    friend class Isai;
public:
    using value_type = V;
    using index_type = I;
    using Csr = matrix::Csr<V, I>;
    using Comp = Composition<V>;
    using transposed_type = Isai<Type == isai_type::general ? isai_type::general : Type == isai_type::spd ? isai_type::spd : Type == isai_type::lower ? isai_type::upper : isai_type::lower, V, I>;
    using inverse_type = typename std::conditional<Type == isai_type::spd, Comp, Csr>::type;
    static constexpr isai_type type{Type};

    class Factory : public LinOpFactory {
    public:
        Factory() : LinOpFactory(nullptr) {}
        Factory& with_skip_sorting(bool s) { skip_sorting_ = s; return *this; }
        Factory& with_sparsity_power(int p) { sparsity_power_ = p; return *this; }
        Factory& with_excess_limit(size_type l) { excess_limit_ = l; return *this; }
        Factory& with_excess_solver_factory(std::shared_ptr<const LinOpFactory> f) { excess_solver_factory_ = std::move(f); return *this; }
        std::shared_ptr<Factory> on(std::shared_ptr<const Executor> exec) const { auto f = std::make_shared<Factory>(*this); f->exec_ = std::move(exec); return f; }
        std::unique_ptr<Isai> generate(std::shared_ptr<const LinOp> A) const { return std::unique_ptr<Isai>(new Isai(*this, std::move(A))); }
        std::unique_ptr<LinOp> generate_impl(std::shared_ptr<const LinOp> A) const override { return generate(std::move(A)); }
        bool skip_sorting_{false};
        int sparsity_power_{1};
        size_type excess_limit_{0};
        std::shared_ptr<const LinOpFactory> excess_solver_factory_;
    };
    static Factory build() { return Factory{}; }

    // the approximate inverse: a Csr, for spd the Composition (L^T, L)
    std::shared_ptr<const inverse_type> get_approximate_inverse() const { return std::dynamic_pointer_cast<const inverse_type>(approximate_inverse_); }

    // isai.cpp:321-345: spd is its own transpose, any other kind the transposed kind over the transposed inverse
    std::unique_ptr<LinOp> transpose() const override
    {
        if (Type == isai_type::spd) return std::unique_ptr<LinOp>(new Isai(*this));
        std::unique_ptr<transposed_type> t(new transposed_type(exec_, dim<2>(size_[1], size_[0])));
        t->approximate_inverse_ = share(dynamic_cast<const Csr&>(*approximate_inverse_).transpose());
        return std::unique_ptr<LinOp>(t.release());
    }

    // one SpMV, or L then L^T, as gkomi_isai_apply_cb + record
    bool native_callback(gkomi_apply_fn& fn, void*& ctx, size_type nrhs) const override
    {
        if (!std::is_same<V, double>::value || !std::is_same<I, int32>::value || !approximate_inverse_) return false;
        const size_type n = size_[0];
        if (Type == isai_type::spd) {
            const auto& ops = dynamic_cast<const Comp&>(*approximate_inverse_).get_operators();
            if (mid_.get_num_elems() != n * nrhs || mid_.get_executor() == nullptr) mid_ = array<V>(exec_, n * nrhs);
            ::gko::preconditioner::detail::fill_isai_ctx(record_, n, nrhs, dynamic_cast<const Csr*>(ops[1].get()), dynamic_cast<const Csr*>(ops[0].get()), mid_.get_data());
        } else {
            ::gko::preconditioner::detail::fill_isai_ctx(record_, n, nrhs, dynamic_cast<const Csr*>(approximate_inverse_.get()), nullptr, nullptr);
        }
        fn = &gkomi_isai_apply_cb;
        ctx = &record_;
        return true;
    }
    // the inverse as a Csr (not for spd): what Ilu / Ic put into their two-SpMV record
    const Csr* inverse_csr() const { return dynamic_cast<const Csr*>(approximate_inverse_.get()); }

protected:
    Isai(std::shared_ptr<const Executor> exec, dim<2> size) : LinOp(std::move(exec), size) {}
    Isai(const Isai&) = default;
    Isai(const Factory& f, std::shared_ptr<const LinOp> A) : LinOp(f.get_executor(), A->get_size())
    {
        generate_inverse(A.get(), f.skip_sorting_, f.sparsity_power_, f.excess_limit_, f.excess_solver_factory_);
    }
    void apply_impl(const LinOp* b, LinOp* x) const override { approximate_inverse_->apply(b, x); }
    void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const override { approximate_inverse_->apply(alpha, b, beta, x); }

    // Isai::generate_inverse (isai.cpp:121-265)
    void generate_inverse(const LinOp* input, bool skip_sorting, int power, size_type excess_limit, const std::shared_ptr<const LinOpFactory>& excess_solver_factory)
    {
        namespace fd = ::gko::factorization::detail;
        using arrays = fd::csr_arrays<V, I>;
        using view = fd::csr_view<V, I>;
        using Dense = matrix::Dense<V>;
        constexpr bool is_lower = Type == isai_type::lower, is_spd = Type == isai_type::spd;
        constexpr bool is_tri = is_lower || Type == isai_type::upper;
        if (power < 1) throw ValueMismatch(__FILE__, __LINE__, "Isai: sparsity_power must be at least 1");
        fd::source<V, I> src(exec_, input, "isai::generate_inverse", "Isai", !skip_sorting);
        const size_type n = src.n;
        const view m(src.mtx);
        auto copy_of = [&](view a) {
            arrays c(exec_, a.n, static_cast<size_type>(a.nnz));
            exec_->copy(a.n + 1, a.rp, c.rp.get_data());
            exec_->copy(static_cast<size_type>(a.nnz), a.ci, c.ci.get_data());
            exec_->copy(static_cast<size_type>(a.nnz), a.v, c.v.get_data());
            return c;
        };
        // extend_sparsity (:87-118): square-and-multiply through csr::spgemm, as it is written there
        auto extend = [&](view a) {
            if (power == 1) return copy_of(a);
            array<char> ws(exec_, gkomi_csr_spgemm_workspace_bytes(n, n));
            arrays id_power = copy_of(a), acc = copy_of(a);
            auto product = [&](const arrays& p, const arrays& q) {
                arrays r = fd::spgemm(exec_, view(p), view(q), ws);
                exec_->synchronize();  // before an operand is released
                return r;
            };
            int i = power - 1;
            while (i > 1) {
                if (i % 2 != 0) {
                    acc = product(id_power, acc);
                    i--;
                }
                id_power = product(id_power, id_power);
                i /= 2;
            }
            return product(id_power, acc);
        };
        arrays inv;
        if (!is_spd) {
            inv = extend(m);
        } else {
            arrays base = fd::split_l(exec_, m, false);
            exec_->synchronize();
            inv = power == 1 ? std::move(base) : extend(view(base));
        }
        array<I> rhs_ptrs(exec_, n + 1), nz_ptrs(exec_, n + 1);
        {
            array<char> ws(exec_, gkomi_isai_generate_workspace_bytes(n) + 8);
            auto gen = is_tri ? gkomi_isai_generate_tri_inverse_f64_i32 : gkomi_isai_generate_general_inverse_f64_i32;
            GKOMI_CALL(gen(nullptr, n, m.rp, m.ci, m.v, inv.rp.get_const_data(), inv.ci.get_const_data(), inv.v.get_data(), rhs_ptrs.get_data(), nz_ptrs.get_data(),
                           is_tri ? (is_lower ? 1 : 0) : (is_spd ? 1 : 0), ws.get_data(), ws.get_num_elems()));
            exec_->synchronize();
        }
        const auto host_rhs = rhs_ptrs.to_host(), host_nz = nz_ptrs.to_host();
        const size_type total = static_cast<size_type>(host_rhs[n]);
        const size_type lim = excess_limit == 0 ? total : excess_limit;
        size_type block = 0;
        while (total > 0 && block < n) {
            const size_type start = block;
            size_type e_dim = 0;
            for (; e_dim < lim && block < n; e_dim = static_cast<size_type>(host_rhs[block] - host_rhs[start])) block++;
            if (e_dim == 0) break;
            const size_type e_nnz = static_cast<size_type>(host_nz[block] - host_nz[start]);
            arrays sys(exec_, e_dim, e_nnz);
            auto rhs = Dense::create(exec_, dim<2>(e_dim, 1));
            auto sol = Dense::create(exec_, dim<2>(e_dim, 1));
            GKOMI_CALL(gkomi_isai_generate_excess_system_f64_i32(nullptr, n, m.rp, m.ci, m.v, inv.rp.get_const_data(), inv.ci.get_const_data(), rhs_ptrs.get_const_data(),
                                                                 nz_ptrs.get_const_data(), e_dim, e_nnz, sys.rp.get_data(), sys.ci.get_data(), sys.v.get_data(), rhs->get_values(), start,
                                                                 block));
            std::shared_ptr<const LinOp> sys_t = fd::transposed(exec_, view(sys)).to_csr();
            std::shared_ptr<const LinOpFactory> solver_factory;
            if (excess_solver_factory) {
                solver_factory = excess_solver_factory;
                sol->copy_from(rhs.get());
            } else if (!is_tri) {
                solver_factory = solver::Gmres<V>::build()
                                     .with_preconditioner(Jacobi<V, I>::build().with_max_block_size(32u).on(exec_))
                                     .with_criteria(stop::Iteration::build().with_max_iters(e_dim).on(exec_),
                                                    stop::ResidualNorm<V>::build().with_baseline(stop::mode::rhs_norm).with_reduction_factor(1e-6).on(exec_))
                                     .on(exec_);
                sol->copy_from(rhs.get());
            } else if (is_lower) {
                solver_factory = solver::UpperTrs<V, I>::build().on(exec_);
            } else {
                solver_factory = solver::LowerTrs<V, I>::build().on(exec_);
            }
            solver_factory->generate_impl(sys_t)->apply(rhs.get(), sol.get());
            if (is_spd) GKOMI_CALL(gkomi_isai_scale_excess_solution_f64_i32(nullptr, n, rhs_ptrs.get_const_data(), sol->get_values(), start, block));
            GKOMI_CALL(gkomi_isai_scatter_excess_solution_f64_i32(nullptr, n, rhs_ptrs.get_const_data(), sol->get_const_values(), inv.rp.get_const_data(), inv.v.get_data(), start, block));
            exec_->synchronize();  // the block's arrays leave scope
        }
        std::shared_ptr<Csr> inverse = std::move(inv).to_csr();
        if (is_spd) {
            approximate_inverse_ = share(Comp::create(share(inverse->transpose()), inverse));
        } else {
            approximate_inverse_ = inverse;
        }
    }
    std::shared_ptr<const LinOp> approximate_inverse_;
    mutable gkomi_isai_ctx record_{};
    mutable array<V> mid_;
};
template <typename V = double, typename I = int32>
using LowerIsai = Isai<isai_type::lower, V, I>;
template <typename V = double, typename I = int32>
using UpperIsai = Isai<isai_type::upper, V, I>;
template <typename V = double, typename I = int32>
using GeneralIsai = Isai<isai_type::general, V, I>;
template <typename V = double, typename I = int32>
using SpdIsai = Isai<isai_type::spd, V, I>;

namespace detail {
// What Ilu and Ic share: the two factors of whatever generates them, the solvers over them -- the triangular solvers
// unless a factory for them is given (ilu.hpp:349-356, ic.hpp:320-328) --, and the apply through one intermediate vector.
template <typename V, typename I>
class two_solves : public LinOp, public Transposable {
protected:
    two_solves(std::shared_ptr<const Executor> exec, dim<2> size) : LinOp(std::move(exec), size) {}
    // what a factorization's Factory generates of A, on this executor unless the factory has one
    template <class FactorizationFactory>
    auto generated(const FactorizationFactory& f, std::shared_ptr<const LinOp> A) const { return (f.exec_ ? f : *f.on(exec_)).generate(std::move(A)); }
    // upper_from_lower (Ic with an l_solver_factory, ic.hpp:327-328): the second solver is the conjugate transpose of
    // the first instead of a solver generated from the upper factor
    void set_factors(std::shared_ptr<const matrix::Csr<V, I>> lower, std::shared_ptr<const matrix::Csr<V, I>> upper,
                     const std::shared_ptr<const LinOpFactory>& lower_solver_factory = nullptr, const std::shared_ptr<const LinOpFactory>& upper_solver_factory = nullptr,
                     bool upper_from_lower = false)
    {
        lower_factor_ = std::move(lower);
        upper_factor_ = std::move(upper);
        if (lower_solver_factory) {
            lower_solver_ = share(lower_solver_factory->generate_impl(lower_factor_));
        } else {
            lower_solver_ = solver::LowerTrs<V, I>::build().on(exec_)->generate(lower_factor_);
        }
        if (upper_from_lower && lower_solver_factory) {
            auto t = dynamic_cast<const Transposable*>(lower_solver_.get());
            if (t == nullptr) GKO_NOT_SUPPORTED("Ic: the solver of l_solver_factory is not Transposable");
            upper_solver_ = share(t->conj_transpose());
        } else if (upper_solver_factory) {
            upper_solver_ = share(upper_solver_factory->generate_impl(upper_factor_));
        } else {
            upper_solver_ = solver::UpperTrs<V, I>::build().on(exec_)->generate(upper_factor_);
        }
    }
    // both solvers LowerIsai / UpperIsai: the two-SpMV record of gkomi_isai_apply_cb
    bool isai_callback(gkomi_apply_fn& fn, void*& ctx, size_type nrhs) const
    {
        if (!std::is_same<V, double>::value || !std::is_same<I, int32>::value) return false;
        auto l = dynamic_cast<const LowerIsai<V, I>*>(lower_solver_.get());
        auto u = dynamic_cast<const UpperIsai<V, I>*>(upper_solver_.get());
        if (l == nullptr || u == nullptr || l->inverse_csr() == nullptr || u->inverse_csr() == nullptr) return false;
        const size_type n = size_[0];
        if (isai_mid_.get_num_elems() != n * nrhs || isai_mid_.get_executor() == nullptr) isai_mid_ = array<V>(exec_, n * nrhs);
        fill_isai_ctx(isai_record_, n, nrhs, l->inverse_csr(), u->inverse_csr(), isai_mid_.get_data());
        fn = &gkomi_isai_apply_cb;
        ctx = &isai_record_;
        return true;
    }
    mutable gkomi_isai_ctx isai_record_{};
    mutable array<V> isai_mid_;
    void apply_impl(const LinOp* b, LinOp* x) const override
    {
        auto db = matrix::detail_fmt::dense(b);
        auto mid = matrix::Dense<V>::create(exec_, db->get_size());
        lower_solver_->apply(b, mid.get());
        upper_solver_->apply(mid.get(), x);
    }
    void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const override
    {
        auto dx = matrix::detail_fmt::dense(x);
        auto x_clone = dx->clone();
        this->apply_impl(b, x_clone.get());
        dx->scale(matrix::detail_fmt::dense(beta));
        dx->add_scaled(matrix::detail_fmt::dense(alpha), x_clone.get());
    }
    std::shared_ptr<const matrix::Csr<V, I>> lower_factor_, upper_factor_;
    std::shared_ptr<const LinOp> lower_solver_, upper_solver_;
};
}  // namespace detail

template <typename V = double, typename I = int32>
class Ilu : public detail::two_solves<V, I>, public ::gko::detail::native_preconditioner {
    using base = detail::two_solves<V, I>;
    using base::exec_; using base::size_; using base::lower_factor_; using base::upper_factor_; using base::lower_solver_; using base::upper_solver_;
public:
    // L^-1 then U^-1 as gkomi_ilu_apply_cb + record: the two brick solves of an apply then run as a chain (no launch
    // that pre-fills an output with the ready flags), and no Dense objects are built per apply.  The record, the
    // intermediate vector and the analysis-free kernels' workspace live in the object (the reference's Ilu caches its
    // intermediate too): one solve at a time per preconditioner object.
    bool native_callback(gkomi_apply_fn& fn, void*& ctx, size_type nrhs) const override
    {
        if (!std::is_same<V, double>::value || !std::is_same<I, int32>::value) return false;
        if (this->isai_callback(fn, ctx, nrhs)) return true;
        auto l = dynamic_cast<const solver::LowerTrs<V, I>*>(lower_solver_.get());
        auto u = dynamic_cast<const solver::UpperTrs<V, I>*>(upper_solver_.get());
        if (l == nullptr || u == nullptr || u->has_unit_diagonal()) return false;
        const size_type n = size_[0];
        if (mid_.get_num_elems() != n * nrhs || mid_.get_executor() == nullptr) {
            mid_ = array<V>(exec_, n * nrhs);
            mid_.fill(V{0});
            record_.pad_ = 0;
        }
        if (tws_.get_num_elems() == 0) {
            tws_ = array<char>(exec_, gkomi_trs_workspace_bytes());
            tws_.fill(0);
        }
        const int32_t chain_state = record_.pad_;
        record_ = gkomi_ilu_ctx{};
        record_.pad_ = chain_state;
        record_.n = static_cast<int64_t>(n);
        record_.nrhs = static_cast<int64_t>(nrhs);
        record_.l_row_ptrs = lower_factor_->get_const_row_ptrs();
        record_.l_col_idxs = lower_factor_->get_const_col_idxs();
        record_.l_vals = lower_factor_->get_const_values();
        record_.u_row_ptrs = upper_factor_->get_const_row_ptrs();
        record_.u_col_idxs = upper_factor_->get_const_col_idxs();
        record_.u_vals = upper_factor_->get_const_values();
        record_.intermediate = mid_.get_data();
        record_.trs_workspace = tws_.get_data();
        record_.trs_workspace_bytes = tws_.get_num_elems();
        record_.l_unit_diag = l->has_unit_diagonal() ? 1 : 0;
        l->fill_callback_record(record_.l_plan, record_.l_nslices, record_.l_entries, record_.l_max_deps, record_.l_bricks, record_.l_bricks_plan);
        u->fill_callback_record(record_.u_plan, record_.u_nslices, record_.u_entries, record_.u_max_deps, record_.u_bricks, record_.u_bricks_plan);
        fn = &gkomi_ilu_apply_cb;
        ctx = &record_;
        return true;
    }
    class Factory : public LinOpFactory {
    public:
        Factory() : LinOpFactory(nullptr) {}
        Factory& with_factorization_iterations(size_type n) { iterations_ = n; return *this; }
        std::shared_ptr<Factory> on(std::shared_ptr<const Executor> exec) const { auto f = std::make_shared<Factory>(*this); f->exec_ = std::move(exec); return f; }
        // the exact ILU(0) instead of the default ParIlu sweeps
        Factory& with_factorization_factory(std::shared_ptr<const typename ::gko::factorization::Ilu<V, I>::Factory> f) { exact_ = std::move(f); return *this; }
        // the threshold ILU
        Factory& with_factorization_factory(std::shared_ptr<const typename ::gko::factorization::ParIlut<V, I>::Factory> f) { ilut_ = std::move(f); return *this; }
        // the solvers generated from the factors (ilu.hpp:349-356) instead of LowerTrs / UpperTrs, e.g. LowerIsai / UpperIsai
        Factory& with_l_solver_factory(std::shared_ptr<const LinOpFactory> f) { l_solver_ = std::move(f); return *this; }
        Factory& with_u_solver_factory(std::shared_ptr<const LinOpFactory> f) { u_solver_ = std::move(f); return *this; }
        std::unique_ptr<Ilu> generate(std::shared_ptr<const LinOp> A) const
        {
            if (ilut_) return std::unique_ptr<Ilu>(new Ilu(*this, *ilut_, std::move(A)));
            if (exact_) return std::unique_ptr<Ilu>(new Ilu(*this, *exact_, std::move(A)));
            return std::unique_ptr<Ilu>(new Ilu(*this, ::gko::factorization::ParIlu<V, I>::build().with_iterations(iterations_), std::move(A)));
        }
        std::unique_ptr<LinOp> generate_impl(std::shared_ptr<const LinOp> A) const override { return generate(std::move(A)); }
        size_type iterations_{0};
        std::shared_ptr<const typename ::gko::factorization::Ilu<V, I>::Factory> exact_;
        std::shared_ptr<const typename ::gko::factorization::ParIlut<V, I>::Factory> ilut_;
        std::shared_ptr<const LinOpFactory> l_solver_, u_solver_;
    };
    static Factory build() { return Factory{}; }
    std::shared_ptr<const LinOp> get_l_solver() const { return lower_solver_; }
    std::shared_ptr<const LinOp> get_u_solver() const { return upper_solver_; }
    // Ilu::transpose (include/ginkgo/core/preconditioner/ilu.hpp:200-230): (U^-1 L^-1)^T =
    // L^-T U^-T, i.e. the lower solver of U^T followed by the upper solver of L^T
    std::unique_ptr<LinOp> transpose() const override
    {
        std::unique_ptr<Ilu> t(new Ilu(exec_, size_));
        t->set_factors(upper_factor_->transpose(), lower_factor_->transpose());
        return std::unique_ptr<LinOp>(t.release());
    }
protected:
    Ilu(std::shared_ptr<const Executor> exec, dim<2> size) : base(std::move(exec), size) {}
    // a factorization factory that gives get_l_factor() / get_u_factor(): factorization::ParIlu, Ilu or ParIlut
    template <class FactorizationFactory>
    Ilu(const Factory& own, const FactorizationFactory& f, std::shared_ptr<const LinOp> A) : base(own.get_executor(), A->get_size())
    {
        auto fact = this->generated(f, std::move(A));
        this->set_factors(fact->get_l_factor(), fact->get_u_factor(), own.l_solver_, own.u_solver_);
    }
    mutable gkomi_ilu_ctx record_{};
    mutable array<V> mid_;
    mutable array<char> tws_;
};

// Ic::apply = L^-1 then L^-H (ic.hpp: two triangular solves, like Ilu).  A solver reaches it through the generic
// callback, except over LowerIsai, where both solvers are SpMVs and gkomi_isai_apply_cb runs them.
template <typename V = double, typename I = int32>
class Ic : public detail::two_solves<V, I>, public ::gko::detail::native_preconditioner {
    using base = detail::two_solves<V, I>;
public:
    bool native_callback(gkomi_apply_fn& fn, void*& ctx, size_type nrhs) const override { return this->isai_callback(fn, ctx, nrhs); }
    // (L L^T)^-1 is symmetric: the transpose applies the same two solves
    std::unique_ptr<LinOp> transpose() const override { return std::unique_ptr<LinOp>(new Ic(*this)); }
    class Factory : public LinOpFactory {
    public:
        Factory() : LinOpFactory(nullptr) {}
        Factory& with_factorization_iterations(size_type n) { iterations_ = n; return *this; }
        std::shared_ptr<Factory> on(std::shared_ptr<const Executor> exec) const { auto f = std::make_shared<Factory>(*this); f->exec_ = std::move(exec); return f; }
        // the exact IC(0) instead of the default ParIc sweeps
        Factory& with_factorization_factory(std::shared_ptr<const typename ::gko::factorization::Ic<V, I>::Factory> f) { exact_ = std::move(f); return *this; }
        // the threshold IC
        Factory& with_factorization_factory(std::shared_ptr<const typename ::gko::factorization::ParIct<V, I>::Factory> f) { ict_ = std::move(f); return *this; }
        // the solver generated from L (ic.hpp:320-328) instead of LowerTrs, e.g. LowerIsai; the second solver is then its conjugate transpose
        Factory& with_l_solver_factory(std::shared_ptr<const LinOpFactory> f) { l_solver_ = std::move(f); return *this; }
        std::unique_ptr<Ic> generate(std::shared_ptr<const LinOp> A) const
        {
            if (ict_) return std::unique_ptr<Ic>(new Ic(*this, *ict_, std::move(A)));
            if (exact_) {
                auto both = *exact_;
                both.with_both_factors(true);  // the preconditioner needs L^T whatever the factory says
                return std::unique_ptr<Ic>(new Ic(*this, both, std::move(A)));
            }
            return std::unique_ptr<Ic>(new Ic(*this, ::gko::factorization::ParIc<V, I>::build().with_iterations(iterations_), std::move(A)));
        }
        std::unique_ptr<LinOp> generate_impl(std::shared_ptr<const LinOp> A) const override { return generate(std::move(A)); }
        size_type iterations_{0};
        std::shared_ptr<const typename ::gko::factorization::Ic<V, I>::Factory> exact_;
        std::shared_ptr<const typename ::gko::factorization::ParIct<V, I>::Factory> ict_;
        std::shared_ptr<const LinOpFactory> l_solver_;
    };
    static Factory build() { return Factory{}; }
    std::shared_ptr<const LinOp> get_l_solver() const { return this->lower_solver_; }
    std::shared_ptr<const LinOp> get_lh_solver() const { return this->upper_solver_; }
protected:
    Ic(const Ic&) = default;
    // a factorization factory that gives get_l_factor() / get_lt_factor(): factorization::ParIc, Ic or ParIct
    template <class FactorizationFactory>
    Ic(const Factory& own, const FactorizationFactory& f, std::shared_ptr<const LinOp> A) : base(own.get_executor(), A->get_size())
    {
        auto fact = this->generated(f, std::move(A));
        this->set_factors(fact->get_l_factor(), fact->get_lt_factor(), own.l_solver_, nullptr, true);
    }
};
}  // namespace preconditioner

// ---- the sparse direct solver: elimination forest, symbolic Cholesky, Lu, Direct --------------------
// (core/factorization/elimination_forest.hpp, symbolic.cpp:66-93, lu.cpp:85-145, core/solver/direct.cpp:131-227)
namespace factorization {
// core/factorization/elimination_forest.hpp: the pseudo-root of every tree is `size`; child_ptrs has size + 2 entries
template <typename I = int32>
struct elimination_forest {
    elimination_forest(std::shared_ptr<const Executor> exec, I size)
        : parents(exec, size), child_ptrs(exec, size + 2), children(exec, size), postorder(exec, size), inv_postorder(exec, size), postorder_parents(exec, size)
    {}
    array<I> parents, child_ptrs, children, postorder, inv_postorder, postorder_parents;
};

// compute_elim_forest (elimination_forest.cpp:183-207): host work on a copy of the pattern; the arrays live where the matrix does
template <typename V, typename I>
elimination_forest<I> compute_elim_forest(const matrix::Csr<V, I>* mtx)
{
    static_assert(std::is_same<I, int32>::value, "compute_elim_forest: int32 indices");
    auto exec = mtx->get_executor();
    const auto n = static_cast<I>(mtx->get_size()[0]);
    elimination_forest<I> f(exec, n);
    auto fn = exec->is_device() ? nullptr : gkomi_elimination_forest_host_i32;
    if (fn != nullptr) {
        GKOMI_CALL(fn(n, mtx->get_const_row_ptrs(), mtx->get_const_col_idxs(), f.parents.get_data(), f.child_ptrs.get_data(), f.children.get_data(), f.postorder.get_data(),
                      f.inv_postorder.get_data(), f.postorder_parents.get_data()));
    } else {
        GKOMI_CALL(gkomi_elimination_forest_i32(nullptr, n, mtx->get_const_row_ptrs(), mtx->get_const_col_idxs(), f.parents.get_data(), f.child_ptrs.get_data(), f.children.get_data(),
                                                f.postorder.get_data(), f.inv_postorder.get_data(), f.postorder_parents.get_data()));
    }
    return f;
}

// symbolic_cholesky (symbolic.cpp:66-93): the pattern of L + L^T with zero values, rows sorted
template <typename V, typename I>
std::unique_ptr<matrix::Csr<V, I>> symbolic_cholesky(const matrix::Csr<V, I>* mtx)
{
    static_assert(std::is_same<V, double>::value && std::is_same<I, int32>::value, "symbolic_cholesky is <double, int32>");
    using matrix_type = matrix::Csr<V, I>;
    auto exec = mtx->get_executor();
    ::gko::detail::require_device(exec, "cholesky::cholesky_symbolic_count");
    const size_type n = mtx->get_size()[0];
    const size_type nnz = mtx->get_num_stored_elements();
    const auto forest = compute_elim_forest(mtx);
    array<I> row_ptrs(exec, n + 1);
    row_ptrs.fill(0);
    array<char> ws(exec, gkomi_cholesky_symbolic_workspace_bytes(n, nnz) + 8);
    int64_t factor_nnz = 0;
    GKOMI_CALL(gkomi_cholesky_symbolic_count_i32(nullptr, n, nnz, mtx->get_const_row_ptrs(), mtx->get_const_col_idxs(), forest.inv_postorder.get_const_data(),
                                                 forest.postorder_parents.get_const_data(), row_ptrs.get_data(), ws.get_data(), ws.get_num_elems(), &factor_nnz));
    array<char> sws(exec, gkomi_prefix_sum_workspace_bytes(n + 1) + 8);
    GKOMI_CALL(gkomi_prefix_sum_i32(nullptr, row_ptrs.get_data(), n + 1, sws.get_data(), sws.get_num_elems()));
    array<I> cols(exec, static_cast<size_type>(factor_nnz));
    array<V> vals(exec, static_cast<size_type>(factor_nnz));
    vals.fill(V{});
    GKOMI_CALL(gkomi_cholesky_symbolic_factorize_i32(nullptr, n, nnz, mtx->get_const_row_ptrs(), mtx->get_const_col_idxs(), forest.postorder.get_const_data(),
                                                     forest.inv_postorder.get_const_data(), forest.postorder_parents.get_const_data(), row_ptrs.get_const_data(), cols.get_data(),
                                                     ws.get_data(), ws.get_num_elems()));
    GKOMI_CALL(gkomi_synchronize(nullptr));  // the workspaces leave scope
    auto factor = matrix_type::create(exec);
    factor->adopt(mtx->get_size(), std::move(row_ptrs), std::move(cols), std::move(vals));
    factor->sort_by_column_index();
    auto lt_factor = factor->transpose();
    auto scalar = matrix::Dense<V>::create(exec, dim<2>(1, 1));
    scalar->fill(V{1});
    auto id = matrix::Identity<V>::create(exec, n);
    lt_factor->apply(scalar.get(), id.get(), scalar.get(), factor.get());
    return factor;
}
}  // namespace factorization

namespace experimental {
namespace factorization {
// include/ginkgo/core/factorization/factorization.hpp: the storage types this backend produces
enum class storage_type { empty, composition, combined_lu };

template <typename V = double, typename I = int32>
class Factorization : public LinOp {
public:
    using matrix_type = matrix::Csr<V, I>;
    // L (strictly lower, unit diagonal not stored) and U in one matrix, as Lu::generate leaves them
    static std::unique_ptr<Factorization> create_from_combined_lu(std::unique_ptr<matrix_type> combined)
    {
        auto f = std::unique_ptr<Factorization>(new Factorization(combined->get_executor(), combined->get_size(), storage_type::combined_lu));
        f->combined_ = std::move(combined);
        return f;
    }
    static std::unique_ptr<Factorization> create_from_composition(std::shared_ptr<const matrix_type> l, std::shared_ptr<const matrix_type> u)
    {
        auto f = std::unique_ptr<Factorization>(new Factorization(l->get_executor(), l->get_size(), storage_type::composition));
        f->lower_ = std::move(l);
        f->upper_ = std::move(u);
        return f;
    }
    storage_type get_storage_type() const noexcept { return type_; }
    std::shared_ptr<const matrix_type> get_combined() const { return type_ == storage_type::combined_lu ? combined_ : nullptr; }
    std::shared_ptr<const matrix_type> get_lower_factor() const { return type_ == storage_type::composition ? lower_ : nullptr; }
    std::shared_ptr<const matrix_type> get_upper_factor() const { return type_ == storage_type::composition ? upper_ : nullptr; }
    // the composition L U: L with its unit diagonal stored, U with the diagonal, through factorization::initialize_l_u
    std::unique_ptr<Factorization> unpack() const
    {
        if (type_ == storage_type::composition) return create_from_composition(lower_, upper_);
        if (type_ == storage_type::empty) GKO_NOT_SUPPORTED("Factorization::unpack of an empty factorization");
        static_assert(std::is_same<V, double>::value && std::is_same<I, int32>::value, "Factorization is <double, int32>");
        const auto& exec = exec_;
        ::gko::detail::require_device(exec, "factorization::initialize_l_u");
        auto lu = ::gko::factorization::detail::split_l_u<V, I>(exec, combined_.get());
        GKOMI_CALL(gkomi_synchronize(nullptr));
        return create_from_composition(std::move(lu.first).to_csr(), std::move(lu.second).to_csr());
    }
protected:
    Factorization(std::shared_ptr<const Executor> exec, const dim<2>& size, storage_type type) : LinOp(std::move(exec), size), type_(type) {}
    // x = L U b
    void apply_impl(const LinOp* b, LinOp* x) const override
    {
        auto f = type_ == storage_type::composition ? nullptr : unpack();
        const auto& l = f ? f->lower_ : lower_;
        const auto& u = f ? f->upper_ : upper_;
        auto mid = matrix::Dense<V>::create(exec_, b->get_size());
        u->apply(b, mid.get());
        l->apply(mid.get(), x);
    }
    void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const override
    {
        auto f = type_ == storage_type::composition ? nullptr : unpack();
        const auto& l = f ? f->lower_ : lower_;
        const auto& u = f ? f->upper_ : upper_;
        auto mid = matrix::Dense<V>::create(exec_, b->get_size());
        u->apply(b, mid.get());
        l->apply(alpha, mid.get(), beta, x);
    }
    storage_type type_;
    std::shared_ptr<const matrix_type> combined_, lower_, upper_;
};

// experimental::factorization::Lu (core/factorization/lu.cpp:85-145)
template <typename V = double, typename I = int32>
class Lu {
public:
    using matrix_type = matrix::Csr<V, I>;
    using factorization_type = Factorization<V, I>;
    class Factory : public LinOpFactory {
    public:
        Factory() : LinOpFactory(nullptr) {}
        // the pattern of the factors (sorted rows, diagonal stored, closed under fill); copied at generate
        Factory& with_symbolic_factorization(std::shared_ptr<const matrix_type> s) { symbolic_ = std::move(s); return *this; }
        // without a symbolic factorization: take symbolic_cholesky of the matrix (its pattern must be symmetric)
        Factory& with_symmetric_sparsity(bool s) { symmetric_sparsity_ = s; return *this; }
        std::shared_ptr<Factory> on(std::shared_ptr<const Executor> exec) const { auto f = std::make_shared<Factory>(*this); f->exec_ = std::move(exec); return f; }
        std::unique_ptr<factorization_type> generate(std::shared_ptr<const LinOp> A) const
        {
            static_assert(std::is_same<V, double>::value && std::is_same<I, int32>::value, "Lu is <double, int32>");
            const auto& exec = this->exec_;
            ::gko::detail::require_device(exec, "lu_factorization::factorize");
            auto mtx = as<const matrix_type>(A.get());
            if (mtx->get_size()[0] != mtx->get_size()[1]) throw DimensionMismatch(__FILE__, __LINE__, "Lu needs a square matrix");
            const size_type n = mtx->get_size()[0];
            if (gkomi_lu_symbolic_supported(symbolic_ ? 1 : 0, symmetric_sparsity_ ? 1 : 0) != GKOMI_SUCCESS) {
                GKO_NOT_SUPPORTED("Lu::generate without a symbolic factorization needs with_symmetric_sparsity(true)");
            }
            std::unique_ptr<matrix_type> factors;
            if (!symbolic_) {
                factors = ::gko::factorization::symbolic_cholesky(mtx);
            } else {
                const size_type factor_nnz = symbolic_->get_num_stored_elements();
                array<I> rp(exec, n + 1), ci(exec, factor_nnz);
                array<V> v(exec, factor_nnz);
                exec->copy_from(symbolic_->get_executor().get(), factor_nnz, symbolic_->get_const_col_idxs(), ci.get_data());
                exec->copy_from(symbolic_->get_executor().get(), n + 1, symbolic_->get_const_row_ptrs(), rp.get_data());
                factors = matrix_type::create(exec);
                factors->adopt(mtx->get_size(), std::move(rp), std::move(ci), std::move(v));
            }
            const size_type factor_nnz = factors->get_num_stored_elements();
            // the level analysis first: it rejects rows that are not strictly ascending or lack their diagonal
            array<char> aws(exec, gkomi_ilu_analysis_workspace_bytes(n) + 8);
            int64_t info[6] = {};
            GKOMI_CALL(gkomi_ilu_analyse_i32(nullptr, n, factors->get_const_row_ptrs(), factors->get_const_col_idxs(), aws.get_data(), aws.get_num_elems(), info));
            array<I> diag_idxs(exec, n);
            array<char> flag(exec, 8);
            GKOMI_CALL(gkomi_lu_initialize_f64_i32(nullptr, n, mtx->get_const_row_ptrs(), mtx->get_const_col_idxs(), mtx->get_const_values(), factor_nnz,
                                                   factors->get_const_row_ptrs(), factors->get_const_col_idxs(), factors->get_values(), diag_idxs.get_data(), flag.get_data(),
                                                   flag.get_num_elems()));
            GKOMI_CALL(gkomi_lu_factorize_f64_i32(nullptr, n, factors->get_const_row_ptrs(), factors->get_const_col_idxs(), factors->get_values(), aws.get_const_data(),
                                                  aws.get_num_elems()));
            GKOMI_CALL(gkomi_synchronize(nullptr));  // the analysis leaves scope
            return factorization_type::create_from_combined_lu(std::move(factors));
        }
        std::unique_ptr<LinOp> generate_impl(std::shared_ptr<const LinOp> A) const override { return generate(std::move(A)); }
        std::shared_ptr<const matrix_type> symbolic_;
        bool symmetric_sparsity_{false};
    };
    static Factory build() { return Factory{}; }
};
}  // namespace factorization

namespace solver {
// experimental::solver::Direct (core/solver/direct.cpp:131-227): LowerTrs(unit_diagonal) then UpperTrs through one
// intermediate vector.  A combined factorization is unpacked first (Factorization::unpack): LowerTrs / UpperTrs::generate
// may pick the level plan or the brick plan, whose analyses are written for one-sided factors.  L then stores its unit
// diagonal, which a unit-diagonal solve does not read: the same bits as the solve on the combined matrix.
template <typename V = double, typename I = int32>
class Direct : public LinOp, public Transposable {
public:
    using factorization_type = ::gko::experimental::factorization::Factorization<V, I>;
    class Factory : public LinOpFactory {
    public:
        Factory() : LinOpFactory(nullptr) {}
        Factory& with_factorization(std::shared_ptr<const LinOpFactory> f) { factorization_ = std::move(f); return *this; }
        Factory& with_num_rhs(size_type n) { num_rhs_ = n; return *this; }
        std::shared_ptr<Factory> on(std::shared_ptr<const Executor> exec) const { auto f = std::make_shared<Factory>(*this); f->exec_ = std::move(exec); return f; }
        std::unique_ptr<Direct> generate(std::shared_ptr<const LinOp> A) const { return std::unique_ptr<Direct>(new Direct(this, std::move(A))); }
        std::unique_ptr<LinOp> generate_impl(std::shared_ptr<const LinOp> A) const override { return generate(std::move(A)); }
        std::shared_ptr<const LinOpFactory> factorization_;
        size_type num_rhs_{1};
    };
    static Factory build() { return Factory{}; }
    // the factorization (the reference's EnableSolverBase<Direct, Factorization>)
    std::shared_ptr<const factorization_type> get_system_matrix() const { return factors_; }
    std::unique_ptr<LinOp> transpose() const override { GKO_NOT_IMPLEMENTED; }
    std::unique_ptr<LinOp> conj_transpose() const override { GKO_NOT_IMPLEMENTED; }
protected:
    // a Factorization as the system matrix is taken as it is (direct.cpp:114-127)
    static std::shared_ptr<const factorization_type> generate_factorization(const Factory* f, std::shared_ptr<const LinOp> A)
    {
        if (auto given = std::dynamic_pointer_cast<const factorization_type>(A)) return given;
        if (!f->factorization_) GKO_NOT_SUPPORTED("Direct needs with_factorization(...) unless its system matrix is a Factorization");
        std::shared_ptr<LinOp> made = f->factorization_->generate_impl(std::move(A));
        auto fact = std::dynamic_pointer_cast<const factorization_type>(made);
        if (!fact) GKO_NOT_SUPPORTED("the factorization factory of Direct must produce a Factorization");
        return fact;
    }
    Direct(const Factory* f, std::shared_ptr<const LinOp> A) : LinOp(f->get_executor(), A->get_size()), factors_(generate_factorization(f, A))
    {
        using ::gko::experimental::factorization::storage_type;
        if (factors_->get_storage_type() == storage_type::empty) return;
        const bool combined = factors_->get_storage_type() == storage_type::combined_lu;
        std::shared_ptr<const factorization_type> split = combined ? std::shared_ptr<const factorization_type>(factors_->unpack()) : factors_;
        lower_solver_ = ::gko::solver::LowerTrs<V, I>::build().with_num_rhs(f->num_rhs_).with_unit_diagonal(combined).on(exec_)->generate(split->get_lower_factor());
        upper_solver_ = ::gko::solver::UpperTrs<V, I>::build().with_num_rhs(f->num_rhs_).with_unit_diagonal(false).on(exec_)->generate(split->get_upper_factor());
    }
    void apply_impl(const LinOp* b, LinOp* x) const override
    {
        if (!lower_solver_ || !upper_solver_) return;
        auto intermediate = matrix::Dense<V>::create(exec_, b->get_size());
        lower_solver_->apply(b, intermediate.get());
        upper_solver_->apply(intermediate.get(), x);
    }
    void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const override
    {
        if (!lower_solver_ || !upper_solver_) return;
        auto intermediate = matrix::Dense<V>::create(exec_, b->get_size());
        lower_solver_->apply(b, intermediate.get());
        upper_solver_->apply(alpha, intermediate.get(), beta, x);
    }
    std::shared_ptr<const factorization_type> factors_;
    std::shared_ptr<const LinOp> lower_solver_, upper_solver_;
};
}  // namespace solver
}  // namespace experimental

// ---- multigrid ------------------------------------------------------------------------------------------------------
namespace multigrid {

// include/ginkgo/core/multigrid/multigrid_level.hpp:60-95
class MultigridLevel {
public:
    virtual ~MultigridLevel() = default;
    virtual std::shared_ptr<const LinOp> get_fine_op() const = 0;
    virtual std::shared_ptr<const LinOp> get_restrict_op() const = 0;
    virtual std::shared_ptr<const LinOp> get_coarse_op() const = 0;
    virtual std::shared_ptr<const LinOp> get_prolong_op() const = 0;
};

// multigrid_level.hpp:109-200: the four operators; as a LinOp the level is prolong(coarse(restrict(b)))
template <typename V>
class EnableMultigridLevel : public MultigridLevel {
public:
    using value_type = V;
    std::shared_ptr<const LinOp> get_fine_op() const override { return fine_op_; }
    std::shared_ptr<const LinOp> get_restrict_op() const override { return restrict_op_; }
    std::shared_ptr<const LinOp> get_coarse_op() const override { return coarse_op_; }
    std::shared_ptr<const LinOp> get_prolong_op() const override { return prolong_op_; }
protected:
    EnableMultigridLevel() = default;
    explicit EnableMultigridLevel(std::shared_ptr<const LinOp> fine_op) : fine_op_(std::move(fine_op)) {}
    void set_multigrid_level(std::shared_ptr<const LinOp> prolong_op, std::shared_ptr<const LinOp> coarse_op, std::shared_ptr<const LinOp> restrict_op)
    {
        if (fine_op_->get_size() != dim<2>(prolong_op->get_size()[0], restrict_op->get_size()[1])) {
            throw DimensionMismatch(__FILE__, __LINE__, "prolong x restrict does not have the fine operator's size");
        }
        prolong_op_ = std::move(prolong_op);
        coarse_op_ = std::move(coarse_op);
        restrict_op_ = std::move(restrict_op);
    }
    void set_fine_op(std::shared_ptr<const LinOp> fine_op) { fine_op_ = std::move(fine_op); }
    // get_composition()->apply: alpha and beta act on the last factor (core/base/composition.cpp)
    void apply_composition(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const
    {
        auto exec = fine_op_->get_executor();
        const auto nrhs = b->get_size()[1];
        auto t1 = matrix::Dense<V>::create(exec, dim<2>(restrict_op_->get_size()[0], nrhs));
        auto t2 = matrix::Dense<V>::create(exec, dim<2>(coarse_op_->get_size()[0], nrhs));
        restrict_op_->apply(b, t1.get());
        coarse_op_->apply(t1.get(), t2.get());
        if (alpha) {
            prolong_op_->apply(alpha, t2.get(), beta, x);
        } else {
            prolong_op_->apply(t2.get(), x);
        }
    }
private:
    std::shared_ptr<const LinOp> fine_op_, restrict_op_, coarse_op_, prolong_op_;
};

// multigrid::FixedCoarsening (include/ginkgo/core/multigrid/fixed_coarsening.hpp, core/multigrid/fixed_coarsening.cpp:69-118):
// the coarse rows are given; R selects them, P = R^T, A_c = R (A P) through csr::transpose and two csr::spgemm.
// The system matrix is a Csr, or an Fbcsr, which comes in through Fbcsr::convert_to(Csr*); the mirror's Coo, Ell, Sellp and
// Hybrid have no conversion to Csr yet and are refused.
template <typename V = double, typename I = int32>
class FixedCoarsening : public LinOp, public EnableMultigridLevel<V> {
public:
    using csr_type = matrix::Csr<V, I>;
    class Factory : public LinOpFactory {
    public:
        Factory() : LinOpFactory(nullptr) {}
        Factory& with_coarse_rows(array<I> rows) { coarse_rows_ = std::move(rows); return *this; }
        Factory& with_skip_sorting(bool skip) { skip_sorting_ = skip; return *this; }
        std::shared_ptr<Factory> on(std::shared_ptr<const Executor> exec) const { auto f = std::make_shared<Factory>(*this); f->exec_ = std::move(exec); return f; }
        std::unique_ptr<FixedCoarsening> generate(std::shared_ptr<const LinOp> A) const { return std::unique_ptr<FixedCoarsening>(new FixedCoarsening(this, std::move(A))); }
        std::unique_ptr<LinOp> generate_impl(std::shared_ptr<const LinOp> A) const override { return generate(std::move(A)); }
        array<I> coarse_rows_;
        bool skip_sorting_{false};
    };
    static Factory build() { return Factory{}; }
    std::shared_ptr<const LinOp> get_system_matrix() const { return system_matrix_; }
protected:
    FixedCoarsening(const Factory* f, std::shared_ptr<const LinOp> A) : LinOp(f->get_executor(), A->get_size()), EnableMultigridLevel<V>(A), system_matrix_(std::move(A))
    {
        if (size_[0] != size_[1]) throw DimensionMismatch(__FILE__, __LINE__, "FixedCoarsening needs a square matrix");
        if (size_[0] != 0) this->generate(f);
    }
    void generate(const Factory* f)
    {
        ::gko::detail::require_device(exec_, "FixedCoarsening::generate");
        auto given = std::dynamic_pointer_cast<const csr_type>(system_matrix_);
        if (!given) {
            // fixed_coarsening.cpp:77-87: another format is converted and the Csr becomes the fine operator
            given = converted_to_csr(system_matrix_.get(), std::integral_constant<bool, std::is_same<V, double>::value && std::is_same<I, int32>::value>{});
            if (!given) GKO_NOT_SUPPORTED("FixedCoarsening: the system matrix must be a Csr or an Fbcsr");
            this->set_fine_op(given);
        }
        std::shared_ptr<const csr_type> fine = given;
        if (!f->skip_sorting_ && !given->is_sorted_by_column_index()) {
            auto sorted = csr_type::create(exec_, given->get_size(), given->get_num_stored_elements(), given->get_strategy());
            exec_->copy_from(exec_.get(), given->get_size()[0] + 1, given->get_const_row_ptrs(), sorted->get_row_ptrs());
            exec_->copy_from(exec_.get(), given->get_num_stored_elements(), given->get_const_col_idxs(), sorted->get_col_idxs());
            exec_->copy_from(exec_.get(), given->get_num_stored_elements(), given->get_const_values(), sorted->get_values());
            sorted->sort_by_column_index();
            fine = std::move(sorted);
            this->set_fine_op(fine);   // fixed_coarsening.cpp:87
        }
        const size_type coarse_dim = f->coarse_rows_.get_num_elems();
        if (coarse_dim == 0) GKO_NOT_SUPPORTED("FixedCoarsening: coarse_rows is empty");
        const size_type fine_dim = size_[0];
        auto restrict_op = std::shared_ptr<csr_type>(csr_type::create(exec_, dim<2>(coarse_dim, fine_dim), coarse_dim, fine->get_strategy()));
        exec_->copy_from(f->coarse_rows_.get_executor().get(), coarse_dim, f->coarse_rows_.get_const_data(), restrict_op->get_col_idxs());
        std::vector<V> ones(coarse_dim, V{1});
        std::vector<I> seq(coarse_dim + 1);
        for (size_type i = 0; i <= coarse_dim; ++i) seq[i] = static_cast<I>(i);
        exec_->copy_from(exec_->get_master().get(), coarse_dim, ones.data(), restrict_op->get_values());
        exec_->copy_from(exec_->get_master().get(), coarse_dim + 1, seq.data(), restrict_op->get_row_ptrs());
        auto prolong_op = std::shared_ptr<csr_type>(restrict_op->transpose());
        auto coarse = std::shared_ptr<csr_type>(csr_type::create(exec_, dim<2>(coarse_dim, coarse_dim), 0, fine->get_strategy()));
        auto tmp = csr_type::create(exec_, dim<2>(fine_dim, coarse_dim), 0, fine->get_strategy());
        fine->apply(prolong_op.get(), tmp.get());
        restrict_op->apply(tmp.get(), coarse.get());
        this->set_multigrid_level(prolong_op, coarse, restrict_op);
    }
    void apply_impl(const LinOp* b, LinOp* x) const override { this->apply_composition(nullptr, b, nullptr, x); }
    void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const override { this->apply_composition(alpha, b, beta, x); }
private:
    // the mirror's conversions to a Csr: Fbcsr<double, int32> has one; a null pointer for everything else
    static std::shared_ptr<const csr_type> converted_to_csr(const LinOp*, std::false_type) { return nullptr; }
    static std::shared_ptr<const csr_type> converted_to_csr(const LinOp* A, std::true_type)
    {
        auto fbcsr = dynamic_cast<const matrix::Fbcsr<double, int32>*>(A);
        if (!fbcsr) return nullptr;
        auto result = csr_type::create(A->get_executor());
        fbcsr->convert_to(result.get());
        return std::shared_ptr<const csr_type>(std::move(result));
    }
    std::shared_ptr<const LinOp> system_matrix_;
};

// multigrid::Pgm (include/ginkgo/core/multigrid/pgm.hpp, core/multigrid/pgm.cpp:147-236) through gkomi_pgm_generate_f64_i32:
// the aggregates, the restriction and the coarse matrix of the reference executor, all computed on the device.  The
// restriction (num_agg x n, sorted rows) and the prolongation (one entry per row at column agg[i]) are unit-valued Csr
// matrices, whose applies add what SparsityCsr's and RowGatherer's add in the same order; classes of their own are a
// follow-up.  The system matrix is a Csr, or an Fbcsr through its conversion.  When the matrix is sorted
// or converted the new Csr becomes the fine operator (pgm.cpp:163-169); with skip_sorting a Csr stays the caller's object.
template <typename V = double, typename I = int32>
class Pgm : public LinOp, public EnableMultigridLevel<V> {
public:
    using value_type = V;
    using index_type = I;
    using csr_type = matrix::Csr<V, I>;
    class Factory : public LinOpFactory {
    public:
        Factory() : LinOpFactory(nullptr) {}
        Factory& with_max_iterations(unsigned v) { max_iterations_ = v; return *this; }
        Factory& with_max_unassigned_ratio(double v) { max_unassigned_ratio_ = v; return *this; }
        Factory& with_deterministic(bool v) { deterministic_ = v; return *this; }
        Factory& with_skip_sorting(bool v) { skip_sorting_ = v; return *this; }
        std::shared_ptr<Factory> on(std::shared_ptr<const Executor> exec) const { auto f = std::make_shared<Factory>(*this); f->exec_ = std::move(exec); return f; }
        std::unique_ptr<Pgm> generate(std::shared_ptr<const LinOp> A) const { return std::unique_ptr<Pgm>(new Pgm(this, std::move(A))); }
        std::unique_ptr<LinOp> generate_impl(std::shared_ptr<const LinOp> A) const override { return generate(std::move(A)); }
        unsigned max_iterations_{15};
        double max_unassigned_ratio_{0.05};
        bool deterministic_{false};
        bool skip_sorting_{false};
    };
    static Factory build() { return Factory{}; }
    std::shared_ptr<const LinOp> get_system_matrix() const { return system_matrix_; }
    I* get_agg() noexcept { return agg_.get_data(); }
    const I* get_const_agg() const noexcept { return agg_.get_const_data(); }
protected:
    Pgm(const Factory* f, std::shared_ptr<const LinOp> A)
        : LinOp(f->get_executor(), A->get_size()), EnableMultigridLevel<V>(A), system_matrix_(std::move(A)), agg_(f->get_executor(), system_matrix_->get_size()[0])
    {
        if (size_[0] != size_[1]) throw DimensionMismatch(__FILE__, __LINE__, "Pgm needs a square matrix");
        if (size_[0] != 0) this->generate(f, std::integral_constant<bool, std::is_same<V, double>::value && std::is_same<I, int32>::value>{});
    }
    void generate(const Factory*, std::false_type) { GKO_NOT_SUPPORTED("multigrid::Pgm: <double, int32> only"); }
    void generate(const Factory* f, std::true_type)
    {
        ::gko::detail::require_device(exec_, "Pgm::generate");
        auto given = std::dynamic_pointer_cast<const csr_type>(system_matrix_);
        if (!given) {
            auto fbcsr = dynamic_cast<const matrix::Fbcsr<double, int32>*>(system_matrix_.get());
            if (!fbcsr) GKO_NOT_SUPPORTED("Pgm: the system matrix must be a Csr or an Fbcsr");
            auto converted = csr_type::create(exec_);
            fbcsr->convert_to(converted.get());
            given = std::shared_ptr<const csr_type>(std::move(converted));
            this->set_fine_op(given);
        }
        const size_type n = size_[0], nnz = given->get_num_stored_elements();
        std::shared_ptr<csr_type> sorted;
        if (!f->skip_sorting_) {
            // the driver writes the sorted columns and values; the row pointers are the matrix's
            sorted = csr_type::create(exec_, given->get_size(), nnz, given->get_strategy());
            exec_->copy(n + 1, given->get_const_row_ptrs(), sorted->get_row_ptrs());
        }
        array<I> r_row_ptrs(exec_, n + 1), r_col_idxs(exec_, n), c_row_ptrs(exec_, n + 1);
        array<char> ws(exec_, gkomi_pgm_generate_workspace_bytes(n, nnz) + 8);
        int64_t num_agg = 0, coarse_nnz = 0;
        auto call = [&](I* cc, V* cv) {
            return gkomi_pgm_generate_f64_i32(nullptr, n, nnz, given->get_const_row_ptrs(), given->get_const_col_idxs(), given->get_const_values(),
                                              f->max_iterations_, f->max_unassigned_ratio_, f->deterministic_, f->skip_sorting_,
                                              sorted ? sorted->get_col_idxs() : nullptr, sorted ? sorted->get_values() : nullptr, agg_.get_data(),
                                              r_row_ptrs.get_data(), r_col_idxs.get_data(), c_row_ptrs.get_data(), cc, cv, &num_agg, &coarse_nnz, nullptr,
                                              ws.get_data(), ws.get_num_elems());
        };
        GKOMI_CALL(call(nullptr, nullptr));
        const size_type coarse_dim = static_cast<size_type>(num_agg);
        auto strategy = given->get_strategy();
        auto coarse = std::shared_ptr<csr_type>(csr_type::create(exec_, dim<2>(coarse_dim, coarse_dim), static_cast<size_type>(coarse_nnz), strategy));
        exec_->copy(coarse_dim + 1, c_row_ptrs.get_const_data(), coarse->get_row_ptrs());
        if (coarse_nnz > 0) GKOMI_CALL(call(coarse->get_col_idxs(), coarse->get_values()));
        auto restrict_op = std::shared_ptr<csr_type>(csr_type::create(exec_, dim<2>(coarse_dim, n), n, strategy));
        auto prolong_op = std::shared_ptr<csr_type>(csr_type::create(exec_, dim<2>(n, coarse_dim), n, strategy));
        std::vector<V> ones(n, V{1});
        std::vector<I> seq(n + 1);
        for (size_type i = 0; i <= n; ++i) seq[i] = static_cast<I>(i);
        auto host = exec_->get_master();
        exec_->copy(coarse_dim + 1, r_row_ptrs.get_const_data(), restrict_op->get_row_ptrs());
        exec_->copy(n, r_col_idxs.get_const_data(), restrict_op->get_col_idxs());
        exec_->copy_from(host.get(), n, ones.data(), restrict_op->get_values());
        exec_->copy_from(host.get(), n + 1, seq.data(), prolong_op->get_row_ptrs());
        exec_->copy(n, agg_.get_const_data(), prolong_op->get_col_idxs());
        exec_->copy_from(host.get(), n, ones.data(), prolong_op->get_values());
        GKOMI_CALL(gkomi_synchronize(nullptr));  // the workspace goes away with this scope
        if (sorted) this->set_fine_op(sorted);   // pgm.cpp:168
        this->set_multigrid_level(prolong_op, coarse, restrict_op);
    }
    void apply_impl(const LinOp* b, LinOp* x) const override { this->apply_composition(nullptr, b, nullptr, x); }
    void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const override { this->apply_composition(alpha, b, beta, x); }
private:
    std::shared_ptr<const LinOp> system_matrix_;
    array<I> agg_;
};

}  // namespace multigrid

namespace solver {

// build_smoother (include/ginkgo/core/solver/ir.hpp:314-350): Ir with an Iteration criterion and a relaxation factor
template <typename V>
std::shared_ptr<typename Ir<V>::Factory> build_smoother(std::shared_ptr<const LinOpFactory> factory, size_type iteration = 1, V relaxation_factor = 0.9)
{
    auto exec = factory->get_executor();
    return Ir<V>::build().with_solver(factory).with_relaxation_factor(relaxation_factor).with_criteria(stop::Iteration::build().with_max_iters(iteration).on(exec)).on(exec);
}
template <typename V>
std::shared_ptr<typename Ir<V>::Factory> build_smoother(std::shared_ptr<const LinOp> solver, size_type iteration = 1, V relaxation_factor = 0.9)
{
    auto exec = solver->get_executor();
    return Ir<V>::build().with_generated_solver(solver).with_relaxation_factor(relaxation_factor).with_criteria(stop::Iteration::build().with_max_iters(iteration).on(exec)).on(exec);
}

namespace multigrid {
enum class cycle { v, f, w };
enum class mid_smooth_type { both, post_smoother, pre_smoother, standalone };
namespace detail {
using factory_list = std::vector<std::shared_ptr<const LinOpFactory>>;
inline factory_list make_list(const factory_list& v) { return v; }
inline factory_list make_list(factory_list& v) { return v; }
inline factory_list make_list(factory_list&& v) { return std::move(v); }
template <typename... Args>
factory_list make_list(Args&&... args) { return factory_list{std::shared_ptr<const LinOpFactory>(std::forward<Args>(args))...}; }
}  // namespace detail
}  // namespace multigrid

// solver::Multigrid (include/ginkgo/core/solver/multigrid.hpp, core/solver/multigrid.cpp) for double: generate() and
// validate() as :491-574 and :711-748, the cycle as MultigridState::run_cycle :377-485, the outer loop as :646-705 with the
// criterion checked before each cycle, the advanced apply on a clone as :615-643.  The recursion runs on the host and only
// queues work; the one look at the device is the residual norm of a ResidualNorm criterion between two cycles (a smoother
// or coarsest solver the caller supplies does what it does).  A smoother slot whose product does not use an initial guess
// is wrapped by build_smoother; Ir over a scalar Jacobi then runs the fused sweep or the three-call sequence on buffers
// it keeps, without a synchronisation (Ir::apply_with_initial_guess).
class Multigrid : public detail::iterative_solver<Multigrid>, public ApplyWithInitialGuess {
    using base = detail::iterative_solver<Multigrid>;
    using Vec = matrix::Dense<double>;
public:
    using selector = std::function<size_type(const size_type, const LinOp*)>;
    class Factory : public detail::factory_base<Multigrid> {
    public:
        template <typename... A> Factory& with_mg_level(A&&... a) { mg_level = multigrid::detail::make_list(std::forward<A>(a)...); return *this; }
        template <typename... A> Factory& with_pre_smoother(A&&... a) { pre_smoother = multigrid::detail::make_list(std::forward<A>(a)...); return *this; }
        template <typename... A> Factory& with_mid_smoother(A&&... a) { mid_smoother = multigrid::detail::make_list(std::forward<A>(a)...); return *this; }
        template <typename... A> Factory& with_post_smoother(A&&... a) { post_smoother = multigrid::detail::make_list(std::forward<A>(a)...); return *this; }
        template <typename... A> Factory& with_coarsest_solver(A&&... a) { coarsest_solver = multigrid::detail::make_list(std::forward<A>(a)...); return *this; }
        Factory& with_level_selector(selector s) { level_selector = std::move(s); return *this; }
        Factory& with_solver_selector(selector s) { solver_selector = std::move(s); return *this; }
        Factory& with_post_uses_pre(bool v) { post_uses_pre = v; return *this; }
        Factory& with_mid_case(multigrid::mid_smooth_type v) { mid_case = v; return *this; }
        Factory& with_max_levels(size_type v) { max_levels = v; return *this; }
        Factory& with_min_coarse_rows(size_type v) { min_coarse_rows = v; return *this; }
        Factory& with_cycle(multigrid::cycle v) { cycle = v; return *this; }
        Factory& with_smoother_relax(double v) { smoother_relax = v; return *this; }
        Factory& with_smoother_iters(size_type v) { smoother_iters = v; return *this; }
        Factory& with_default_initial_guess(initial_guess_mode v) { default_initial_guess = v; return *this; }
        multigrid::detail::factory_list mg_level, pre_smoother, mid_smoother, post_smoother, coarsest_solver;
        selector level_selector, solver_selector;
        bool post_uses_pre{true};
        multigrid::mid_smooth_type mid_case{multigrid::mid_smooth_type::standalone};
        size_type max_levels{10}, min_coarse_rows{64};
        multigrid::cycle cycle{multigrid::cycle::v};
        double smoother_relax{0.9};
        size_type smoother_iters{1};
        initial_guess_mode default_initial_guess{initial_guess_mode::provided};
    };
    static Factory build() { return Factory{}; }
    const Factory& get_parameters() const noexcept { return parameters_; }
    bool apply_uses_initial_guess() const override { return this->get_default_initial_guess() == initial_guess_mode::provided; }
    const std::vector<std::shared_ptr<const ::gko::multigrid::MultigridLevel>>& get_mg_level_list() const { return mg_level_list_; }
    const std::vector<std::shared_ptr<const LinOp>>& get_pre_smoother_list() const { return pre_smoother_list_; }
    const std::vector<std::shared_ptr<const LinOp>>& get_mid_smoother_list() const { return mid_smoother_list_; }
    const std::vector<std::shared_ptr<const LinOp>>& get_post_smoother_list() const { return post_smoother_list_; }
    std::shared_ptr<const LinOp> get_coarsest_solver() const { return coarsest_solver_; }
    multigrid::cycle get_cycle() const noexcept { return cycle_; }
    void set_cycle(multigrid::cycle c) { cycle_ = c; }
    void apply_with_initial_guess(const LinOp* b, LinOp* x, initial_guess_mode guess) const override
    {
        this->validate(b, x);
        prepare_initial_guess(b, x, guess);
        this->run(matrix::detail_fmt::dense(b), matrix::detail_fmt::dense(x), guess);
    }
    void apply_with_initial_guess(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x, initial_guess_mode guess) const
    {
        this->validate(b, x);
        prepare_initial_guess(b, x, guess);
        auto dx = matrix::detail_fmt::dense(x);
        auto x_clone = dx->clone();
        this->run(matrix::detail_fmt::dense(b), x_clone.get(), guess);
        dx->scale(matrix::detail_fmt::dense(beta));
        dx->add_scaled(matrix::detail_fmt::dense(alpha), x_clone.get());
    }
protected:
    friend class detail::factory_base<Multigrid>;
    Multigrid(const Factory* f, std::shared_ptr<const LinOp> A) : base(f, std::move(A)), parameters_(*f), cycle_(f->cycle)
    {
        this->validate_parameters();
        level_selector_ = parameters_.level_selector ? parameters_.level_selector
                          : parameters_.mg_level.size() == 1 ? selector([](const size_type, const LinOp*) { return size_type{0}; })
                                                             : selector([](const size_type level, const LinOp*) { return level; });
        solver_selector_ = parameters_.solver_selector ? parameters_.solver_selector : selector([](const size_type, const LinOp*) { return size_type{0}; });
        this->set_default_initial_guess(parameters_.default_initial_guess);
        if (this->size_[0] != 0) this->generate();
    }
    static void verify_legal_length(bool checked, size_type len, size_type ref_len)
    {
        if (checked && len > 1 && len != ref_len) GKO_NOT_SUPPORTED("Multigrid: a smoother list has 0, 1 or as many entries as mg_level");
    }
    void validate_parameters() const
    {
        const auto len = parameters_.mg_level.size();
        if (len == 0) GKO_NOT_SUPPORTED("Multigrid: mg_level is empty");
        for (const auto& f : parameters_.mg_level) {
            if (f == nullptr) GKO_NOT_SUPPORTED("Multigrid: an mg_level entry is null");
        }
        verify_legal_length(true, parameters_.pre_smoother.size(), len);
        verify_legal_length(!parameters_.post_uses_pre, parameters_.post_smoother.size(), len);
        verify_legal_length(parameters_.mid_case == multigrid::mid_smooth_type::standalone, parameters_.mid_smoother.size(), len);
    }
    void handle_list(size_type index, std::shared_ptr<const LinOp> matrix, const multigrid::detail::factory_list& list,
                     std::vector<std::shared_ptr<const LinOp>>& out) const
    {
        if (list.empty()) {
            out.emplace_back(nullptr);
            return;
        }
        const auto at = list.size() == 1 ? size_type{0} : index;
        if (at >= list.size()) GKO_NOT_SUPPORTED("Multigrid: a selector's index is out of the list's bounds");
        const auto& item = list[at];
        if (item == nullptr) {
            out.emplace_back(nullptr);
            return;
        }
        std::shared_ptr<const LinOp> solver(item->generate_impl(matrix));
        if (solver->apply_uses_initial_guess()) {
            out.emplace_back(std::move(solver));
        } else {
            out.emplace_back(build_smoother<double>(solver, parameters_.smoother_iters, parameters_.smoother_relax)->generate(matrix));
        }
    }
    void generate()
    {
        auto num_rows = this->size_[0];
        size_type level = 0;
        std::shared_ptr<const LinOp> matrix = this->A_;
        while (level < parameters_.max_levels && num_rows > parameters_.min_coarse_rows) {
            const auto index = level_selector_(level, matrix.get());
            if (index >= parameters_.mg_level.size()) GKO_NOT_SUPPORTED("Multigrid: a selector's index is out of the list's bounds");
            std::shared_ptr<const LinOp> product(parameters_.mg_level[index]->generate_impl(matrix));
            auto mg_level = std::dynamic_pointer_cast<const ::gko::multigrid::MultigridLevel>(product);
            if (!mg_level) GKO_NOT_SUPPORTED("Multigrid: an mg_level factory must generate a MultigridLevel");
            if (mg_level->get_coarse_op()->get_size()[0] == num_rows) break;   // does not reduce the dimension
            handle_list(index, mg_level->get_fine_op(), parameters_.pre_smoother, pre_smoother_list_);
            if (parameters_.mid_case == multigrid::mid_smooth_type::standalone) {
                handle_list(index, mg_level->get_fine_op(), parameters_.mid_smoother, mid_smoother_list_);
            }
            if (!parameters_.post_uses_pre) handle_list(index, mg_level->get_fine_op(), parameters_.post_smoother, post_smoother_list_);
            mg_level_list_.emplace_back(mg_level);
            level_owners_.emplace_back(std::move(product));
            matrix = mg_level->get_coarse_op();
            num_rows = matrix->get_size()[0];
            ++level;
        }
        if (parameters_.post_uses_pre) post_smoother_list_ = pre_smoother_list_;
        if (level == 0) GKO_NOT_SUPPORTED("Multigrid: no level was generated");
        std::shared_ptr<const LinOpFactory> coarsest;
        if (!parameters_.coarsest_solver.empty()) {
            const auto at = solver_selector_(level, matrix.get());
            if (at >= parameters_.coarsest_solver.size()) GKO_NOT_SUPPORTED("Multigrid: a selector's index is out of the list's bounds");
            coarsest = parameters_.coarsest_solver[at];
        }
        coarsest_solver_ = coarsest ? std::shared_ptr<const LinOp>(coarsest->generate_impl(matrix))
                                    : std::shared_ptr<const LinOp>(matrix::Identity<double>::create(this->exec_, matrix->get_size()[0]));
    }
    // MultigridState::generate: r of every level's rows, g and e of the next level's, once per number of columns
    void allocate(size_type nrhs) const
    {
        if (state_nrhs_ == nrhs) return;
        r_.clear(), g_.clear(), e_.clear();
        for (const auto& lvl : mg_level_list_) {
            r_.emplace_back(Vec::create(this->exec_, dim<2>(lvl->get_fine_op()->get_size()[0], nrhs)));
            g_.emplace_back(Vec::create(this->exec_, dim<2>(lvl->get_coarse_op()->get_size()[0], nrhs)));
            e_.emplace_back(Vec::create(this->exec_, dim<2>(lvl->get_coarse_op()->get_size()[0], nrhs)));
        }
        one_ = initialize<Vec>({1.0}, this->exec_);
        neg_one_ = initialize<Vec>({-1.0}, this->exec_);
        state_nrhs_ = nrhs;
    }
    void smooth(const LinOp* smoother, const LinOp* b, LinOp* x, bool x_is_zero, size_type level) const
    {
        if (auto with_guess = dynamic_cast<const ApplyWithInitialGuess*>(smoother)) {
            with_guess->apply_with_initial_guess(b, x, x_is_zero ? initial_guess_mode::zero : with_guess->get_default_initial_guess());
            return;
        }
        // x of the first level is zero already (multigrid.cpp:413-419)
        if (x_is_zero && level != 0) matrix::detail_fmt::dense(x)->fill(0.0);
        smoother->apply(b, x);
    }
    void run_cycle(multigrid::cycle cycle, size_type level, const LinOp* matrix, const LinOp* b, LinOp* x, bool x_is_zero, bool first, bool end) const
    {
        using multigrid::mid_smooth_type;
        const auto total = mg_level_list_.size();
        if (level == total) {
            coarsest_solver_->apply(b, x);
            return;
        }
        const auto& lvl = mg_level_list_[level];
        const auto mid_case = parameters_.mid_case;
        const LinOp* pre = pre_smoother_list_[level].get();
        const LinOp* post = post_smoother_list_[level].get();
        const LinOp* mid = mid_case == mid_smooth_type::standalone ? mid_smoother_list_[level].get() : nullptr;
        if ((first || mid_case == mid_smooth_type::both || mid_case == mid_smooth_type::pre_smoother) && pre) smooth(pre, b, x, x_is_zero, level);
        auto r = r_[level].get(), g = g_[level].get(), e = e_[level].get();
        r->copy_from(matrix::detail_fmt::dense(b));
        matrix->apply(neg_one_.get(), x, one_.get(), r);
        lvl->get_restrict_op()->apply(r, g);
        if (level + 1 == total) e->fill(0.0);
        const LinOp* next = level + 1 < total ? mg_level_list_[level + 1]->get_fine_op().get() : lvl->get_coarse_op().get();
        run_cycle(cycle, level + 1, next, g, e, true, true, cycle == multigrid::cycle::v);
        if (level + 1 < total) {
            if (cycle == multigrid::cycle::f) {
                run_cycle(multigrid::cycle::v, level + 1, next, g, e, false, false, true);
            } else if (cycle == multigrid::cycle::w) {
                run_cycle(cycle, level + 1, next, g, e, false, false, true);
            }
        }
        lvl->get_prolong_op()->apply(one_.get(), e, one_.get(), x);
        if ((end || mid_case == mid_smooth_type::both || mid_case == mid_smooth_type::post_smoother) && post) smooth(post, b, x, false, level);
        if ((cycle == multigrid::cycle::w || cycle == multigrid::cycle::f) && !end && mid_case == mid_smooth_type::standalone && mid) {
            smooth(mid, b, x, false, level);
        }
    }
    std::vector<double> host_norm2(const Vec* v) const
    {
        auto norm = Vec::create(this->exec_, dim<2>(1, v->get_size()[1]));
        v->compute_norm2(norm.get());
        std::vector<double> out(v->get_size()[1]);
        this->exec_->get_master()->copy_from(this->exec_.get(), out.size(), norm->get_const_values(), out.data());
        return out;
    }
    // apply_dense_impl (:646-705): Iteration and ResidualNorm, both asked before each cycle
    void run(const Vec* b, Vec* x, initial_guess_mode guess) const
    {
        ::gko::detail::require_device(this->exec_, "multigrid::apply");
        const auto& st = this->settings_;
        if (st.implicit) GKO_NOT_SUPPORTED("Multigrid: ImplicitResidualNorm");
        allocate(b->get_size()[1]);
        std::vector<double> base_norm;
        int64_t iter = 0;
        bool converged = false;
        while (true) {
            if (iter >= st.max_iters) break;
            if (st.reduction_factor > 0.0) {
                auto r = r_[0].get();
                r->copy_from(b);
                this->A_->apply(neg_one_.get(), x, one_.get(), r);
                const auto res = host_norm2(r);
                if (base_norm.empty()) {
                    base_norm = st.baseline == stop::mode::rhs_norm ? host_norm2(b) : st.baseline == stop::mode::initial_resnorm ? res : std::vector<double>(res.size(), 1.0);
                }
                converged = true;
                for (size_type j = 0; j < res.size(); ++j) converged = converged && res[j] <= st.reduction_factor * base_norm[j];
                if (converged) break;
            }
            run_cycle(cycle_, 0, this->A_.get(), b, x, iter == 0 && guess == initial_guess_mode::zero, true, true);
            ++iter;
        }
        this->last_iters_ = iter;
        this->last_converged_ = converged;
    }
    using base::apply_impl;
    void apply_impl(const LinOp* b, LinOp* x) const override { this->apply_with_initial_guess(b, x, this->get_default_initial_guess()); }
    void apply_impl(const LinOp* alpha, const LinOp* b, const LinOp* beta, LinOp* x) const override
    {
        this->apply_with_initial_guess(alpha, b, beta, x, this->get_default_initial_guess());
    }
private:
    Factory parameters_;
    multigrid::cycle cycle_;
    selector level_selector_, solver_selector_;
    std::vector<std::shared_ptr<const ::gko::multigrid::MultigridLevel>> mg_level_list_;
    std::vector<std::shared_ptr<const LinOp>> level_owners_;
    std::vector<std::shared_ptr<const LinOp>> pre_smoother_list_, mid_smoother_list_, post_smoother_list_;
    std::shared_ptr<const LinOp> coarsest_solver_;
    mutable std::vector<std::unique_ptr<Vec>> r_, g_, e_;
    mutable std::unique_ptr<Vec> one_, neg_one_;
    mutable size_type state_nrhs_{0};
};

}  // namespace solver

}  // namespace gko

#include "distributed.hpp"

#endif  // GKOMI_GINKGO_HPP_
