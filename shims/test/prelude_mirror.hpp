// Compile-test environment of the shims (tests/test_cpp_mirror.py): the host mirror provides the
// class and accessor names the reference's headers provide in a real tree, plus the few types of
// the reference's kernel interfaces that the mirror's public API does not need.
#pragma once
#include <ginkgo/ginkgo.hpp>
#define GKOMI_SROW_IS_OURS true  // the mirror's Csr::make_srow is gkomi_csr_make_srow_i32

namespace gko {
// include/ginkgo/core/stop/stopping_status.hpp: one byte
class stopping_status {
public:
    uint8 data_{0};
};
namespace matrix {
// include/ginkgo/core/matrix/diagonal.hpp, as far as the extract_diagonal kernels use it: n values
template <typename V = double>
class Diagonal {
public:
    static std::unique_ptr<Diagonal> create(std::shared_ptr<const Executor> exec, size_type n) { return std::unique_ptr<Diagonal>(new Diagonal(std::move(exec), n)); }
    dim<2> get_size() const noexcept { return dim<2>(values_.get_num_elems(), values_.get_num_elems()); }
    V* get_values() noexcept { return values_.get_data(); }
    const V* get_const_values() const noexcept { return values_.get_const_data(); }
    std::shared_ptr<const Executor> get_executor() const noexcept { return values_.get_executor(); }
private:
    Diagonal(std::shared_ptr<const Executor> exec, size_type n) : values_(std::move(exec), n) {}
    array<V> values_;
};
}  // namespace matrix
namespace kernels {
namespace hip {
// the mirror's Csr keeps the statistic itself (gkomi_bindings.hpp has the reference-tree version)
inline int64_t gkomi_row_hint(const matrix::Csr<double, int32>* a) { return a->get_max_row_nnz(); }
}  // namespace hip
}  // namespace kernels
namespace solver {
struct SolveStruct {
    virtual ~SolveStruct() = default;
};
enum class trisolve_algorithm { sparselib, syncfree };
}  // namespace solver
}  // namespace gko
