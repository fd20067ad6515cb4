// Compile-test environment of shims/hip/solver/cb_gmres_kernels.hip.cpp on top of prelude_mirror.hpp: the names of the
// reference's accessor/ directory that the CB-GMRES kernel interface is written in (accessor/range.hpp,
// reduced_row_major.hpp, scaled_reduced_row_major.hpp; core/base/extended_float.hpp for half), as far as the shim
// uses them -- sizes, strides and the two pointers.  No element access: the host mirror never reads a compressed
// basis, and in a reference tree the shim sees the reference's own headers, not these.
#pragma once
#include "prelude_mirror.hpp"
#include <array>

namespace gko {
using int16 = std::int16_t;
struct half {
    std::uint16_t data_;
};
static_assert(sizeof(half) == 2, "half is 16 bits of storage");

namespace acc {
template <typename Accessor>
class range {
public:
    using accessor = Accessor;
    template <typename... Args>
    explicit range(Args&&... args) : accessor_(std::forward<Args>(args)...) {}
    size_type length(size_type dimension) const { return accessor_.length(dimension); }
    const accessor* operator->() const noexcept { return &accessor_; }
    const accessor& get_accessor() const noexcept { return accessor_; }
private:
    accessor accessor_;
};

// entry (k, row, col) at k stride[0] + row stride[1] + col
template <std::size_t Dimensionality, typename ArithmeticType, typename StorageType>
class reduced_row_major {
public:
    static_assert(Dimensionality == 3, "only the 3-d basis is mirrored");
    using arithmetic_type = typename std::remove_cv<ArithmeticType>::type;
    using storage_type = StorageType;
    using dim_type = std::array<size_type, 3>;
    using storage_stride_type = std::array<size_type, 2>;
    reduced_row_major(dim_type size, storage_type* storage) : reduced_row_major(size, storage, {{size[1] * size[2], size[2]}}) {}
    reduced_row_major(dim_type size, storage_type* storage, storage_stride_type stride) : size_(size), storage_(storage), stride_(stride) {}
    size_type length(size_type dimension) const { return dimension < 3 ? size_[dimension] : 1; }
    dim_type get_size() const { return size_; }
    const storage_stride_type& get_stride() const { return stride_; }
    storage_type* get_stored_data() const { return storage_; }
    const storage_type* get_const_storage() const { return storage_; }
private:
    dim_type size_;
    storage_type* storage_;
    storage_stride_type stride_;
};

// the same with one arithmetic scalar per (k, col) for ScalarMask 0b101, at k scalar_stride[0] + col
template <std::size_t Dimensionality, typename ArithmeticType, typename StorageType, std::uint64_t ScalarMask>
class scaled_reduced_row_major {
public:
    static_assert(Dimensionality == 3 && ScalarMask == 0b101, "only the 3-d basis with a scalar per vector and column is mirrored");
    using arithmetic_type = typename std::remove_cv<ArithmeticType>::type;
    using storage_type = StorageType;
    using scalar_type = typename std::conditional<std::is_const<StorageType>::value, const arithmetic_type, arithmetic_type>::type;
    using dim_type = std::array<size_type, 3>;
    using storage_stride_type = std::array<size_type, 2>;
    using scalar_stride_type = std::array<size_type, 1>;
    scaled_reduced_row_major(dim_type size, storage_type* storage, scalar_type* scalar)
        : scaled_reduced_row_major(size, storage, {{size[1] * size[2], size[2]}}, scalar, {{size[2]}}) {}
    scaled_reduced_row_major(dim_type size, storage_type* storage, storage_stride_type storage_stride, scalar_type* scalar, scalar_stride_type scalar_stride)
        : size_(size), storage_(storage), storage_stride_(storage_stride), scalar_(scalar), scalar_stride_(scalar_stride) {}
    size_type length(size_type dimension) const { return dimension < 3 ? size_[dimension] : 1; }
    dim_type get_size() const { return size_; }
    const storage_stride_type& get_storage_stride() const { return storage_stride_; }
    const scalar_stride_type& get_scalar_stride() const { return scalar_stride_; }
    storage_type* get_stored_data() const { return storage_; }
    const storage_type* get_const_storage() const { return storage_; }
    scalar_type* get_scalar() const { return scalar_; }
    const scalar_type* get_const_scalar() const { return scalar_; }
private:
    dim_type size_;
    storage_type* storage_;
    storage_stride_type storage_stride_;
    scalar_type* scalar_;
    scalar_stride_type scalar_stride_;
};
}  // namespace acc
}  // namespace gko
