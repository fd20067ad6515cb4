// hip/solver/cb_gmres_kernels.hip.cpp: cb_gmres::{initialize, restart, arnoldi, solve_krylov}
// (core/solver/cb_gmres_kernels.hpp:128-169) for the six <double, storage> accessor instantiations of
// GKO_INSTANTIATE_FOR_EACH_CB_GMRES_TYPE (:65-86): reduced_row_major over double, float and half,
// scaled_reduced_row_major<.., 0b101> over int64, int32 and int16.  The float and complex value types are not bound.
// The accessor hands over its two pointers; its strides must be the packed ones of Range3dHelper
// (core/solver/cb_gmres_accessor.hpp), entry (k, row, col) at (k n + row) nrhs + col and scalar (k, col) at k nrhs + col.
// The Dense arguments are the contiguous workspace matrices of CbGmres::apply_dense_impl (core/solver/cb_gmres.cpp:229-261);
// hessenberg_iter is a column block of hessenberg and keeps its stride.  A padded operand is refused rather than misread.
// reorth_status and num_reorth are scratch of the reference's device kernels (cb_gmres.cpp:266-272) and stay untouched:
// the re-orthogonalisation loop is decided on the device.  arnoldi has no reduction_tmp in its interface and allocates
// its partial-sum workspace per call.
#include "../gkomi_bindings.hpp"
#include <type_traits>

namespace gko {
namespace kernels {
namespace hip {
namespace cb_gmres {
namespace {
inline void contiguous(const matrix::Dense<double>* m, const char* what)
{
    if (m->get_stride() != m->get_size()[1]) GKO_NOT_SUPPORTED(what);
}
inline uint8_t* raw(stopping_status* s) { return reinterpret_cast<uint8_t*>(s); }
inline const uint8_t* raw(const stopping_status* s) { return reinterpret_cast<const uint8_t*>(s); }
static_assert(sizeof(size_type) == sizeof(uint64_t), "final_iter_nums are 64-bit");

// the `storage` code of gkomi_cb_gmres_* (the order of solver::cb_gmres::storage_precision)
template <typename S> struct storage_code;
template <> struct storage_code<double> { static constexpr int value = 0; };
template <> struct storage_code<float> { static constexpr int value = 1; };
template <> struct storage_code<half> { static constexpr int value = 2; };
template <> struct storage_code<int64> { static constexpr int value = 3; };
template <> struct storage_code<int32> { static constexpr int value = 4; };
template <> struct storage_code<int16> { static constexpr int value = 5; };
static_assert(sizeof(half) == 2 && sizeof(int16) == 2, "16-bit storages");

struct basis_view {
    int storage;
    int64_t krylov_dim, n, nrhs;
    void* data;
    double* scalars;
};

inline void packed(bool ok)
{
    if (!ok) GKO_NOT_SUPPORTED("cb_gmres: a krylov basis whose strides are not the packed ones");
}

template <typename S>
basis_view view_of(const acc::reduced_row_major<3, double, S>& a)
{
    const auto size = a.get_size();
    packed(a.get_stride()[0] == size[1] * size[2] && a.get_stride()[1] == size[2]);
    using plain = typename std::remove_const<S>::type;
    return {storage_code<plain>::value, static_cast<int64_t>(size[0]) - 1, static_cast<int64_t>(size[1]), static_cast<int64_t>(size[2]),
            const_cast<plain*>(a.get_const_storage()), nullptr};
}

template <typename S>
basis_view view_of(const acc::scaled_reduced_row_major<3, double, S, 0b101>& a)
{
    const auto size = a.get_size();
    packed(a.get_storage_stride()[0] == size[1] * size[2] && a.get_storage_stride()[1] == size[2] && a.get_scalar_stride()[0] == size[2]);
    using plain = typename std::remove_const<S>::type;
    return {storage_code<plain>::value, static_cast<int64_t>(size[0]) - 1, static_cast<int64_t>(size[1]), static_cast<int64_t>(size[2]),
            const_cast<plain*>(a.get_const_storage()), const_cast<double*>(a.get_const_scalar())};
}
}  // namespace

template <typename ValueType>
void initialize(std::shared_ptr<const HipExecutor> exec, const matrix::Dense<ValueType>* b, matrix::Dense<ValueType>* residual,
                matrix::Dense<ValueType>* givens_sin, matrix::Dense<ValueType>* givens_cos, array<stopping_status>* stop_status,
                size_type krylov_dim)
{
    contiguous(givens_sin, "cb_gmres::initialize: padded givens_sin");
    contiguous(givens_cos, "cb_gmres::initialize: padded givens_cos");
    GKOMI_CALL(gkomi_cb_gmres_initialize_f64(GKOMI_NULL_STREAM, b->get_size()[0], b->get_size()[1], static_cast<int64_t>(krylov_dim),
                                             b->get_const_values(), b->get_stride(), residual->get_values(), residual->get_stride(),
                                             givens_sin->get_values(), givens_cos->get_values(), raw(stop_status->get_data())));
}

template void initialize<double>(std::shared_ptr<const HipExecutor>, const matrix::Dense<double>*, matrix::Dense<double>*,
                                 matrix::Dense<double>*, matrix::Dense<double>*, array<stopping_status>*, size_type);

template <typename ValueType, typename Accessor3d>
void restart(std::shared_ptr<const HipExecutor> exec, const matrix::Dense<ValueType>* residual,
             matrix::Dense<remove_complex<ValueType>>* residual_norm, matrix::Dense<ValueType>* residual_norm_collection,
             matrix::Dense<remove_complex<ValueType>>* arnoldi_norm, Accessor3d krylov_bases, matrix::Dense<ValueType>* next_krylov_basis,
             array<size_type>* final_iter_nums, array<char>& reduction_tmp, size_type krylov_dim)
{
    const basis_view v = view_of(krylov_bases.get_accessor());
    if (v.krylov_dim != static_cast<int64_t>(krylov_dim) || v.n != static_cast<int64_t>(residual->get_size()[0]) ||
        v.nrhs != static_cast<int64_t>(residual->get_size()[1])) {
        GKO_NOT_SUPPORTED("cb_gmres::restart: a krylov basis that is not (krylov_dim + 1) x rows x columns");
    }
    contiguous(residual, "cb_gmres::restart: padded residual");
    contiguous(residual_norm_collection, "cb_gmres::restart: padded residual_norm_collection");
    contiguous(arnoldi_norm, "cb_gmres::restart: padded arnoldi_norm");
    contiguous(next_krylov_basis, "cb_gmres::restart: padded next_krylov_basis");
    const size_type need = gkomi_cb_gmres_step_workspace_bytes(v.nrhs, v.krylov_dim);
    if (reduction_tmp.get_num_elems() < need) reduction_tmp.resize_and_reset(need);
    GKOMI_CALL(gkomi_cb_gmres_restart_f64(GKOMI_NULL_STREAM, v.n, v.nrhs, v.krylov_dim, v.storage, residual->get_const_values(),
                                          residual_norm->get_values(), residual_norm_collection->get_values(), arnoldi_norm->get_values(),
                                          v.data, v.scalars, next_krylov_basis->get_values(),
                                          reinterpret_cast<uint64_t*>(final_iter_nums->get_data()), 1, reduction_tmp.get_data(),
                                          reduction_tmp.get_num_elems()));
}

template <typename ValueType, typename Accessor3d>
void arnoldi(std::shared_ptr<const HipExecutor> exec, matrix::Dense<ValueType>* next_krylov_basis, matrix::Dense<ValueType>* givens_sin,
             matrix::Dense<ValueType>* givens_cos, matrix::Dense<remove_complex<ValueType>>* residual_norm,
             matrix::Dense<ValueType>* residual_norm_collection, Accessor3d krylov_bases, matrix::Dense<ValueType>* hessenberg_iter,
             matrix::Dense<ValueType>* buffer_iter, matrix::Dense<remove_complex<ValueType>>* arnoldi_norm, size_type iter,
             array<size_type>* final_iter_nums, const array<stopping_status>* stop_status, array<stopping_status>* reorth_status,
             array<size_type>* num_reorth)
{
    const basis_view v = view_of(krylov_bases.get_accessor());
    if (v.n != static_cast<int64_t>(next_krylov_basis->get_size()[0]) || v.nrhs != static_cast<int64_t>(next_krylov_basis->get_size()[1])) {
        GKO_NOT_SUPPORTED("cb_gmres::arnoldi: a krylov basis that does not match next_krylov_basis");
    }
    contiguous(next_krylov_basis, "cb_gmres::arnoldi: padded next_krylov_basis");
    contiguous(givens_sin, "cb_gmres::arnoldi: padded givens_sin");
    contiguous(givens_cos, "cb_gmres::arnoldi: padded givens_cos");
    contiguous(residual_norm_collection, "cb_gmres::arnoldi: padded residual_norm_collection");
    contiguous(buffer_iter, "cb_gmres::arnoldi: padded buffer_iter");
    contiguous(arnoldi_norm, "cb_gmres::arnoldi: padded arnoldi_norm");
    array<char> ws(exec, gkomi_cb_gmres_step_workspace_bytes(v.nrhs, v.krylov_dim));
    GKOMI_CALL(gkomi_cb_gmres_arnoldi_f64(GKOMI_NULL_STREAM, v.n, v.nrhs, v.krylov_dim, v.storage, next_krylov_basis->get_values(),
                                          givens_sin->get_values(), givens_cos->get_values(), residual_norm->get_values(),
                                          residual_norm_collection->get_values(), v.data, v.scalars, hessenberg_iter->get_values(),
                                          hessenberg_iter->get_stride(), buffer_iter->get_values(), arnoldi_norm->get_values(),
                                          static_cast<int64_t>(iter), reinterpret_cast<uint64_t*>(final_iter_nums->get_data()),
                                          raw(stop_status->get_const_data()), nullptr, ws.get_data(), ws.get_num_elems()));
    exec->synchronize();  // ws is released on return
}

template <typename ValueType, typename ConstAccessor3d>
void solve_krylov(std::shared_ptr<const HipExecutor> exec, const matrix::Dense<ValueType>* residual_norm_collection,
                  ConstAccessor3d krylov_bases, const matrix::Dense<ValueType>* hessenberg, matrix::Dense<ValueType>* y,
                  matrix::Dense<ValueType>* before_preconditioner, const array<size_type>* final_iter_nums)
{
    const basis_view v = view_of(krylov_bases.get_accessor());
    if (v.n != static_cast<int64_t>(before_preconditioner->get_size()[0]) ||
        v.nrhs != static_cast<int64_t>(before_preconditioner->get_size()[1])) {
        GKO_NOT_SUPPORTED("cb_gmres::solve_krylov: a krylov basis that does not match before_preconditioner");
    }
    contiguous(residual_norm_collection, "cb_gmres::solve_krylov: padded residual_norm_collection");
    contiguous(y, "cb_gmres::solve_krylov: padded y");
    contiguous(before_preconditioner, "cb_gmres::solve_krylov: padded before_preconditioner");
    GKOMI_CALL(gkomi_cb_gmres_solve_krylov_f64(GKOMI_NULL_STREAM, v.n, v.nrhs, v.storage, residual_norm_collection->get_const_values(), v.data,
                                               v.scalars, hessenberg->get_const_values(), hessenberg->get_stride(), y->get_values(),
                                               before_preconditioner->get_values(),
                                               reinterpret_cast<const uint64_t*>(final_iter_nums->get_const_data())));
}

#define GKOMI_CB_RESTART(_range)                                                                                                   \
    template void restart<double, _range>(std::shared_ptr<const HipExecutor>, const matrix::Dense<double>*, matrix::Dense<double>*, \
                                          matrix::Dense<double>*, matrix::Dense<double>*, _range, matrix::Dense<double>*,           \
                                          array<size_type>*, array<char>&, size_type)
#define GKOMI_CB_ARNOLDI(_range)                                                                                                      \
    template void arnoldi<double, _range>(std::shared_ptr<const HipExecutor>, matrix::Dense<double>*, matrix::Dense<double>*,          \
                                          matrix::Dense<double>*, matrix::Dense<double>*, matrix::Dense<double>*, _range,              \
                                          matrix::Dense<double>*, matrix::Dense<double>*, matrix::Dense<double>*, size_type,           \
                                          array<size_type>*, const array<stopping_status>*, array<stopping_status>*, array<size_type>*)
#define GKOMI_CB_SOLVE_KRYLOV(_range)                                                                                             \
    template void solve_krylov<double, _range>(std::shared_ptr<const HipExecutor>, const matrix::Dense<double>*, _range,          \
                                               const matrix::Dense<double>*, matrix::Dense<double>*, matrix::Dense<double>*,      \
                                               const array<size_type>*)
#define GKOMI_CB_REDUCED(_storage) acc::range<acc::reduced_row_major<3, double, _storage>>
#define GKOMI_CB_SCALED(_storage) acc::range<acc::scaled_reduced_row_major<3, double, _storage, 0b101>>
#define GKOMI_CB_EACH_STORAGE(_macro, _const)       \
    _macro(GKOMI_CB_REDUCED(_const double));        \
    _macro(GKOMI_CB_REDUCED(_const float));         \
    _macro(GKOMI_CB_REDUCED(_const half));          \
    _macro(GKOMI_CB_SCALED(_const int64));          \
    _macro(GKOMI_CB_SCALED(_const int32));          \
    _macro(GKOMI_CB_SCALED(_const int16))

GKOMI_CB_EACH_STORAGE(GKOMI_CB_RESTART, );
GKOMI_CB_EACH_STORAGE(GKOMI_CB_ARNOLDI, );
GKOMI_CB_EACH_STORAGE(GKOMI_CB_SOLVE_KRYLOV, const);

}  // namespace cb_gmres
}  // namespace hip
}  // namespace kernels
}  // namespace gko
