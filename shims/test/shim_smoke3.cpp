// Runs the IDR shims (shims/hip/solver/idr_kernels.hip.cpp) on the device, each against a closed-form answer on a
// 3000-row problem with s = 2 and one right-hand side.  Prints one "ran idr::<kernel> ok|WRONG" line per kernel like
// shim_smoke2.cpp and returns the number of wrong ones.
#include "prelude_mirror.hpp"
#include <cmath>
#include <cstdio>
#include <vector>

namespace gko { namespace kernels { namespace hip {
using Vec = matrix::Dense<double>;
using Status = array<stopping_status>;
namespace idr {
void initialize(std::shared_ptr<const HipExecutor>, const size_type, Vec*, Vec*, bool, Status*);
void step_1(std::shared_ptr<const HipExecutor>, const size_type, const size_type, const Vec*, const Vec*, const Vec*, const Vec*, Vec*, Vec*, const Status*);
void step_2(std::shared_ptr<const HipExecutor>, const size_type, const size_type, const Vec*, const Vec*, const Vec*, Vec*, const Status*);
void step_3(std::shared_ptr<const HipExecutor>, const size_type, const size_type, const Vec*, Vec*, Vec*, Vec*, Vec*, Vec*, Vec*, Vec*, Vec*, const Status*);
void compute_omega(std::shared_ptr<const HipExecutor>, const size_type, const double, const Vec*, const Vec*, Vec*, const Status*);
}
}}}

using namespace gko;
namespace k = gko::kernels::hip;
using Vec = matrix::Dense<double>;

static int wrong = 0;
static void ran(const char* name, bool ok)
{
    std::printf("ran %s %s\n", name, ok ? "ok" : "WRONG");
    if (!ok) ++wrong;
}
static std::vector<double> host_of(const Vec* v)
{
    auto h = v->clone(v->get_executor()->get_master());
    std::vector<double> out(v->get_size()[0] * v->get_size()[1]);
    for (size_type i = 0; i < v->get_size()[0]; ++i)
        for (size_type j = 0; j < v->get_size()[1]; ++j) out[i * v->get_size()[1] + j] = h->at(i, j);
    return out;
}
// every entry of column `col` equals `value`
static bool column_equal(const Vec* v, size_type col, double value, double tol = 0.0)
{
    const auto h = host_of(v);
    const size_type cols = v->get_size()[1];
    for (size_type i = 0; i < v->get_size()[0]; ++i) if (!(std::abs(h[i * cols + col] - value) <= tol)) return false;
    return true;
}
static std::unique_ptr<Vec> filled(std::shared_ptr<const Executor> exec, size_type rows, size_type cols, double value)
{
    auto v = Vec::create(exec, dim<2>(rows, cols));
    v->fill(value);
    return v;
}
// rows x cols with column j filled with values[j]
static std::unique_ptr<Vec> columns(std::shared_ptr<const Executor> exec, size_type rows, std::vector<double> values)
{
    auto h = Vec::create(exec->get_master(), dim<2>(rows, values.size()));
    for (size_type i = 0; i < rows; ++i)
        for (size_type j = 0; j < values.size(); ++j) h->at(i, j) = values[j];
    return h->clone(exec);
}

int main()
{
    auto hip = HipExecutor::create(0, ReferenceExecutor::create());
    const size_type n = 3000, s = 2, nrhs = 1;
    array<stopping_status> status(hip, nrhs);
    // initialize: rows (1 .. 1) and (1 .. 1, -1 .. -1) are orthogonal already; m = I, P = rows / sqrt(n)
    {
        auto m = filled(hip, s, s * nrhs, 9.0);
        auto ph = Vec::create(hip->get_master(), dim<2>(s, n));
        for (size_type j = 0; j < n; ++j) {
            ph->at(0, j) = 1.0;
            ph->at(1, j) = j < n / 2 ? 1.0 : -1.0;
        }
        auto p = ph->clone(hip);
        k::idr::initialize(hip, nrhs, m.get(), p.get(), true, &status);
        const auto mh = host_of(m.get()), pp = host_of(p.get());
        bool ok = mh[0] == 1.0 && mh[1] == 0.0 && mh[2] == 0.0 && mh[3] == 1.0;
        const double inv = 1.0 / std::sqrt(double(n));
        for (size_type j = 0; j < n; ++j) ok = ok && std::abs(pp[j] - inv) < 1e-14 && std::abs(pp[n + j] - (j < n / 2 ? inv : -inv)) < 1e-14;
        // without `deterministic` the shim draws the rows itself: orthonormal afterwards
        auto q = filled(hip, s, n, 0.0);
        k::idr::initialize(hip, nrhs, m.get(), q.get(), false, &status);
        const auto qq = host_of(q.get());
        double d00 = 0.0, d01 = 0.0, d11 = 0.0;
        for (size_type j = 0; j < n; ++j) { d00 += qq[j] * qq[j]; d01 += qq[j] * qq[n + j]; d11 += qq[n + j] * qq[n + j]; }
        ran("idr::initialize", ok && std::abs(d00 - 1.0) < 1e-12 && std::abs(d11 - 1.0) < 1e-12 && std::abs(d01) < 1e-12);
    }
    // m = (2 0; 1 4), f = (2, 5): c = (1, 1)
    auto m = initialize<Vec>({{2.0, 0.0}, {1.0, 4.0}}, hip);
    auto f = initialize<Vec>({2.0, 5.0}, hip);
    auto c = filled(hip, s, nrhs, 9.0);
    {
        // step_1, k = 0: v = r - c_0 g_0 - c_1 g_1 = 10 - 2 - 3 = 5
        auto r = filled(hip, n, nrhs, 10.0), v = filled(hip, n, nrhs, 9.0);
        auto g = columns(hip, n, {2.0, 3.0});
        k::idr::step_1(hip, nrhs, 0, m.get(), f.get(), r.get(), g.get(), c.get(), v.get(), &status);
        const auto ch = host_of(c.get());
        ran("idr::step_1", ch[0] == 1.0 && ch[1] == 1.0 && column_equal(v.get(), 0, 5.0));
        // step_2, k = 1: u_1 = omega * helper + c_1 u_1 = 0.5 * 5 + 7 = 9.5, u_0 untouched
        auto u = columns(hip, n, {6.0, 7.0});
        auto omega = initialize<Vec>({0.5}, hip);
        k::idr::step_2(hip, nrhs, 1, omega.get(), v.get(), c.get(), u.get(), &status);
        ran("idr::step_2", column_equal(u.get(), 0, 6.0) && column_equal(u.get(), 1, 9.5));
    }
    {
        // step_3, k = 1, P = (e, h) / sqrt(n) with e = ones, h = (+1 | -1): g_0 = sqrt(n) e (so p_0 . g_0 = n = m_00),
        // g_k = 2 sqrt(n) e + sqrt(n) h: alpha = p_0 . g_k / m_00 = 2 n / n = 2, g_k -= 2 g_0 -> sqrt(n) h,
        // u_1 -= 2 u_0 = 7 - 2 = 5, m_11 = p_1 . g_k = n, beta = f_1 / m_11 = n / n = 1,
        // residual -= g_k -> 1 - sqrt(n) h, x += u_1 -> 5
        const double rt = std::sqrt(double(n));
        auto ph = Vec::create(hip->get_master(), dim<2>(s, n));
        auto gh = Vec::create(hip->get_master(), dim<2>(n, s)), gkh = Vec::create(hip->get_master(), dim<2>(n, 1));
        for (size_type j = 0; j < n; ++j) {
            const double h = j < n / 2 ? 1.0 : -1.0;
            ph->at(0, j) = 1.0 / rt;
            ph->at(1, j) = h / rt;
            gh->at(j, 0) = rt;
            gh->at(j, 1) = 0.0;
            gkh->at(j, 0) = 2.0 * rt + rt * h;
        }
        auto p = ph->clone(hip), g = gh->clone(hip), g_k = gkh->clone(hip);
        auto u = columns(hip, n, {1.0, 7.0});
        auto m3 = initialize<Vec>({{double(n), 0.0}, {0.0, 9.0}}, hip);
        auto f3 = initialize<Vec>({0.0, double(n)}, hip);
        auto alpha = filled(hip, 1, nrhs, 9.0), residual = filled(hip, n, nrhs, 1.0), x = filled(hip, n, nrhs, 0.0);
        k::idr::step_3(hip, nrhs, 1, p.get(), g.get(), g_k.get(), u.get(), m3.get(), f3.get(), alpha.get(), residual.get(), x.get(), &status);
        const auto gg = host_of(g.get()), rr = host_of(residual.get()), mm = host_of(m3.get());
        bool ok = column_equal(u.get(), 1, 5.0, 1e-9) && column_equal(x.get(), 0, 5.0, 1e-9) && std::abs(mm[3] - double(n)) < 1e-8;
        for (size_type j = 0; j < n; ++j) {
            const double h = j < n / 2 ? 1.0 : -1.0;
            ok = ok && std::abs(gg[2 * j + 1] - rt * h) < 1e-9 && std::abs(rr[j] - (1.0 - rt * h)) < 1e-8;
        }
        ran("idr::step_3", ok);
    }
    {
        // compute_omega: thr = 2, tht = 16, |r| = 1: omega = 1/8, |rho| = 2 / (4 * 1) = 0.5 < 0.7 -> omega *= 0.7 / 0.5
        auto omega = initialize<Vec>({2.0}, hip), tht = initialize<Vec>({16.0}, hip), rn = initialize<Vec>({1.0}, hip);
        k::idr::compute_omega(hip, nrhs, 0.7, tht.get(), rn.get(), omega.get(), &status);
        ran("idr::compute_omega", hip->copy_val_to_host(omega->get_const_values()) == 0.125 * (0.7 / 0.5));
    }
    return wrong;
}
