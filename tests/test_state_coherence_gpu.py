"""Cached matrix state must follow every change made to a matrix.

The objects users hold -- gko::matrix::Csr / Coo / Hybrid of the C++ mirror and gkomi.formats.Csr / Csr64 / Coo --
cache data derived from their arrays (srow, the longest row that goes to every kernel as its hint, the column
statistic, the column-partitioned COPY of the gkomi_partitioned strategy, the sorted-rows state of Coo).  Every
scenario here: build the object, apply once (caches warm), change the matrix through one mutator, apply again, and
build a FRESH object from the final arrays.  examples/state_coherence.cpp drives the C++ objects as a child process
(one per group of scenarios that share matrices); the Python objects are driven in this process.

Checks, in this order:
  * the scenario can see staleness (a condition on the inputs, computed on the CPU): what a stale cache would give
    -- old values, or new values beside old columns -- lies beyond 1000 x the bound below in >= 90 % of the rows;
  * against the oracle on the final arrays: |y - y_ref| <= 2 (len_i + 2) u (|alpha| sum_j |a_ij b_j| + |beta c_i|),
    u = 2^-53 (2^-24 for float): the worst-case rounding error of ANY summation order of a row of len_i products
    (+ the scaling and the beta c term), taken twice because y and y_ref are both rounded sums.  Derived, not tuned;
    it holds for the partitioned copy and the load-balanced kernel as well.  Where the suite already demands the
    oracle's bits for a strategy and shape (merge_path and Csr<double, int64> on the 532 x 231 matrix:
    test_csr_spmv_gpu.py::test_random_532x231[stream], test_csr_i64_gpu.py::test_random_532x231_int64), bits;
  * against the fresh object: bitwise equal.  Two exceptions, both because a fresh object may legitimately differ:
    the load_balance strategy adds the parts of a row that a tile cuts with fp64 atomics (csrc/csr_spmv.hip, as the
    reference does), so its bits are not reproducible between two launches; and gkomi_partitioned WITHOUT a pinned
    block count, whose analysis TIMES two block counts and may decline (the state tests pin the copy with
    gkomi_partitioned(blocks) / colpart(nb); one scenario keeps the automatic form and asserts correctness only).
    These compare with the fresh object's product within twice the bound instead.
No scenario skips or accepts "either outcome": a precondition that does not hold (no copy, rows not sorted) fails."""
import os
import subprocess

import numpy as np
import pytest
import torch

import matgen
from gkomi import formats
from gpu_util import dev, host, stream_ptr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EX = os.path.join(os.path.dirname(HERE), "repo-8852-ginkgo_amd", "examples")
U64, U32 = 2.0 ** -53, 2.0 ** -24
ALPHA, BETA = -0.75, 1.5
STRATEGIES = ["classical", "load_balance", "merge_path", "automatical", "sparselib", "gkomi_partitioned2"]


# ---------------------------------------------------------------- matrices (all generated here, numpy only)
class Mat:
    """a matrix in CSR (rp) or COO (ri) form + the vectors its products are taken with"""

    def __init__(self, rows, cols, ci, v, rp=None, ri=None, seed=0):
        self.rows, self.cols = int(rows), int(cols)
        self.rp = None if rp is None else np.ascontiguousarray(rp, np.int32)
        self.ri = None if ri is None else np.ascontiguousarray(ri, np.int32)
        self.ci, self.v = np.ascontiguousarray(ci, np.int32), np.ascontiguousarray(v, np.float64)
        rng = np.random.default_rng(1000 + seed)
        self.b = {k: rng.standard_normal((self.cols, k)) for k in (1, 3)}
        self.c = {k: rng.standard_normal((self.rows, k)) for k in (1, 3)}

    def with_(self, **kw):
        m = Mat.__new__(Mat)
        m.__dict__.update(self.__dict__)
        for k, val in kw.items():
            setattr(m, k, np.ascontiguousarray(val, np.float64 if k == "v" else np.int32))
        return m

    def csr(self):
        """(rp, ci, v) of the matrix; COO entries go to their rows in storage order"""
        if self.rp is not None:
            return self.rp, self.ci, self.v
        order = np.argsort(self.ri, kind="stable")
        rp = np.zeros(self.rows + 1, np.int32)
        np.cumsum(np.bincount(self.ri, minlength=self.rows), out=rp[1:])
        return rp, self.ci[order], self.v[order]

    def row_of_entry(self):
        return np.repeat(np.arange(self.rows), np.diff(self.rp))

    def write(self, d, shared=None):
        """raw little-endian arrays for the driver; arrays that are `shared`'s own (another written Mat) are linked"""
        os.makedirs(d)
        self.dir = d
        if shared is self:
            shared = None
        with open(os.path.join(d, "meta.txt"), "w") as f:
            f.write(f"{self.rows} {self.cols} {len(self.v)}\n")
        arrays = {"rp.i32": self.rp, "ri.i32": self.ri, "ci.i32": self.ci, "v.f64": self.v}
        for k in (1, 3):
            arrays[f"b{k}.f64"], arrays[f"c{k}.f64"] = self.b[k], self.c[k]
        key = {"rp.i32": "rp", "ri.i32": "ri", "ci.i32": "ci", "v.f64": "v"}
        for name, a in arrays.items():
            if a is None:
                continue
            if shared is not None and name in key and getattr(shared, key[name]) is a:
                os.symlink(os.path.join(shared.dir, name), os.path.join(d, name))
            else:
                np.ascontiguousarray(a).astype(a.dtype.newbyteorder("<"), copy=False).tofile(os.path.join(d, name))


def shuffle_rows(m, seed):
    """the same matrix with the entries of every row in another order"""
    rng = np.random.default_rng(seed)
    p = np.lexsort((rng.random(len(m.ci)), m.row_of_entry()))
    return m.with_(ci=m.ci[p], v=m.v[p])


def sort_rows(m):
    p = np.lexsort((m.ci, m.row_of_entry()))
    return m.with_(ci=m.ci[p], v=m.v[p])


def transpose(m, seed):
    """rows of the transpose ordered by the original row (what csr::transpose gives)"""
    p = np.argsort(m.ci, kind="stable")
    rp = np.zeros(m.cols + 1, np.int32)
    np.cumsum(np.bincount(m.ci, minlength=m.cols), out=rp[1:])
    return Mat(m.cols, m.rows, m.row_of_entry()[p], m.v[p], rp=rp, seed=seed)


def grow_row(m, r0, longer_than):
    """same nnz, row boundaries moved: row r0 swallows the rows behind it until it has more than `longer_than`
    nonzeros; the swallowed rows become empty"""
    rp = m.rp.copy()
    j = 1
    while rp[r0 + j] - rp[r0] <= longer_than:
        j += 1
    rp[r0 + 1:r0 + j] = rp[r0 + j]
    return m.with_(rp=rp)


def empty_run(m, r0, run):
    """same nnz: rows r0 .. r0+run-1 become empty, their nonzeros go evenly to the `run` rows behind them"""
    rp = m.rp.copy()
    lo, hi = int(rp[r0]), int(rp[r0 + 2 * run])
    rp[r0:r0 + run] = lo
    rp[r0 + run:r0 + 2 * run + 1] = lo + (np.arange(run + 1) * (hi - lo)) // run
    return m.with_(rp=rp)


def unsorted_rows_fraction(m):
    d = np.diff(m.ci.astype(np.int64)) < 0
    inside = m.row_of_entry()[1:] == m.row_of_entry()[:-1]
    bad = np.bincount(m.row_of_entry()[1:][d & inside], minlength=m.rows) > 0
    return bad.mean()


def f32_exact(m):
    return m.with_(v=m.v.astype(np.float32).astype(np.float64))


# ---------------------------------------------------------------- oracle + bound
def oracle_product(oracle, m, k, advanced, f32=False, plus=None):
    """y_ref and the bound per entry.  plus = (alpha,): apply2, c + alpha A b (alpha None = 1)"""
    rp, ci, v = m.csr()
    b, c = m.b[k], m.c[k]
    alpha, beta = (ALPHA, BETA) if advanced else (None, None)
    if plus is not None:
        alpha, beta = (1.0 if plus[0] is None else plus[0]), 1.0
    if f32:
        v, b, c = v.astype(np.float32), b.astype(np.float32), c.astype(np.float32)
    if alpha is None:
        y = np.full((m.rows, k), np.nan, b.dtype)
        (oracle.ref_csr_spmv_f32 if f32 else oracle.ref_csr_spmv)(m.rows, k, rp, ci, v, b, k, y, k)
    else:
        y = c.copy()
        (oracle.ref_csr_advanced_spmv_f32 if f32 else oracle.ref_csr_advanced_spmv)(m.rows, k, alpha, rp, ci, v, b, k, beta, y, k)
    rows = np.repeat(np.arange(m.rows), np.diff(rp))
    absum = np.stack([np.bincount(rows, weights=np.abs(v.astype(np.float64) * b[ci, j].astype(np.float64)), minlength=m.rows)
                      for j in range(k)], axis=1)
    scale = absum if alpha is None else abs(alpha) * absum + np.abs(beta * c.astype(np.float64))
    bound = 2.0 * (np.diff(rp).reshape(-1, 1) + 2) * (U32 if f32 else U64) * scale
    return y.astype(np.float64), bound


def assert_staleness_visible(oracle, final, stale, what, rows=None):
    """a condition on the INPUTS: the product a stale cache would give is far outside the bound in most rows"""
    ref, bound = oracle_product(oracle, final, 1, False)
    wrong, _ = oracle_product(oracle, stale, 1, False)
    seen = np.abs(wrong - ref) > 1000.0 * bound
    if rows is not None:
        seen = seen[rows]
    print(f"  staleness ({what}): {100 * seen.mean():.2f} % of rows beyond 1000 x bound")
    assert seen.mean() >= 0.9, what


class Products:
    """the products one scenario left under out/"""

    def __init__(self, out, sid):
        self.out, self.sid = out, sid
        self.info = {}
        with open(os.path.join(out, sid + ".info")) as f:
            for line in f:
                key, val = line.split()
                self.info[key] = val

    def get(self, tag, rows, k):
        y = np.fromfile(os.path.join(self.out, f"{self.sid}.{tag}.f64"), dtype="<f8")
        assert y.size == rows * k, (tag, y.size, rows, k)
        return y.reshape(rows, k)

    def raw(self, name, dtype):
        return np.fromfile(os.path.join(self.out, f"{self.sid}.{name}.raw"), dtype=dtype)


def check(oracle, p, prefix, m, three, f32=False, bits=False, fresh=None, fresh_bits=True, modes=("", "a")):
    """products <prefix>{1,a1,3,a3} against the oracle on m (bound, or bits), then against the fresh object's"""
    for k in (1, 3) if three else (1,):
        for mode in modes:
            tag = f"{prefix}{mode}{k}"
            plus = {"p": (None,), "q": (ALPHA,)}.get(mode)
            ref, bound = oracle_product(oracle, m, k, mode == "a", f32, plus)
            y = p.get(tag, m.rows, k)
            err = np.abs(y - ref)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)))
            line = f"  {p.sid}.{tag}: max |y - y_ref| / bound = {ratio:.3g}, bitwise = {np.array_equal(y, ref)}"
            if fresh is not None:
                yf = p.get(f"{fresh}{mode}{k}", m.rows, k)
                line += f", equals fresh bitwise = {np.array_equal(y, yf)}"
            print(line)
            assert np.all(err <= bound), tag            # (a NaN fails this)
            if bits:
                assert np.array_equal(y, ref), tag
            if fresh is not None:
                assert np.all(np.abs(yf - ref) <= bound), tag + " (fresh)"
                if fresh_bits:
                    assert np.array_equal(y, yf), tag + " differs from the fresh object's"
                else:
                    assert np.all(np.abs(y - yf) <= 2.0 * bound), tag


def reproducible(strategy):
    """may two objects of this strategy over the same arrays differ in bits?  (module docstring: atomics, timed analysis)"""
    return strategy not in ("load_balance", "gkomi_partitioned")


# ---------------------------------------------------------------- the child process
@pytest.fixture(scope="module")
def driver():
    r = subprocess.run(["make", "-C", EX], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(EX, "bin", "state_coherence")


def run_driver(driver, d, mats, scenarios, timeout):
    """writes the matrices and scenarios.txt under d, runs the driver once (one child, a time limit of its own)"""
    for name, m in mats.items():            # "X_something" links the arrays it has in common with "X"
        m.write(os.path.join(d, name), mats.get(name.split("_")[0]))
    os.makedirs(os.path.join(d, "out"))
    with open(os.path.join(d, "scenarios.txt"), "w") as f:
        for sid, s in scenarios.items():
            f.write(f"{sid} {s['object']} {s['strategy']} {s['mutator']} {s['base']} {s['payload']} {int(s.get('three', 0))} {int(s.get('dump', 0))}\n")
    try:
        r = subprocess.run([driver, str(d)], capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        pytest.exit("state_coherence hung: nothing more is started on this GPU", returncode=1)
    print(r.stdout[-2000:], r.stderr[-2000:])
    if r.returncode < 0:    # died of a signal (a GPU fault aborts the process): stop the session, start nothing more
        pytest.exit(f"state_coherence died of signal {-r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-2000:]}", returncode=1)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"scenarios {len(scenarios)}" in r.stdout
    return os.path.join(d, "out")


def S(obj, strategy, mutator, base, payload, **kw):
    return dict(object=obj, strategy=strategy, mutator=mutator, base=base, payload=payload, **kw)


# ---------------------------------------------------------------- small matrices: every strategy x every mutator
def small_matrices():
    M = {}
    rng = np.random.default_rng(2024)
    rp, ci, v = matgen.random_csr(532, 231, 1, 231, seed=42, sort=False)
    R = M["R"] = Mat(532, 231, ci, v, rp=rp, seed=1)
    M["R_values"] = R.with_(v=R.v * rng.uniform(0.5, 2.0, len(R.v)))
    M["R_values2"] = R.with_(v=R.v * rng.uniform(0.5, 2.0, len(R.v)))
    M["R_values3"] = R.with_(v=R.v * rng.uniform(0.5, 2.0, len(R.v)))
    M["R_perm"] = shuffle_rows(R, 5)
    M["R_cols"] = R.with_(ci=(R.ci + 57) % 231)                       # other columns under the same values
    M["R_sorted"] = sort_rows(R)
    M["R_builder"] = R.with_(ci=(R.ci + 101) % 231, v=R.v * rng.uniform(0.5, 2.0, len(R.v)))
    M["R_T"] = transpose(R, 2)
    for i, name in enumerate(("R_values2", "R_values3", "R"), 1):    # the rounds of the "repeated" scenarios
        M[f"R_values_r{i}"] = M[name].with_()
    # a matrix of another size and nnz, values exactly representable in float (for the conversion from Csr<float>)
    rp, ci, v = matgen.random_csr(300, 411, 0, 40, seed=7, sort=False)
    M["Q"] = f32_exact(Mat(300, 411, ci, v, rp=rp, seed=3))
    # short rows (6-11) so that a moved row boundary makes the cached longest row wrong by a lot
    rp, ci, v = matgen.random_rows_csr(3000, 3000, rng.integers(6, 12, size=3000), 11)
    T = M["T"] = shuffle_rows(Mat(3000, 3000, ci, v, rp=rp, seed=4), 6)
    M["T_values"] = T.with_(v=T.v * rng.uniform(0.5, 2.0, len(T.v)))
    M["T_long64"] = grow_row(T, 100, 64)
    M["T_long256"] = grow_row(T, 1700, 256)
    M["T_empty"] = empty_run(T, 900, 300)
    # COO: sorted rows of at most 11 entries; the same entries under shuffled row indices; sorted rows, one > 64
    ri = T.row_of_entry().astype(np.int32)
    C = M["C"] = Mat(3000, 3000, T.ci, T.v, ri=ri, seed=5)
    M["C_unsorted"] = C.with_(ri=ri[rng.permutation(len(ri))])
    M["C_long"] = C.with_(ri=np.repeat(np.arange(3000), np.diff(M["T_long256"].rp)))
    M["Qcoo"] = Mat(300, 411, M["Q"].ci, M["Q"].v, ri=M["Q"].row_of_entry(), seed=3)
    # SPD system of the solver scenario: 2-D Poisson, then a positive diagonal shift that varies along the diagonal
    n, rp, ci, v = matgen.poisson_2d_5pt(32)
    P = M["P"] = Mat(n, n, ci, v, rp=rp, seed=8)
    diag = P.row_of_entry() == P.ci
    v2 = P.v.copy()
    v2[diag] += 3.0 + np.sin(np.arange(n))
    M["P_shifted"] = P.with_(v=v2)
    return M


def small_scenarios():
    sc = {}
    for st in STRATEGIES:
        sc[f"values-{st}"] = S("csr", st, "values", "R", "R_values", three=1)
        sc[f"cols_permuted-{st}"] = S("csr", st, "cols", "R", "R_perm", three=1)
        sc[f"cols_different-{st}"] = S("csr", st, "cols_only", "R", "R_cols")
        sc[f"sort-{st}"] = S("csr", st, "sort", "R", "R_sorted", three=1, dump=1)
        sc[f"rowptrs_longer_than_64-{st}"] = S("csr", st, "rowptrs", "T", "T_long64")
        sc[f"rowptrs_longer_than_256-{st}"] = S("csr", st, "rowptrs", "T", "T_long256", three=1)
        sc[f"rowptrs_empty_run-{st}"] = S("csr", st, "rowptrs", "T", "T_empty")
    for st in ("automatical", "gkomi_partitioned2"):
        sc[f"read_matrix_data-{st}"] = S("csr", st, "read_md", "R", "Q", three=1)
        sc[f"read_device_matrix_data-{st}"] = S("csr", st, "read_dmd", "R", "Q")
        sc[f"convert_from_float-{st}"] = S("csr", st, "convert_from_float", "R", "Q")
        sc[f"builder-{st}"] = S("csr", st, "builder", "R", "R_builder", three=1)
        sc[f"transpose-{st}"] = S("csr", st, "transpose", "R", "R_T", dump=1)
        sc[f"repeated-{st}"] = S("csr", st, "repeated", "R", "R_values")
    sc["set_strategy-gkomi_partitioned2-to-classical"] = S("csr", "gkomi_partitioned2", "set_strategy=classical", "R", "R", three=1)
    sc["set_strategy-classical-to-gkomi_partitioned2"] = S("csr", "classical", "set_strategy=gkomi_partitioned2", "R", "R", three=1)
    sc["set_strategy-automatical-to-load_balance"] = S("csr", "automatical", "set_strategy=load_balance", "R", "R", three=1)
    for obj in ("csr64", "csrf"):
        sc[f"{obj}-values"] = S(obj, "automatical", "values", "R", "R_values", three=1)
        sc[f"{obj}-rowptrs_longer_than_256"] = S(obj, "automatical", "rowptrs", "T", "T_long256", three=1)
        sc[f"{obj}-read_matrix_data"] = S(obj, "automatical", "read_md", "R", "Q", three=1)
    sc["coo-rows_unsorted"] = S("coo", "-", "rows", "C", "C_unsorted")
    sc["coo-rows_longer_than_64"] = S("coo", "-", "rows", "C", "C_long")
    sc["coo-resize"] = S("coo", "-", "resize", "C", "Qcoo")
    sc["coo-convert_from_csr"] = S("coo", "-", "convert_from_csr", "C_unsorted", "Q")
    sc["hybrid-convert_from_csr"] = S("hybrid", "-", "convert_from_csr", "T", "Q")
    sc["cg-values"] = S("cg", "automatical", "values", "P", "P_shifted")
    return sc


SMALL = small_scenarios()


@pytest.fixture(scope="module")
def small(driver, tmp_path_factory):
    d = tmp_path_factory.mktemp("state_small")
    M = small_matrices()
    return run_driver(driver, d, M, SMALL, timeout=300), M


def check_csr_scenario(oracle, out, M, sid, s):
    """the checks of the module docstring for one Csr scenario"""
    p = Products(out, sid)
    base, final = M[s["base"]], M[s["payload"]]
    st, mut, three = s["strategy"], s["mutator"], bool(s.get("three"))
    f32 = s["object"] == "csrf"
    final_st = mut.split("=")[1] if mut.startswith("set_strategy=") else st
    pinned = st.startswith("gkomi_partitioned") and st != "gkomi_partitioned"
    # 1. the scenario can see staleness / its precondition holds
    if mut == "values":
        assert_staleness_visible(oracle, final, base, "old values")
    elif mut == "cols":
        assert_staleness_visible(oracle, final, base.with_(v=final.v), "new values beside old columns")
        ref, bound = oracle_product(oracle, final, 1, False)
        same, _ = oracle_product(oracle, base, 1, False)
        assert np.all(np.abs(same - ref) <= bound)                       # the same matrix in another order
    elif mut in ("cols_only", "builder"):
        assert_staleness_visible(oracle, final, base, "old matrix")
        assert_staleness_visible(oracle, final, base.with_(v=final.v), "new values beside old columns")
    elif mut == "sort":
        frac = unsorted_rows_fraction(base)
        print(f"  rows unsorted before the sort: {100 * frac:.2f} %")
        assert frac >= 0.9 and unsorted_rows_fraction(final) == 0.0
        assert_staleness_visible(oracle, final, base.with_(v=final.v), "sorted values beside unsorted columns")
    elif mut == "rowptrs":
        lb, lf = np.diff(base.rp).max(), np.diff(final.rp).max()
        assert lb <= 11 and np.array_equal(base.ci, final.ci) and base.rp[-1] == final.rp[-1]
        if "longer_than_64" in sid:
            assert 64 < lf <= 256
        elif "longer_than_256" in sid:
            assert lf > 256
        else:
            assert np.array_equal(np.diff(final.rp)[900:1200], np.zeros(300)) and lf > lb
    elif mut in ("read_md", "read_dmd", "convert_from_float"):
        assert (base.rows, base.cols, len(base.v)) != (final.rows, final.cols, len(final.v))
    elif mut == "repeated":
        for i in (1, 2, 3):
            prev = base if i == 1 else M[f"{s['payload']}_r{i - 1}"]
            assert_staleness_visible(oracle, M[f"{s['payload']}_r{i}"], prev, f"round {i}: the values of the round before")
        assert_staleness_visible(oracle, final, M[f"{s['payload']}_r3"], "last write: the values of round 3")
    # 2. the pinned copy exists where the scenario relies on it
    if pinned:
        assert p.info["has_copy_warm"] == "1", "no partitioned copy although the block count is pinned"
    if final_st.startswith("gkomi_partitioned") and final_st != "gkomi_partitioned" and not f32 and s["object"] == "csr":
        assert p.info["has_copy_after"] == "1" and p.info["has_copy_fresh"] == "1"
    if not final_st.startswith("gkomi_partitioned"):
        assert p.info["has_copy_after"] == "0" and p.info["has_copy_fresh"] == "0"
    # 3. oracle, then the fresh object
    on_532 = (final.rows, final.cols) == (532, 231)
    bits = on_532 and (final_st == "merge_path" or s["object"] == "csr64")
    check(oracle, p, "w", base, three, f32)                              # the warm apply (the driver itself is sane)
    if mut == "repeated":
        for i in (1, 2, 3):
            check(oracle, p, f"r{i}y", M[f"{s['payload']}_r{i}"], False, f32, bits)
    check(oracle, p, "y", final, three, f32, bits, fresh="f", fresh_bits=reproducible(final_st))
    if mut == "transpose":
        check(oracle, p, "o", base, three, f32, fresh="w", fresh_bits=reproducible(st))   # the original, undisturbed
        assert p.info["has_copy_original"] == p.info["has_copy_warm"]
    if mut == "convert_from_float":
        assert p.info["strategy_after"] == ("gkomi_partitioned" if st.startswith("gkomi_partitioned") else st)
    if s.get("dump"):
        assert np.array_equal(p.raw("rp", "<i4"), final.rp) and np.array_equal(p.raw("ci", "<i4"), final.ci)
        assert np.array_equal(p.raw("v", "<f8"), final.v)


@pytest.mark.parametrize("sid", [k for k, s in SMALL.items() if s["object"] in ("csr", "csr64", "csrf")])
def test_csr_small(small, oracle, sid):
    out, M = small
    check_csr_scenario(oracle, out, M, sid, SMALL[sid])


@pytest.mark.parametrize("sid", [k for k, s in SMALL.items() if s["object"] == "coo"])
def test_coo(small, oracle, sid):
    """Coo<double, int32>: apply, advanced apply, apply2 and alpha apply2 on one and three columns.  A stale
    sorted-rows state runs the atomic-free kernels on unsorted rows, a stale longest row is a hint that is too small:
    both give a wrong product by the kernels' contract (test_coo_sorted_gpu.py)"""
    out, M = small
    s = SMALL[sid]
    p = Products(out, sid)
    base, final = M[s["base"]], M[s["payload"]]
    sorted_rows = lambda m: m.ri is None or bool(np.all(np.diff(m.ri) >= 0))
    longest = lambda m: np.diff(m.csr()[0]).max()
    if sid == "coo-rows_unsorted":
        assert sorted_rows(base) and not sorted_rows(final) and np.mean(np.diff(final.ri) < 0) > 0.4
    elif sid == "coo-rows_longer_than_64":
        assert sorted_rows(base) and sorted_rows(final) and longest(base) <= 64 < longest(final)
    elif sid == "coo-resize":
        assert len(base.v) != len(final.v) and sorted_rows(final)
    else:
        assert not sorted_rows(base) and len(base.v) != len(final.v)
    assert p.info["sorted_warm"] == str(int(sorted_rows(base)))
    assert p.info["sorted_after"] == p.info["sorted_fresh"] == str(int(sorted_rows(final)))
    modes = ("", "a", "p", "q")
    check(oracle, p, "w", base, True, modes=modes)
    # unsorted rows go through the atomic kernels: not reproducible in bits, like load_balance
    check(oracle, p, "y", final, True, fresh="f", fresh_bits=sorted_rows(final), modes=modes)


def test_hybrid_convert_into_a_warm_object(small, oracle):
    out, M = small
    p = Products(out, "hybrid-convert_from_csr")
    base, final = M["T"], M["Q"]
    assert int(p.info["coo_nnz_warm"]) == int(np.maximum(np.diff(base.rp) - 3, 0).sum()) > 0
    assert int(p.info["coo_nnz_after"]) == int(np.maximum(np.diff(final.rp) - 3, 0).sum()) > 0
    check(oracle, p, "w", base, True)
    check(oracle, p, "y", final, True, fresh="f")


def test_solver_generated_once_used_twice(small, oracle):
    """Cg (no preconditioner) generated once on an SPD matrix; solve, new values through get_values(), solve again
    (the time-stepping idiom): the second solution is the new matrix's.  The solver stops at a residual reduction of
    1e-10; the shifted matrix has eigenvalues in [2, 12] (Gershgorin: diagonal 6..8, off-diagonal row sums <= 4), so
    cond <= 6 and the relative error of a solution is at most cond x 1e-10, of two solutions against each other
    twice that; the true residual may exceed the recurrence's by rounding, n u cond ~ 1e-12: bar 2e-10."""
    out, M = small
    p = Products(out, "cg-values")
    old, new = M["P"], M["P_shifted"]
    b = new.b[1]

    def residual(m, x):
        r = b.copy()
        oracle.ref_csr_advanced_spmv(m.rows, 1, -1.0, m.rp, m.ci, m.v, x, 1, 1.0, r, 1)
        return np.linalg.norm(r) / np.linalg.norm(b)
    x_old = np.zeros(old.rows)
    oracle.ref_cg_solve(old.rows, old.rp, old.ci, old.v, b[:, 0].copy(), x_old, 1000, 1e-10, 0, None, 0)
    stale = residual(new, x_old.reshape(-1, 1))
    print(f"  the old matrix's solution in the new system: relative residual {stale:.3g}")
    assert stale >= 1000 * 2e-10                                        # the scenario can see a stale matrix
    assert p.info["converged_w1"] == p.info["converged_y1"] == p.info["converged_f1"] == "1"
    assert residual(old, p.get("w1", old.rows, 1)) <= 2e-10
    x2, xf = p.get("y1", new.rows, 1), p.get("f1", new.rows, 1)
    print(f"  second solve: residual {residual(new, x2):.3g}, vs fresh solver {np.linalg.norm(x2 - xf) / np.linalg.norm(xf):.3g}, "
          f"bitwise {np.array_equal(x2, xf)}, iterations {p.info['iterations_y1']} / {p.info['iterations_f1']}")
    assert residual(new, x2) <= 2e-10
    assert np.linalg.norm(x2 - xf) <= 2 * 6 * 1e-10 * np.linalg.norm(xf)


# ---------------------------------------------------------------- the large matrix: a shape the copy is made for
LARGE_N = 600000
P4 = "gkomi_partitioned4"
LARGE = {
    f"values-{P4}": S("csr", P4, "values", "L", "L_values", three=1),
    f"cols_permuted-{P4}": S("csr", P4, "cols", "L", "L_perm"),
    f"cols_different-{P4}": S("csr", P4, "cols_only", "L", "L_cols"),
    f"sort-{P4}": S("csr", P4, "sort", "L", "L_sorted", three=1, dump=1),
    f"rowptrs_longer_than_256-{P4}": S("csr", P4, "rowptrs", "L", "L_long"),
    f"builder-{P4}": S("csr", P4, "builder", "L", "L_builder"),
    f"transpose-{P4}": S("csr", P4, "transpose", "L", "L_T", dump=1),
    f"repeated-{P4}": S("csr", P4, "repeated", "L", "L_values"),
    f"read_matrix_data-{P4}": S("csr", P4, "read_md", "L", "Q"),
    f"convert_from_float-{P4}": S("csr", P4, "convert_from_float", "L", "Q"),
    f"set_strategy-{P4}-to-classical": S("csr", P4, "set_strategy=classical", "L", "L", three=1),
    f"set_strategy-classical-to-{P4}": S("csr", "classical", f"set_strategy={P4}", "L", "L"),
    # the automatic form (the analysis times the copy and may decline): correctness only
    "sort-gkomi_partitioned": S("csr", "gkomi_partitioned", "sort", "L", "L_sorted"),
    "sort-automatical": S("csr", "automatical", "sort", "L", "L_sorted"),
    "values-automatical": S("csr", "automatical", "values", "L", "L_values"),
}


@pytest.fixture(scope="module")
def large(driver, tmp_path_factory, gk):
    """n = ncols = 600 000, 6-11 nonzeros per row, uniform columns (the shape of test_csr_colpart_gpu.py): b
    overflows an L2, gkomi_csr_colpart_blocks_for = 4"""
    d = tmp_path_factory.mktemp("state_large")
    n = LARGE_N
    rng = np.random.default_rng(1)
    rp, ci, v = matgen.random_rows_csr(n, n, rng.integers(6, 12, size=n), 2)
    assert gk.csr_colpart_blocks_for(n, n, len(v)) == 4
    M = {}
    L = M["L"] = shuffle_rows(Mat(n, n, ci, v, rp=rp, seed=20), 21)
    M["L_values"] = L.with_(v=L.v * rng.uniform(0.5, 2.0, len(L.v)))
    M["L_perm"] = shuffle_rows(L, 22)
    M["L_cols"] = L.with_(ci=(L.ci + 200003) % n)
    M["L_sorted"] = sort_rows(L)
    M["L_long"] = grow_row(L, 1000, 256)
    M["L_builder"] = L.with_(ci=(L.ci + 100003) % n, v=L.v * rng.uniform(0.5, 2.0, len(L.v)))
    M["L_T"] = transpose(L, 23)
    M["L_values_r1"] = L.with_(v=M["L_builder"].v)        # the rounds of the "repeated" scenario
    M["L_values_r2"] = L.with_(v=M["L_perm"].v)
    M["L_values_r3"] = L.with_()
    qrp, qci, qv = matgen.random_csr(300, 411, 0, 40, seed=7, sort=False)
    M["Q"] = f32_exact(Mat(300, 411, qci, qv, rp=qrp, seed=3))
    return run_driver(driver, d, M, LARGE, timeout=600), M


@pytest.mark.parametrize("sid", list(LARGE))
def test_csr_large(large, oracle, sid):
    out, M = large
    check_csr_scenario(oracle, out, M, sid, LARGE[sid])


# ---------------------------------------------------------------- the Python objects, in this process
def _py_apply(M, m, k, advanced):
    b = dev(m.b[k])
    if advanced:
        return host(M.apply(b, dev(m.c[k]), ALPHA, BETA))
    return host(M.apply(b, torch.full((m.rows, k), float("nan"), dtype=torch.float64, device="cuda:0")))


def _py_check(oracle, M, F, m, bits):
    for k in (1, 3):
        for advanced in (False, True):
            ref, bound = oracle_product(oracle, m, k, advanced)
            y = _py_apply(M, m, k, advanced)
            yf = _py_apply(F, m, k, advanced)
            err = np.abs(y - ref)
            print(f"  k={k} advanced={advanced}: max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3g}, equals fresh {np.array_equal(y, yf)}")
            assert np.all(err <= bound)
            if bits:
                assert np.array_equal(y, ref)
            assert np.all(np.abs(yf - ref) <= bound) and np.array_equal(y, yf)


PY_CHANGES = ["values", "cols_permuted", "cols_different", "sort", "rowptrs_longer_than_256", "rowptrs_empty_run"]


@pytest.mark.parametrize("change", PY_CHANGES)
@pytest.mark.parametrize("kind", ["csr", "csr_partitioned", "csr64"])
def test_python_csr_objects(gk, oracle, kind, change):
    """formats.Csr with and without PARTITIONED (the copy pinned with colpart(2)) and formats.Csr64: write the
    tensors in place, tell the object (values_changed / structure_changed), apply"""
    M_ = small_matrices()
    base, final = {"values": ("R", "R_values"), "cols_permuted": ("R", "R_perm"), "cols_different": ("R", "R_cols"), "sort": ("R", "R_sorted"),
                   "rowptrs_longer_than_256": ("T", "T_long256"), "rowptrs_empty_run": ("T", "T_empty")}[change]
    base, final = M_[base], M_[final]
    part = kind == "csr_partitioned"
    if change == "values":
        assert_staleness_visible(oracle, final, base, "old values")
    elif change in ("cols_permuted", "sort"):
        assert_staleness_visible(oracle, final, base.with_(v=final.v), "new values beside old columns")
    elif change == "cols_different":
        assert_staleness_visible(oracle, final, base, "old matrix")
    if change == "sort":
        assert unsorted_rows_fraction(base) >= 0.9

    def make(m):
        if kind == "csr64":
            return formats.Csr64.from_host(gk, m.rows, m.cols, m.rp, m.ci, m.v)
        A = formats.Csr.from_host(gk, m.rows, m.cols, m.rp, m.ci, m.v, strategy=formats.Csr.CSR_STRATEGIES["csrp" if part else "csr"])
        if part:
            assert A.colpart(2) is not None
        return A
    A = make(base)
    for k in (1, 3):
        ref, bound = oracle_product(oracle, base, k, False)
        assert np.all(np.abs(_py_apply(A, base, k, False) - ref) <= bound)         # warm
    if change == "values":
        A.vals.copy_(dev(final.v))
        A.values_changed()
    else:
        if change == "sort":
            if kind == "csr64":   # no int64 sort kernel: the sorted arrays are written
                A.col_idxs.copy_(dev(final.ci.astype(np.int64)))
                A.vals.copy_(dev(final.v))
            else:
                gk.csr_sort_by_column_index_f64_i32(stream_ptr(), base.rows, A.row_ptrs, A.col_idxs, A.vals)
                assert np.array_equal(host(A.col_idxs), final.ci) and np.array_equal(host(A.vals), final.v)
        else:
            idx = np.int64 if kind == "csr64" else np.int32
            A.row_ptrs.copy_(dev(final.rp.astype(idx)))
            A.col_idxs.copy_(dev(final.ci.astype(idx)))
            A.vals.copy_(dev(final.v))
        A.structure_changed()
        if part:
            assert A._colpart is None and A.colpart(2) is not None               # dropped, and pinned again
    bits = kind == "csr64" and (final.rows, final.cols) == (532, 231)            # test_csr_i64_gpu.py demands bits there
    _py_check(oracle, A, make(final), final, bits)


@pytest.mark.parametrize("change", ["rows_unsorted", "rows_longer_than_64"])
def test_python_coo_object(gk, oracle, change):
    M_ = small_matrices()
    base, final = M_["C"], M_["C_unsorted" if change == "rows_unsorted" else "C_long"]

    def make(m):
        rp, ci, v = M_["T"].csr()
        C = formats.Coo.from_csr(formats.Csr.from_host(gk, m.rows, m.cols, rp, ci, v))
        C.row_idxs.copy_(dev(m.ri))
        return C
    C = make(base)
    ref, bound = oracle_product(oracle, base, 1, False)
    assert np.all(np.abs(_py_apply(C, base, 1, False) - ref) <= bound) and C._sorted is True and C.max_row_nnz <= 64
    C.row_idxs.copy_(dev(final.ri))
    C.structure_changed()
    F = make(final)
    F.structure_changed()         # (make() wrote row_idxs behind from_csr: nothing was cached yet, the call is harmless)
    for k in (1, 3):
        for advanced in (False, True):
            ref, bound = oracle_product(oracle, final, k, advanced)
            y, yf = _py_apply(C, final, k, advanced), _py_apply(F, final, k, advanced)
            assert np.all(np.abs(y - ref) <= bound) and np.all(np.abs(yf - ref) <= bound)
            if change == "rows_longer_than_64":                                  # sorted rows: the atomic-free kernels
                assert np.array_equal(y, yf)
        ref, bound = oracle_product(oracle, final, k, False, plus=(ALPHA,))
        y = host(C.apply2(dev(final.b[k]), dev(final.c[k]), ALPHA))
        assert np.all(np.abs(y - ref) <= bound)
    assert C._sorted is (change == "rows_longer_than_64")
    if change == "rows_longer_than_64":
        assert C.max_row_nnz > 64
