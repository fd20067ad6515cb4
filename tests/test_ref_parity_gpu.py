"""HIP kernels against the reference library's own ReferenceExecutor, directly:
the driver (oracle/_ref/ref_driver, a CPU child process, see ref_exec.py)
computes every expected result, one process for the whole module.  Only what
README.md and DESIGN.md claim bit for bit is compared, by the rule of
test_ref_oracle_parity.py (integers; NaN matches NaN).  The driver is never
optional here.  A clean checkout on a machine that has neither the reference's
sources nor a built oracle/_ref/ cannot have it; there the expected results are
the bytes this very driver wrote for exactly these inputs, kept as
tests/golden/ref_parity_gpu.bin (`python tests/test_ref_parity_gpu.py` records
them where the driver is built; the file is keyed by a hash of the driver's
input, and test_ref_oracle_table.py fails on the build machine when it is not
what the driver gives now).  With neither driver nor a recording for these
inputs the module fails; it never skips.

Shapes are the smallest that cross the kernels' boundaries; the solvers are
not repeated here on generic systems (their reductions are re-ordered on the
device by design, and test_ref_oracle_parity_solvers.py proves the restatements
they are bounded against equal to the reference on the same systems).  On the
exact systems of exact_systems.py, where no summation order changes a bit,
test_whole_solves_exact_gpu.py holds every solve driver to the oracle bit for
bit, iteration count included, and test_ref_oracle_parity_solvers.py holds the
oracle to the reference on the same inputs."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fbcsr_util
import ilu_util
import matgen
import ref_exec
from gkomi import formats, solvers
from gpu_util import DevCsr, csr_apply, csr_apply_srow, dev, host, make_srow, stream_ptr
from ref_cases import GOLDEN, Registry, golden_csr, grid_5pt_reversed, jacobi_written, ok, rhs, rows_csr, run_case
from test_assembly_gpu import gpu_compact, gpu_sort
from ref_exec import COO, CSR, ELL, FBCSR, HYBRID, SELLP, assert_bits

pytestmark = pytest.mark.gpu
REG = Registry()
STREAM, SPLIT = 1, 4          # GKOMI_CSR_* strategies whose sums keep the reference's order for any row length


RECORDING = os.path.join(GOLDEN, "ref_parity_gpu.bin")


@pytest.fixture(scope="module")
def prepared(oracle):
    # the driver where there is one, else what it wrote for these inputs; neither: an error, never a skip
    return REG.prepare(oracle, RECORDING)


def ani1():
    return golden_csr("ani1")


def queue_apply(batch, fmt, m, n, rp, ci, v, b, c0, alpha=None, beta=None, **extra):
    arrays, params = ref_exec.csr_arrays(m, n, rp, ci, v)
    nrhs = b.shape[1]
    arrays.update(b=b.reshape(-1), x=c0.reshape(-1))
    params.update(b_rows=n, b_cols=nrhs, x_rows=m, x_cols=nrhs, fmt=fmt, mode=0 if alpha is None else 1, **extra)
    if alpha is not None:
        params.update(alpha=alpha, beta=beta)
    return batch.add("spmv", arrays, **params)


# ---- CSR: plain (row-cut stream kernel), srow (nonzero-split) and automatic entry points

def csr_matrices():
    mats = {}
    rng = np.random.default_rng(21)
    for tile in (1536, 3072):
        for k in (tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1):
            counts = rng.multinomial(k, np.full(257, 1 / 257))
            counts[100] += counts[7]
            counts[7] = 0                                   # an empty row
            mats[f"nnz{k}"] = rows_csr(257, 300, counts, k)
    counts = rng.integers(0, 12, 257)
    counts[131] = 5000
    mats["row5000"] = rows_csr(257, 6000, counts, 3)
    mats["unsorted"] = rows_csr(257, 300, rng.integers(0, 40, 257), 4, sort=False)
    return mats


CSR_MATS = csr_matrices()


def csr_case(mname):
    m, n, rp, ci, v = CSR_MATS[mname]

    def build(oracle, batch):
        runs = {}
        for nrhs in (1, 3):
            b, c0 = rhs(n, nrhs, 31), rhs(m, nrhs, 32)
            runs[nrhs] = (b, c0, queue_apply(batch, CSR, m, n, rp, ci, v, b, c0),
                          queue_apply(batch, CSR, m, n, rp, ci, v, b, c0, 2.5, -1.0))

        def check(results, gk):
            assert int(rp[-1]) == len(v)
            A = DevCsr(m, n, rp, ci, v)
            own = formats.Csr.from_host(gk, m, n, rp, ci, v)
            srows = {tile: make_srow(gk, A, tile)[0] for tile in (1536, 3072)}
            counts = np.diff(rp)
            inside = rp[:-1] // 1536 == (np.maximum(rp[1:], rp[:-1] + 1) - 1) // 1536
            short = inside & (counts <= 128)

            def absrow(b):
                out = np.zeros((m, b.shape[1]))
                np.add.at(out, np.repeat(np.arange(m), counts), np.abs(v)[:, None] * np.abs(b[ci]))
                return out
            for nrhs, (b, c0, simple, adv) in runs.items():
                es = ok(results[simple])["x"].reshape(m, nrhs)
                ea = ok(results[adv])["x"].reshape(m, nrhs)
                what = f"csr {mname} nrhs={nrhs}"
                assert_bits(host(csr_apply(gk, A, dev(b), strategy=STREAM)), es, what + " plain")
                assert_bits(host(csr_apply(gk, A, dev(b), dev(c0), 2.5, -1.0, STREAM)), ea, what + " plain advanced")
                for tile, srow in srows.items():
                    assert_bits(host(csr_apply_srow(gk, A, dev(b), srow, tile, strategy=SPLIT)), es, f"{what} srow {tile}")
                    assert_bits(host(csr_apply_srow(gk, A, dev(b), srow, tile, dev(c0), 2.5, -1.0, SPLIT)), ea,
                                f"{what} srow {tile} advanced")
                x = torch.full((m, nrhs), float("nan"), dtype=torch.float64, device="cuda:0")
                gs, ga = host(own.apply(dev(b), x)), host(own.apply(dev(b), dev(c0), 2.5, -1.0))
                if counts.max() <= 128:
                    assert_bits(gs, es, what + " automatic")
                    assert_bits(ga, ea, what + " automatic advanced")
                else:
                    # a row of more than 128 nonzeros may go to the load-balanced kernel, which adds long segments
                    # with a whole wave: README and test_csr_spmv_gpu.py claim the reference's bits only for rows
                    # of at most 128 nonzeros inside one 1536-nonzero tile of c = A b, and 4 eps sqrt(longest row)
                    # relative to sum |a_ij b_j| (+ |beta c|) for the rest
                    assert_bits(gs[short], es[short], what + " automatic, short rows")
                    eps = np.finfo(np.float64).eps
                    for got, want, scale, al in ((gs, es, 0.0, 1.0), (ga, ea, np.abs(c0), 2.5)):
                        bound = 4 * eps * np.sqrt(counts.max()) * (al * absrow(b) + scale) + 1e-300
                        assert np.all(np.abs(got - want) <= bound), what + " automatic, long row"
        return check
    return build


for _m in CSR_MATS:
    REG.case(f"csr-{_m}")(csr_case(_m))


# ---- ELL and SELL-P: one thread per row, storage order

def ell_sellp_case(fmt, nrows):
    counts = np.random.default_rng(nrows).integers(0, 9, nrows)
    counts[nrows // 2] = 150
    m, n, rp, ci, v = rows_csr(nrows, 200, counts, nrows + 1)

    def build(oracle, batch):
        code = {"ell": ELL, "sellp": SELLP}[fmt]
        runs = {}
        for nrhs in (1, 3):
            b, c0 = rhs(n, nrhs, 41), rhs(m, nrhs, 42)
            runs[nrhs] = (b, c0, queue_apply(batch, code, m, n, rp, ci, v, b, c0),
                          queue_apply(batch, code, m, n, rp, ci, v, b, c0, -1.0, 2.5))

        def check(results, gk):
            A = formats.Csr.from_host(gk, m, n, rp, ci, v).to(fmt)
            for nrhs, (b, c0, simple, adv) in runs.items():
                x = torch.full((m, nrhs), float("nan"), dtype=torch.float64, device="cuda:0")
                assert_bits(host(A.apply(dev(b), x)), ok(results[simple])["x"].reshape(m, nrhs), f"{fmt} {nrows} nrhs={nrhs}")
                assert_bits(host(A.apply(dev(b), dev(c0), -1.0, 2.5)), ok(results[adv])["x"].reshape(m, nrhs),
                            f"{fmt} {nrows} nrhs={nrhs} advanced")
        return check
    return build


for _fmt in ("ell", "sellp"):
    for _n in (63, 64, 65, 130):
        REG.case(f"{_fmt}-{_n}rows")(ell_sellp_case(_fmt, _n))


# ---- sorted COO: c = A b keeps the reference's order in rows of at most 128 nonzeros inside one tile

COO_TILE = 1536


def coo_case(name, counts, ncols):
    m, n, rp, ci, v = rows_csr(len(counts), ncols, counts, len(counts))

    def build(oracle, batch):
        runs = {}
        for nrhs in (1, 3):
            b = rhs(n, nrhs, 51)
            runs[nrhs] = (b, queue_apply(batch, COO, m, n, rp, ci, v, b, np.zeros((m, nrhs))))

        def check(results, gk):
            A = formats.Csr.from_host(gk, m, n, rp, ci, v).to("coo")
            first = rp[:-1] // COO_TILE
            last = (np.maximum(rp[1:], rp[:-1] + 1) - 1) // COO_TILE
            exact = (first == last) & (np.diff(rp) <= 128)
            assert exact.sum() >= m - 8
            for nrhs, (b, simple) in runs.items():
                x = torch.full((m, nrhs), float("nan"), dtype=torch.float64, device="cuda:0")
                got = host(A.apply(dev(b), x))
                assert A._sorted, "the rows are sorted: the atomic-free kernels must have run"
                want = ok(results[simple])["x"].reshape(m, nrhs)
                assert_bits(got[exact], want[exact], f"sorted coo {name} nrhs={nrhs}")
                # the other rows (cut by a tile, or longer): partial sums per tile, 1e-13 relative (test_coo_sorted_gpu.py)
                assert matgen.rel_err(got, want) <= 1e-13
        return check
    return build


def _register_coo():
    rng = np.random.default_rng(61)
    for k in (COO_TILE - 1, COO_TILE, COO_TILE + 1):
        REG.case(f"coo-nnz{k}")(coo_case(f"nnz{k}", rng.multinomial(k, np.full(130, 1 / 130)), 300))
    counts = rng.integers(0, 9, 130)
    counts[60] = 3 * COO_TILE + 10
    REG.case("coo-row-over-three-tiles")(coo_case("three_tiles", counts, 6000))


_register_coo()


# ---- Fbcsr

def fbcsr_case(bs):
    def build(oracle, batch):
        m, n, rp, ci, v = fbcsr_util.random_block_csr(9, 11, bs, [0, 3, 1, 0, 0, 11, 2, 5, 1], 70 + bs)
        frp, fci, fv = fbcsr_util.csr_to_fbcsr(m, n, bs, rp, ci, v)
        nrhs = 3
        b, c0 = rhs(n, nrhs, 71), rhs(m, nrhs, 72)
        fb = dict(rp=frp, ci=fci, v=fv, b=b.reshape(-1), x=c0.reshape(-1))
        base = dict(m=m, n=n, bs=bs, b_rows=n, b_cols=nrhs, x_rows=m, x_cols=nrhs)
        simple = batch.add("fbcsr_op", fb, op=6, **base)
        adv = batch.add("fbcsr_op", fb, op=7, alpha=2.5, beta=-1.0, **base)

        def check(results, gk):
            buf = torch.zeros(len(fv) + 1, dtype=torch.float64, device="cuda:0")
            buf[1:] = dev(fv)                                  # the values start 8 bytes off a 16-byte boundary
            A = formats.Fbcsr(gk, m // bs, n // bs, bs, dev(frp), dev(fci), buf[1:])
            x = torch.full((m, nrhs), float("nan"), dtype=torch.float64, device="cuda:0")
            assert_bits(host(A.apply(dev(b), x)), ok(results[simple])["x"].reshape(m, nrhs), f"fbcsr bs={bs}")
            assert_bits(host(A.apply(dev(b), dev(c0), 2.5, -1.0)), ok(results[adv])["x"].reshape(m, nrhs),
                        f"fbcsr bs={bs} advanced")
        return check
    return build


for _bs in (1, 2, 3, 4, 7):
    REG.case(f"fbcsr-bs{_bs}")(fbcsr_case(_bs))


# ---- spgemm, advanced_spgemm, spgeam

def spgemm_case(oracle, batch):
    rng = np.random.default_rng(81)
    n = 300
    counts = rng.integers(1, 7, n)
    counts[40] = 260            # dense enough for the dense accumulator
    counts[77] = 0              # an empty result row
    _, _, arp, aci, av = rows_csr(n, n, counts, 82)
    bcounts = rng.integers(1, 6, n)
    bcounts[10] = bcounts[11] = 4
    _, _, brp, bci, bv = rows_csr(n, n, bcounts, 83)
    _, _, drp, dci, dv_ = rows_csr(n, n, rng.integers(0, 5, n), 84)
    # row 5 of A = e_10 - e_11 (and explicit zeros) and rows 10, 11 of B equal: the products cancel to +0.0,
    # which stays stored
    lo, hi = arp[5], arp[6]
    assert hi - lo >= 2
    aci[lo:hi] = np.arange(10, 10 + hi - lo)
    av[lo:hi] = 0.0
    av[lo], av[lo + 1] = 1.0, -1.0
    bci[brp[11]:brp[12]] = bci[brp[10]:brp[11]]
    bv[brp[11]:brp[12]] = bv[brp[10]:brp[11]]
    arrays, params = {}, {}
    for pre, mat in (("a_", (arp, aci, av)), ("b_", (brp, bci, bv)), ("c_", (drp, dci, dv_))):
        ar, pa = ref_exec.csr_arrays(n, n, *mat, pre=pre)
        arrays.update(ar)
        params.update(pa)
    plain = batch.add("spgemm", arrays, mode=0, **params)
    adv = batch.add("spgemm", arrays, mode=1, alpha=2.5, beta=-1.0, **params)
    geam = batch.add("spgemm", arrays, mode=2, alpha=-1.0, beta=2.5, **params)

    def check(results, gk):
        A = formats.Csr.from_host(gk, n, n, arp, aci, av)
        B = formats.Csr.from_host(gk, n, n, brp, bci, bv)
        D = formats.Csr.from_host(gk, n, n, drp, dci, dv_)
        for what, got, idx in (("spgemm", A.spgemm(B), plain), ("advanced_spgemm", A.spgemm(B, 2.5, -1.0, D), adv),
                               ("spgeam", A.spgeam(-1.0, 2.5, D), geam)):
            r = ok(results[idx])
            assert_bits(host(got.row_ptrs), r["c_rp"], what + " row_ptrs")
            assert_bits(host(got.col_idxs), r["c_ci"], what + " col_idxs")
            assert_bits(host(got.vals), r["c_v"], what + " values")
        r = results[plain]
        assert r["c_rp"][78] == r["c_rp"][77], "row 77 of the product is empty"
        cols5 = r["c_ci"][r["c_rp"][5]:r["c_rp"][6]]
        row5 = r["c_v"][r["c_rp"][5]:r["c_rp"][6]]
        hit = np.isin(cols5, bci[brp[10]:brp[11]])
        assert hit.sum() == 4 and not np.any(row5[hit]) and not np.signbit(row5[hit]).any(), "row 5 cancels to +0.0"
    return check


REG.case("spgemm")(spgemm_case)


# ---- exact ILU, exact IC, Lu, Direct

def factor_case(mname, mat):
    n, rp, ci, v = mat

    def build(oracle, batch):
        arrays, params = ref_exec.csr_arrays(n, n, rp, ci, v)
        ilu = batch.add("factor", arrays, kind=2, **params)
        ic = batch.add("factor", arrays, kind=3, **params)
        lu = batch.add("factor", arrays, kind=4, symmetric=1, **params)
        b = rhs(n, 3, 91)
        da, dp = ref_exec.dense_arrays("b", b)
        xa, xp = ref_exec.dense_arrays("x", np.zeros((n, 3)))
        direct = batch.add("direct", {**arrays, **da, **xa}, symmetric=1, **params, **dp, **xp)

        def same_csr(got, r, pre, what):
            for g, k in zip(got, ("rp", "ci", "v")):
                assert_bits(host(g), r[pre + k], f"{mname} {what} {k}")

        def check(results, gk):
            rpd, cid, vd = dev(rp), dev(ci), dev(v)
            p = solvers.ilu_generate(gk, n, rpd, cid, vd)
            same_csr(p.L, ok(results[ilu]), "l_", "Ilu L")
            same_csr(p.U, results[ilu], "u_", "Ilu U")
            p = solvers.ic_generate(gk, n, rpd, cid, vd)
            same_csr(p.L, ok(results[ic]), "l_", "Ic L")
            same_csr(p.Lt, results[ic], "u_", "Ic L^T")
            f = solvers.lu_generate(gk, n, rpd, cid, vd, symmetric_sparsity=True)
            same_csr(f.combined, ok(results[lu]), "lu_", "Lu")
            x = torch.full((n, 3), float("nan"), dtype=torch.float64, device="cuda:0")
            d = solvers.Direct(gk, f, nrhs=3)
            assert_bits(host(d.apply(dev(b), x)), ok(results[direct])["x"].reshape(n, 3), f"{mname} Direct")
            assert not d.overrun()
        return check
    return build


REG.case("factor-ani1")(factor_case("ani1", ani1()))
REG.case("factor-grid20-reversed")(factor_case("grid20_reversed", grid_5pt_reversed(20)))


# ---- triangular solves: every plan

def trs_case(mname, mat, bricks):
    n, rp, ci, v = mat

    def build(oracle, batch):
        f = ilu_util.oracle_par_ilu(oracle, n, rp, ci, v, 1)      # one L and one U of the matrix's pattern
        nrhs = 2
        b = rhs(n, nrhs, 95)
        idx = {}
        for upper, key in ((0, "L"), (1, "U")):
            for unit in (0, 1):
                arrays, params = ref_exec.csr_arrays(n, n, *f[key])
                arrays.update(b=b.reshape(-1), x=np.zeros(n * nrhs))
                idx[(upper, unit)] = batch.add("trs", arrays, upper=upper, unit_diagonal=unit, b_rows=n, b_cols=nrhs,
                                               x_rows=n, x_cols=nrhs, **params)

        def check(results, gk):
            s = stream_ptr()
            nb = gk.trs_workspace_bytes()
            for upper, key in ((0, "L"), (1, "U")):
                frp, fci, fv = (dev(a) for a in f[key])
                plan = solvers.TrsPlan(gk, n, frp, fci, fv, not upper)
                bk = solvers.TrsBricks(gk, n, frp, fci, fv, not upper) if bricks else None
                for unit in (0, 1):
                    want = ok(results[idx[(upper, unit)]])["x"].reshape(n, nrhs)
                    what = f"{mname} {'upper' if upper else 'lower'} unit={unit}"
                    x = torch.full((n, nrhs), float("nan"), dtype=torch.float64, device="cuda:0")
                    ws = torch.zeros(nb, dtype=torch.uint8, device="cuda:0")
                    solve = gk.upper_trs_solve_f64_i32 if upper else gk.lower_trs_solve_f64_i32
                    solve(s, n, nrhs, frp, fci, fv, unit, dev(b), nrhs, x, nrhs, ws, nb)
                    assert_bits(host(x), want, what + " sync-free")
                    x = torch.full((n, nrhs), float("nan"), dtype=torch.float64, device="cuda:0")
                    # the plan's solve: one workgroup up to 4096 rows, level-scheduled beyond
                    assert_bits(host(plan.solve(dev(b), x, bool(unit))), want,
                                what + (" single-workgroup" if n <= 4096 else " level-scheduled"))
                    assert not plan.overrun()
                    if bk is not None:
                        x = torch.full((n, nrhs), float("nan"), dtype=torch.float64, device="cuda:0")
                        assert_bits(host(bk.solve(dev(b), x, bool(unit))), want, what + " bricks")
                        assert not bk.overrun()
        return check
    return build


REG.case("trs-ani1")(trs_case("ani1", ani1(), False))
REG.case("trs-grid20")(trs_case("grid20", matgen.poisson_2d_5pt(20), False))
REG.case("trs-grid70x45-bricks")(trs_case("grid70x45", matgen.poisson_2d_5pt(70, 45), True))
REG.case("trs-grid70-levels")(trs_case("grid70", matgen.poisson_2d_5pt(70), False))


# ---- Jacobi: generate and apply

def jacobi_case(max_bs, adaptive):
    n, rp, ci, v = ani1()

    def build(oracle, batch):
        arrays, params = ref_exec.csr_arrays(n, n, rp, ci, v)
        nrhs = 3
        b = rhs(n, nrhs, 97)
        arrays.update(b=b.reshape(-1), x=np.zeros(n * nrhs))
        # max_block_stride 64: the storage scheme of a wave of 64 lanes, which the host executor takes as a parameter
        idx = batch.add("jacobi", arrays, op=0, max_block_size=max_bs, max_block_stride=64, adaptive=int(adaptive),
                        accuracy=0.1, b_rows=n, b_cols=nrhs, x_rows=n, x_cols=nrhs, **params)

        def check(results, gk):
            r = ok(results[idx])
            p = solvers.jacobi_generate(gk, n, dev(rp), dev(ci), dev(v), max_bs, nrhs,
                                        storage_optimization=solvers.AUTODETECT if adaptive else None)
            what = f"jacobi max_block_size={max_bs} adaptive={adaptive}"
            if max_bs == 1:
                assert_bits(host(p.keep[0]), r["blocks"], what + " inverted diagonal")
            else:
                nb = int(r["num_blocks"][0])
                assert p.num_blocks == nb, what
                assert_bits(host(p.block_ptrs)[:nb + 1], r["block_pointers"], what + " block pointers")
                prec = r["precisions"][:nb] if adaptive else []
                if adaptive:
                    assert_bits(host(p.block_precisions)[:nb], prec, what + " precisions")
                    assert_bits(host(p.conditioning)[:nb], r["conditioning"], what + " conditioning")
                got = host(p.blocks)
                assert got.size == r["blocks"].size, what
                live = jacobi_written(r["scheme"], r["block_pointers"], prec, got.size * 8)
                assert_bits(got.view(np.uint8)[live], r["blocks"].view(np.uint8)[live], what + " block storage")
            x = torch.full((n, nrhs), float("nan"), dtype=torch.float64, device="cuda:0")
            assert_bits(host(p.apply(dev(b), x)), r["x"].reshape(n, nrhs), what + " apply")
        return check
    return build


for _bs in (1, 4, 13, 32):
    for _ad in (False, True):
        if _bs == 1 and _ad:
            continue            # scalar Jacobi stores no blocks to reduce
        REG.case(f"jacobi-{_bs}-{'adaptive' if _ad else 'plain'}")(jacobi_case(_bs, _ad))


# ---- conversions and Csr operations on one irregular 500-row matrix

def conversions_case(oracle, batch):
    rng = np.random.default_rng(99)
    counts = np.minimum(rng.geometric(0.15, 500) - 1, 200)
    counts[33:41] = 0
    m, n, rp, ci, v = rows_csr(500, 500, counts, 98, sort=False)
    v[::11] = 0.0
    arrays, params = ref_exec.csr_arrays(m, n, rp, ci, v)
    conv = {f: batch.add("convert", arrays, fmt=code, **params)
            for f, code in (("ell", ELL), ("sellp", SELLP), ("coo", COO), ("hybrid", HYBRID))}
    conv["fbcsr"] = batch.add("convert", arrays, fmt=FBCSR, bs=2, **params)
    ops = {op: batch.add("csr_op", arrays, op=op, **params) for op in range(4)}
    # matrix data: values that add exactly, since the reference's std::sort leaves equal entries in any order
    cnt = 4000
    ri = rng.integers(0, 60, cnt).astype(np.int32)
    cj = rng.integers(0, 50, cnt).astype(np.int32)
    mv = rng.integers(-32, 33, cnt) / 8.0
    md = {op: batch.add("mdata", dict(ri=ri, ci=cj, v=mv), m=60, n=50, op=op) for op in range(3)}

    def check(results, gk):
        s = stream_ptr()
        A = formats.Csr.from_host(gk, m, n, rp, ci, v)
        e = A.to("ell")
        r = ok(results[conv["ell"]])
        assert [e.k, e.stride] == list(r["ell_meta"])
        assert_bits(host(e.col_idxs)[:e.k * e.stride], r["ell_ci"], "ell col_idxs")
        assert_bits(host(e.vals)[:e.k * e.stride], r["ell_v"], "ell values")
        sp = A.to("sellp")
        r = ok(results[conv["sellp"]])
        nsl = (m + 63) // 64
        assert_bits(host(sp.sets), r["sellp_set"], "sellp slice_sets")
        assert_bits(host(sp.lens)[:nsl], r["sellp_len"], "sellp slice_lengths")
        total = int(r["sellp_set"][-1]) * 64
        pos = np.arange(total)
        live = np.searchsorted(r["sellp_set"][1:], pos // 64, side="right") * 64 + pos % 64 < m
        assert_bits(host(sp.col_idxs)[:total][live], r["sellp_ci"][live], "sellp col_idxs")
        assert_bits(host(sp.vals)[:total][live], r["sellp_v"][live], "sellp values")
        r = ok(results[conv["coo"]])
        assert_bits(host(A.row_idxs())[:A.nnz], r["coo_ri"], "coo row_idxs")
        h = A.to("hybrid")
        r = ok(results[conv["hybrid"]])
        assert [h.ell_lim, m] == list(r["ell_meta"])
        assert_bits(host(h.ell_cols)[:h.ell_lim * m], r["ell_ci"], "hybrid ell col_idxs")
        assert_bits(host(h.ell_vals)[:h.ell_lim * m], r["ell_v"], "hybrid ell values")
        assert h.coo_nnz == r["coo_v"].size
        assert_bits(host(h.coo_rows)[:h.coo_nnz], r["coo_ri"], "hybrid coo row_idxs")
        assert_bits(host(h.coo_cols)[:h.coo_nnz], r["coo_ci"], "hybrid coo col_idxs")
        assert_bits(host(h.coo_vals)[:h.coo_nnz], r["coo_v"], "hybrid coo values")
        fb = A.to("fbcsr", block_size=2)
        r = ok(results[conv["fbcsr"]])
        assert_bits(host(fb.row_ptrs), r["fb_rp"], "fbcsr row_ptrs")
        assert_bits(host(fb.col_idxs), r["fb_ci"], "fbcsr col_idxs")
        assert_bits(host(fb.vals), r["fb_v"], "fbcsr values")
        back = fb.to_csr()
        for g, k in zip((back.row_ptrs, back.col_idxs, back.vals), ("back_rp", "back_ci", "back_v")):
            assert_bits(host(g), r[k], "fbcsr -> csr " + k)
        # transpose, sort, is_sorted, extract_diagonal
        tb = gk.csr_transpose_workspace_bytes(max(m, n))
        tws = torch.empty(tb, dtype=torch.uint8, device="cuda:0")
        trp = torch.zeros(n + 1, dtype=torch.int32, device="cuda:0")
        tc, tv = torch.zeros_like(A.col_idxs), torch.zeros_like(A.vals)
        gk.csr_transpose_f64_i32(s, m, n, A.nnz, A.row_ptrs, A.col_idxs, A.vals, trp, tc, tv, tws, tb)
        r = ok(results[ops[0]])
        assert_bits(host(trp), r["rp"], "transpose row_ptrs")
        assert_bits(host(tc), r["ci"], "transpose col_idxs")
        assert_bits(host(tv), r["v"], "transpose values")
        flag = ctypes.c_int(-1)
        ws8 = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
        gk.csr_is_sorted_by_column_index_i32(s, m, A.row_ptrs, A.col_idxs, ws8, 8, ctypes.addressof(flag))
        assert flag.value == int(ok(results[ops[2]])["sorted"][0]) == 0
        sc, sv = A.col_idxs.clone(), A.vals.clone()
        gk.csr_sort_by_column_index_f64_i32(s, m, A.row_ptrs, sc, sv)
        r = ok(results[ops[1]])
        assert_bits(host(sc), r["ci"], "sort col_idxs")
        assert_bits(host(sv), r["v"], "sort values")          # the rows hold no column twice: one sorted order
        diag = torch.zeros(m, dtype=torch.float64, device="cuda:0")
        gk.csr_extract_diagonal_f64_i32(s, m, A.row_ptrs, A.col_idxs, A.vals, diag)
        assert_bits(host(diag), ok(results[ops[3]])["diag"], "extract_diagonal")
        # device_matrix_data
        t = (ri, cj, mv)
        srt = gpu_sort(gk, t)
        r = ok(results[md[2]])
        assert_bits(srt[0], r["ri"], "sort_row_major rows")
        assert_bits(srt[1], r["ci"], "sort_row_major cols")
        key = lambda a, b_, c: sorted(zip(a.tolist(), b_.tolist(), [float(x).hex() for x in c]))
        assert key(*srt) == key(r["ri"], r["ci"], r["v"]), "sort_row_major values"
        got = gpu_compact(gk, "matrix_data_sum_duplicates_f64_i32", srt)
        r = ok(results[md[0]])
        for g, k in zip(got, ("ri", "ci", "v")):
            assert_bits(g, r[k], "sum_duplicates " + k)
        got = gpu_compact(gk, "matrix_data_remove_zeros_f64_i32", t)
        r = ok(results[md[1]])
        for g, k in zip(got, ("ri", "ci", "v")):
            assert_bits(g, r[k], "remove_zeros " + k)
    return check


REG.case("conversions")(conversions_case)


@pytest.mark.parametrize("name", REG.names())
def test_kernel_equals_reference(prepared, gk, name):
    run_case(prepared, name, gk)


if __name__ == "__main__":      # record the driver's results for the cases above
    import oracle_lib
    REG.queue(oracle_lib.load())[0].record(RECORDING)
    print(f"{RECORDING}: {os.path.getsize(RECORDING)} bytes")
