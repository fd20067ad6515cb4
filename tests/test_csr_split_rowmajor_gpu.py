"""The row-major lane order of the nonzero-split CSR SpMV (csr_split_kernel<..., RowMajor>): every wave transposes its
own segment of the tile through LDS so that lane l of gather instruction j holds nonzero l*s + j (s = the row length
the caller's hint promises) -- neighbouring lanes gather neighbouring entries of b.  The products land in the slots
they always had, so every case is checked bit for bit against the oracle (reference/matrix/csr_kernels.cpp:75-128), with
the order forced (variant bit 4), forbidden (bit 8) and left to the launcher's rule (odd strides at tiles up to 1536):
stencils, constant row lengths (odd and even, dividing and not dividing the segment), 1 % shorter rows (drift of the
rows against the stride), the clamped last tile, a row crossing into the over-read, rows longer than the hint, int64
indices and the dot epilogue in fused CG.  The launcher's rule itself (gkomi_diag_csr_split_row_stride) needs no GPU."""
import numpy as np
import pytest
import torch

import matgen
from gpu_util import DevCsr, csr_apply_srow, dev, host, make_srow, stream_ptr
from test_csr_spmv_gpu import _oracle_apply

gpu = pytest.mark.gpu
SPLIT = 4
TILES = [1024, 1536, 2048, 3072]
NT = 2 << 8          # variant bit 2: nontemporal streams (the cold apply's instantiation)
ROWMAJOR = 4 << 8    # variant bit 4: row-major lane order whatever the row statistics say
LANEORDER = 8 << 8   # variant bit 8: never
ORDERS = (ROWMAJOR, LANEORDER, 0)


def from_counts(counts, ncols, seed):
    """A CSR matrix with the given row lengths, sorted random columns and random values."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    rp = np.zeros(len(counts) + 1, np.int32)
    np.cumsum(counts, out=rp[1:])
    ci = np.concatenate([np.sort(rng.choice(ncols, size=int(k), replace=False)) for k in counts]).astype(np.int32)
    v = rng.standard_normal(int(rp[-1]))
    return rp, ci, v


def check(gk, oracle, nrows, ncols, rp, ci, v, tile, hint=None, seed=0, orders=ORDERS):
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((ncols, 1))
    c0 = rng.standard_normal((nrows, 1))
    A = DevCsr(nrows, ncols, rp, ci, v)
    srow, _ = make_srow(gk, A, tile)
    expect = _oracle_apply(oracle, nrows, rp, ci, v, b)
    expect_adv = _oracle_apply(oracle, nrows, rp, ci, v, b, c0, -0.75, 1.5)
    for order in orders:
        for variant in (0, NT):
            got = host(csr_apply_srow(gk, A, dev(b), srow, tile, strategy=SPLIT | variant | order, hint=hint))
            assert np.array_equal(got, expect), (order >> 8, variant >> 8)
            got = host(csr_apply_srow(gk, A, dev(b), srow, tile, dev(c0), -0.75, 1.5, SPLIT | variant | order, hint=hint))
            assert np.array_equal(got, expect_adv), (order >> 8, variant >> 8)
    # the automatic strategy (what Csr::apply passes)
    assert np.array_equal(host(csr_apply_srow(gk, A, dev(b), srow, tile, hint=hint)), expect)


# ---- the launcher's rule (host code only) ---------------------------------------------------------------------------

def stride(gk, nrows, nnz, nrhs, hint, tile, variant=0):
    return int(gk.diag_csr_split_row_stride(nrows, nnz, nrhs, hint, tile, variant))


def rule(nrows, nnz, nrhs, hint, tile):
    """the launcher's rule as include/gkomi.h states it"""
    taken = nrhs == 1 and 2 <= hint <= tile // 256 and hint % 2 == 1 and tile <= 1536 and 64 * nnz >= 63 * hint * nrows
    return hint if taken else 0


def test_rule_takes_regular_rows_only(gk):
    # P2 (1000^2 5-pt) at the tile of record; the 256^3 7-pt matrix neither at its tile of 3072 (the large tiles keep the
    # lane order) nor at 1536 (7 > S = 6), but forced
    assert stride(gk, 1000000, 4996000, 1, 5, 1536) == 5
    g = 256
    assert stride(gk, g ** 3, 7 * g ** 3 - 6 * g * g, 1, 7, 3072) == 0
    assert stride(gk, g ** 3, 7 * g ** 3 - 6 * g * g, 1, 7, 1536) == 0
    assert stride(gk, g ** 3, 7 * g ** 3 - 6 * g * g, 1, 7, 3072, 4) == 7
    # no hint, rows of one entry, several right-hand sides
    assert stride(gk, 1000, 5000, 1, -1, 1536) == 0
    assert stride(gk, 1000, 1000, 1, 1, 1536) == 0
    assert stride(gk, 1000, 5000, 2, 5, 1536) == 0
    # odd strides within the sweeps of the tiles up to 1536, nothing else
    taken = {(tile, hint) for tile in TILES for hint in range(0, 14) if stride(gk, 1000, 1000 * hint, 1, hint, tile) != 0}
    assert taken == {(1024, 3), (1536, 3), (1536, 5)}
    for tile in TILES:
        for hint in range(0, 14):
            assert stride(gk, 1000, 1000 * hint, 1, hint, tile) == rule(1000, 1000 * hint, 1, hint, tile)


def test_rule_threshold_is_63_64ths(gk):
    # 64 * nnz >= 63 * hint * nrows, on both sides of it
    nrows, hint = 6400, 5
    full = hint * nrows
    edge = (63 * full + 63) // 64
    assert 64 * edge >= 63 * full > 64 * (edge - 1)
    assert stride(gk, nrows, full, 1, hint, 1536) == hint
    assert stride(gk, nrows, edge, 1, hint, 1536) == hint
    assert stride(gk, nrows, edge - 1, 1, hint, 1536) == 0


def test_rule_forced_and_forbidden(gk):
    force, forbid = 4, 8
    assert stride(gk, 1000, 5000, 1, 5, 1536, forbid) == 0
    assert stride(gk, 1000, 5000, 1, 5, 1536, force | forbid) == 0
    assert stride(gk, 1000, 3000, 1, 5, 1536, force) == 5     # irregular rows
    assert stride(gk, 1000, 5000, 3, 5, 1536, force) == 5     # several columns: one launch each
    assert stride(gk, 1000, 7000, 1, 7, 1536, force) == 6     # 1 <= s <= S: clamped
    assert stride(gk, 1000, 7000, 1, -1, 1536, force) == 1    # unknown rows: s = 1 is today's order


# ---- bits -----------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("stencil", ["5pt", "7pt"])
def test_stencils(gk, oracle, tile, stencil):
    # 5-pt: 0.7 % of the nonzeros of full rows are missing at the boundary, the rule takes the row-major order at tile
    # 1536 (5 > S at 1024; the larger tiles keep the lane order).  7-pt on 23^3: 3.7 % are missing, more than the 1/64
    # the rule allows -- it runs row-major forced only (s = 7 where 7 <= S: tile 2048 and 3072, clamped to S elsewhere)
    n, rp, ci, v = matgen.poisson_2d_5pt(151, 97) if stencil == "5pt" else matgen.poisson_3d_7pt(23)
    hint = 5 if stencil == "5pt" else 7
    assert stride(gk, n, int(rp[-1]), 1, hint, tile) == (5 if stencil == "5pt" and tile == 1536 else 0)
    assert stride(gk, n, int(rp[-1]), 1, hint, tile, 4) == min(hint, tile // 256)
    check(gk, oracle, n, n, rp, ci, v, tile, hint=hint)


@gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("length", [2, 3, 4, 5, 6, 8, 12])
@pytest.mark.parametrize("short", [False, True], ids=["constant", "one_percent_shorter"])
def test_row_lengths(gk, oracle, tile, length, short):
    # a little over three tiles; with every 97th row one entry shorter the rows drift against the stride
    nrows = 3 * tile // length + 50
    counts = np.full(nrows, length, np.int64)
    if short:
        counts[13::97] -= 1
    rp, ci, v = from_counts(counts, 1100, seed=length)
    # about 1 % of the rows short of one entry of `length` is a deficit of at most 0.52 %, below the 1/64 the rule
    # allows: it takes the odd lengths that fit the sweeps of the tiles up to 1536; everything runs forced as well
    assert stride(gk, nrows, int(rp[-1]), 1, length, tile) == rule(nrows, int(rp[-1]), 1, length, tile)
    assert stride(gk, nrows, int(rp[-1]), 1, length, tile, 4) == min(length, tile // 256)
    check(gk, oracle, nrows, 1100, rp, ci, v, tile, hint=length, seed=length)


@gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("short_of_64", [3, 4])
def test_shorter_rows_on_both_sides_of_the_threshold(gk, oracle, tile, short_of_64):
    # rows of 3, of every 64 rows 3 (deficit exactly 1/64: taken, at the tiles the rule takes at all) or 4 (1/48: left
    # alone) one entry shorter
    nrows = (3 * tile // 3 + 128) // 64 * 64
    counts = np.full(nrows, 3, np.int64)
    counts.reshape(-1, 64)[:, 5:5 + short_of_64] -= 1
    rp, ci, v = from_counts(counts, 1100, seed=short_of_64)
    assert 64 * int(rp[-1]) - 63 * 3 * nrows == (0 if short_of_64 == 3 else -nrows)
    assert stride(gk, nrows, int(rp[-1]), 1, 3, tile) == (3 if short_of_64 == 3 and tile <= 1536 else 0)
    check(gk, oracle, nrows, 1100, rp, ci, v, tile, hint=3, seed=short_of_64)


@gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("extra", [1, 2, 3, 5])
def test_clamped_last_tile(gk, oracle, tile, extra):
    # nnz = 3 * tile + extra: the last tile's loads clamp to nnz - 1 under the permutation
    counts = [4] * (3 * tile // 4) + [1] * extra
    rp, ci, v = from_counts(counts, 900, seed=extra)
    assert int(rp[-1]) == 3 * tile + extra
    check(gk, oracle, len(counts), 900, rp, ci, v, tile, hint=4, seed=extra)


@gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("length", [4, 5, 8])
def test_row_crossing_into_the_over_read(gk, oracle, tile, length):
    # a row of `length` starts at tile - 1 and at 2 * tile - 1 and ends in the nonzeros read behind the tile
    fill = tile - 1
    counts = []
    for _ in range(3):
        counts += [3] * (fill // 3) + [fill % 3] * (fill % 3 > 0) + [length]
        fill = tile - 1 - (length - 1)
    counts += [2] * 40
    rp, ci, v = from_counts(counts, 1200, seed=length)
    starts = np.asarray(rp[:-1])
    assert np.any(starts == tile - 1) and np.any(starts == 2 * tile - 1)
    check(gk, oracle, len(counts), 1200, rp, ci, v, tile, hint=length, seed=length)


@gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("hint", [3, 7])
def test_rows_longer_than_the_hint(gk, oracle, tile, hint):
    # rows of up to 90 entries behind a hint of 3 or 7: the finish-from-memory loops, row-major forced
    rp, ci, v = matgen.random_csr(2000, 700, 0, 90, seed=hint)
    check(gk, oracle, 2000, 700, rp, ci, v, tile, hint=hint, seed=hint, orders=(ROWMAJOR, LANEORDER))


@gpu
@pytest.mark.parametrize("tile", [1536, 2048, 3072])
@pytest.mark.parametrize("stencil", ["5pt", "7pt"])
def test_int64(gk, oracle, tile, stencil):
    n, rp, ci, v = matgen.poisson_2d_5pt(131, 77) if stencil == "5pt" else matgen.poisson_3d_7pt(21)
    hint = 5 if stencil == "5pt" else 7
    nnz = int(rp[-1])
    rng = np.random.default_rng(4)
    b, c0 = rng.standard_normal((n, 1)), rng.standard_normal((n, 1))
    expect = _oracle_apply(oracle, n, rp, ci, v, b)
    expect_adv = _oracle_apply(oracle, n, rp, ci, v, b, c0, 1.25, -0.5)
    rpd, cid, vd = dev(rp.astype(np.int64)), dev(ci.astype(np.int64)), dev(v)
    ne = int(gk.csr_srow_entries(nnz, tile))
    srow = torch.zeros(ne, dtype=torch.int64, device="cuda:0")
    gk.csr_make_srow_i64(stream_ptr(), n, nnz, rpd, tile, srow, ne)
    al, be = dev(np.array([1.25])), dev(np.array([-0.5]))
    for order in ORDERS:
        for streaming in (0, 1 << 24):   # GKOMI_CSR_STREAMING: the nontemporal instantiation
            c = torch.full((n, 1), float("nan"), dtype=torch.float64, device="cuda:0")
            gk.csr_spmv_srow_f64_i64(stream_ptr(), n, n, 1, nnz, rpd, cid, vd, dev(b), 1, c, 1, None, None,
                                     SPLIT | order | streaming, hint, srow, tile)
            assert np.array_equal(host(c), expect), (order >> 8, streaming)
            c = dev(c0)
            gk.csr_spmv_srow_f64_i64(stream_ptr(), n, n, 1, nnz, rpd, cid, vd, dev(b), 1, c, 1, al, be,
                                     SPLIT | order | streaming, hint, srow, tile)
            assert np.array_equal(host(c), expect_adv), (order >> 8, streaming)


@gpu
def test_dot_epilogue_in_cg(gk, oracle):
    """Fused CG runs the split kernel with its dot epilogue: the same iterations and the same bytes of x with the
    row-major order forced, forbidden and chosen by the rule (hint 5, tile 1536: taken)."""
    from gkomi import formats, solvers
    n, rp, ci, v = matgen.poisson_2d_5pt(160, 137)
    b = np.sin(0.05 * np.arange(n)) + 0.5
    kw = dict(max_iters=3000, reduction=1e-10, fused=True)
    res = {}
    for name, strategy in (("forbidden", SPLIT | LANEORDER), ("forced", SPLIT | ROWMAJOR), ("rule", 0)):
        A = formats.Csr.from_host(gk, n, n, rp, ci, v, strategy=strategy)
        res[name] = solvers.solve_op(gk, "cg", A, dev(b), **kw)
        assert res[name]["converged"]
    for name in ("forced", "rule"):
        assert res[name]["iterations"] == res["forbidden"]["iterations"]
        assert host(res[name]["x"]).tobytes() == host(res["forbidden"]["x"]).tobytes()
    r = b.copy().reshape(n, 1)
    oracle.ref_csr_advanced_spmv(n, 1, -1.0, rp, ci, v, host(res["forced"]["x"]).reshape(n, 1), 1, 1.0, r, 1)
    assert np.linalg.norm(r) <= 1e-8 * np.linalg.norm(b)
