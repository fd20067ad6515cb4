"""GPU parity tests of the one-nonzero-per-lane layout of the nonzero-split CSR SpMV (csr_split_kernel): every lane
loads, gathers and multiplies single nonzeros, so the edges of that layout are checked bit-exact against the oracle
(reference/matrix/csr_kernels.cpp:75-128) for every tile size: stencils, odd nnz, nnz just past a tile boundary, rows
that cross the tile end by exactly the over-read, rows longer than the caller's hint, sparse-rows mode, alpha/beta,
int64 indices, and the dot epilogue of the fused CG iteration."""
import numpy as np
import pytest
import torch

import matgen
from gpu_util import DevCsr, csr_apply_srow, dev, host, make_srow
from test_csr_spmv_gpu import _oracle_apply

pytestmark = pytest.mark.gpu
SPLIT = 4
TILES = [1024, 1536, 2048, 3072]
NT = 2 << 8   # variant bit 2: nontemporal streams (the cold apply's instantiation)


def from_counts(counts, ncols, seed):
    """A CSR matrix with the given row lengths, sorted random columns and random values."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    rp = np.zeros(len(counts) + 1, np.int32)
    np.cumsum(counts, out=rp[1:])
    ci = np.concatenate([np.sort(rng.choice(ncols, size=int(k), replace=False)) for k in counts]).astype(np.int32)
    v = rng.standard_normal(int(rp[-1]))
    return rp, ci, v


def check(gk, oracle, nrows, ncols, rp, ci, v, tile, hint=None, seed=0):
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((ncols, 1))
    c0 = rng.standard_normal((nrows, 1))
    A = DevCsr(nrows, ncols, rp, ci, v)
    srow, _ = make_srow(gk, A, tile)
    expect = _oracle_apply(oracle, nrows, rp, ci, v, b)
    expect_adv = _oracle_apply(oracle, nrows, rp, ci, v, b, c0, -0.75, 1.5)
    for variant in (0, NT):
        got = host(csr_apply_srow(gk, A, dev(b), srow, tile, strategy=SPLIT | variant, hint=hint))
        assert np.array_equal(got, expect), variant
        got = host(csr_apply_srow(gk, A, dev(b), srow, tile, dev(c0), -0.75, 1.5, SPLIT | variant, hint=hint))
        assert np.array_equal(got, expect_adv), variant


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("stencil", ["5pt", "7pt"])
def test_stencils(gk, oracle, tile, stencil):
    n, rp, ci, v = matgen.poisson_2d_5pt(151, 97) if stencil == "5pt" else matgen.poisson_3d_7pt(23)
    check(gk, oracle, n, n, rp, ci, v, tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("extra", [1, 2, 3, 5])
def test_odd_nnz_and_nnz_just_past_a_tile(gk, oracle, tile, extra):
    # rows of 4 up to 3 tiles, then rows that leave nnz = 3 * tile + extra (odd for odd extra)
    counts = [4] * (3 * tile // 4) + [1] * extra
    rp, ci, v = from_counts(counts, 900, seed=extra)
    assert int(rp[-1]) == 3 * tile + extra
    check(gk, oracle, len(counts), 900, rp, ci, v, tile, seed=extra)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("length", [5, 8, 33, 65])
def test_rows_crossing_the_tile_end_by_the_over_read(gk, oracle, tile, length):
    # a row of `length` starts at tile - 1 and at 2 * tile - 1: it ends `length - 1` nonzeros behind the tile, exactly
    # the over-read for odd lengths (over = hint rounded down to even, at most 64)
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


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("hint", [3, 7])
def test_rows_longer_than_the_hint(gk, oracle, tile, hint):
    rp, ci, v = matgen.random_csr(2000, 700, 0, 90, seed=hint)
    check(gk, oracle, 2000, 700, rp, ci, v, tile, hint=hint, seed=hint)


@pytest.mark.parametrize("tile", TILES)
def test_sparse_rows_mode(gk, oracle, tile):
    # runs of empty rows: one tile starts far more than 2048 rows, so every tile hands its rows out by index
    counts = np.zeros(9000, np.int64)
    counts[::7] = 3
    counts[5000:5010] = 40
    counts[8999] = 1
    rp, ci, v = from_counts(counts, 500, seed=9)
    A = DevCsr(9000, 500, rp, ci, v)
    srow, _ = make_srow(gk, A, tile)
    assert host(srow)[0] < 0   # sparse-rows mode
    check(gk, oracle, 9000, 500, rp, ci, v, tile, seed=9)


@pytest.mark.parametrize("tile", [1536, 2048, 3072])
def test_int64(gk, oracle, tile):
    from gkomi import formats
    n, rp, ci, v = matgen.poisson_2d_5pt(131, 77)
    rp = rp.copy()
    b = np.random.default_rng(4).standard_normal((n, 1))
    expect = _oracle_apply(oracle, n, rp, ci, v, b)
    A = formats.Csr64.from_host(gk, n, n, rp, ci, v, split=True)
    got = host(A.apply(dev(b), torch.full((n, 1), float("nan"), dtype=torch.float64, device="cuda:0")))
    assert np.array_equal(got, expect)


def test_dot_epilogue_in_cg(gk, oracle):
    """The fused CG iteration runs the split kernel with its dot epilogue (one partial per tile): it converges like the
    row-cut path, to the oracle's residual, and the same bits on a second run."""
    from gkomi import formats, solvers
    n, rp, ci, v = matgen.poisson_2d_5pt(160, 137)
    A = formats.Csr.from_host(gk, n, n, rp, ci, v, split=False)
    S = formats.Csr.from_host(gk, n, n, rp, ci, v)
    b = np.sin(0.05 * np.arange(n)) + 0.5
    kw = dict(max_iters=3000, reduction=1e-10, fused=True)
    base = solvers.solve_op(gk, "cg", A, dev(b), **kw)
    res = solvers.solve_op(gk, "cg", S, dev(b), **kw)
    assert base["converged"] and res["converged"] and abs(res["iterations"] - base["iterations"]) <= 2
    assert matgen.rel_err(host(res["x"]), host(base["x"])) <= 1e-8
    r = b.copy().reshape(n, 1)
    oracle.ref_csr_advanced_spmv(n, 1, -1.0, rp, ci, v, host(res["x"]).reshape(n, 1), 1, 1.0, r, 1)
    assert np.linalg.norm(r) <= 1e-8 * np.linalg.norm(b)
    again = solvers.solve_op(gk, "cg", S, dev(b), **kw)
    assert again["iterations"] == res["iterations"] and host(again["x"]).tobytes() == host(res["x"]).tobytes()
