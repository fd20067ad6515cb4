"""GPU parity of the ParIC chain (C ABI) against the oracle: setup kernels
bit-exact, the asynchronous sweeps converge to the oracle's sequential sweep
(= IC(0)), and Ic (L then L^T solve) preconditions CG."""
import json
import os

import numpy as np
import pytest
import torch

import ilu_util
import matgen
from gkomi import solvers
from gpu_util import dev, host, stream_ptr
from test_oracle_par_ic import G, TOL, sparse

pytestmark = pytest.mark.gpu


def test_known_answers(gk):
    n, rp, ci, v = sparse(G["mtx_l_system"])
    rpd, cid = dev(rp), dev(ci)
    vd = dev(v)
    gk.par_ic_init_factor_f64_i32(stream_ptr(), n, rpd, cid, vd)
    assert matgen.rel_err(ilu_util.csr_to_dense(n, n, rp, ci, host(vd)), G["mtx_l_init_expect"]) <= TOL
    for A, L in ((G["identity"], G["identity"]), (G["banded"], G["banded_l_expect"]),
                 (G["mtx_system"], G["mtx_l_it_expect"])):
        n, rp, ci, v = sparse(A)
        f = ilu_util.gpu_par_ic(gk, torch, n, dev(rp), dev(ci), dev(v), iterations=20)
        Lg = ilu_util.csr_to_dense(n, n, *(host(t) for t in f["L"]))
        assert matgen.rel_err(Lg, L) <= 10 * TOL
        Lt = ilu_util.csr_to_dense(n, n, *(host(t) for t in f["Lt"]))
        assert np.array_equal(Lt, Lg.T)


def perturbed_grid(grid):
    n, rp, ci, v = matgen.poisson_2d_5pt(grid)
    # drop a few diagonal entries' storage? no: IC needs an SPD matrix; make it less regular instead
    v = v * (1.0 + 0.1 * np.cos(np.arange(len(v))))
    v = 0.5 * (v + v[np.lexsort((np.repeat(np.arange(n), np.diff(rp)), ci))])  # symmetrise (pattern is symmetric)
    return n, rp, ci, v


@pytest.mark.parametrize("grid", [7, 40])
def test_setup_bitexact_and_sweeps_converge_to_ic0(gk, oracle, grid):
    n, rp, ci, v = perturbed_grid(grid)
    e = ilu_util.oracle_par_ic(oracle, n, rp, ci, v)
    lrp = np.zeros(n + 1, np.int32)
    oracle.ref_initialize_row_ptrs_l(n, rp, ci, lrp)
    s = stream_ptr()
    lrpd = torch.zeros(n + 1, dtype=torch.int32, device="cuda:0")
    sb = gk.prefix_sum_workspace_bytes(n + 1)
    sws = torch.empty(max(sb, 8), dtype=torch.uint8, device="cuda:0")
    gk.factorization_initialize_row_ptrs_l_i32(s, n, dev(rp), dev(ci), lrpd, sws, sb)
    assert np.array_equal(host(lrpd), lrp)
    for diag_sqrt in (0, 1):
        lc, lv = np.zeros(lrp[-1], np.int32), np.zeros(lrp[-1])
        oracle.ref_initialize_l(n, rp, ci, v, lrp, lc, lv, diag_sqrt)
        lcd = torch.zeros(int(lrp[-1]), dtype=torch.int32, device="cuda:0")
        lvd = torch.zeros(int(lrp[-1]), dtype=torch.float64, device="cuda:0")
        gk.factorization_initialize_l_f64_i32(s, n, dev(rp), dev(ci), dev(v), lrpd, lcd, lvd, diag_sqrt)
        assert np.array_equal(host(lcd), lc) and host(lvd).tobytes() == lv.tobytes()
    f = ilu_util.gpu_par_ic(gk, torch, n, dev(rp), dev(ci), dev(v), iterations=60)
    assert np.array_equal(host(f["L"][0]), e["L"][0]) and np.array_equal(host(f["L"][1]), e["L"][1])
    assert matgen.rel_err(host(f["L"][2]), e["L"][2]) <= 1e-12
    few = ilu_util.gpu_par_ic(gk, torch, n, dev(rp), dev(ci), dev(v), iterations=0)   # "Auto" = 10 sweeps
    assert matgen.rel_err(host(few["L"][2]), e["L"][2]) <= 5e-2


def test_par_ic_generate_of_the_python_layer_vs_oracle(gk, oracle):
    """solvers.par_ic_generate itself, not the restatement in ilu_util, on the perturbed 7 x 7 grid: patterns exactly,
    values to the bar of the test above, Lt the exact transpose of L"""
    n, rp, ci, v = perturbed_grid(7)
    e = ilu_util.oracle_par_ic(oracle, n, rp, ci, v)
    p = solvers.par_ic_generate(gk, n, dev(rp), dev(ci), dev(v), iterations=60)
    torch.cuda.synchronize()
    for got, key in ((p.L, "L"), (p.Lt, "Lt")):
        assert np.array_equal(host(got[0]), e[key][0]) and np.array_equal(host(got[1]), e[key][1]), key
        err = matgen.rel_err(host(got[2]), e[key][2])
        print(key, "rel_err", err)
        assert err <= 1e-12, key
    L = ilu_util.csr_to_dense(n, n, *(host(t) for t in p.L))
    Lt = ilu_util.csr_to_dense(n, n, *(host(t) for t in p.Lt))
    assert np.array_equal(Lt, L.T)
    assert np.array_equal(host(p.Lt[1]), e["Lt"][1])


def test_ic_preconditioned_cg(gk):
    n, rp, ci, v = matgen.poisson_2d_5pt(96)
    rpd, cid, vd = dev(rp), dev(ci), dev(v)
    f = ilu_util.gpu_par_ic(gk, torch, n, rpd.clone(), cid, vd, iterations=10)
    pc = solvers.ilu_from_factors(gk, n, f["L"], f["Lt"])     # Ic apply = L^-1 then L^-T
    b = torch.ones(n, dtype=torch.float64, device="cuda:0")
    plain = solvers.cg_solve(gk, n, rpd, cid, vd, b, max_iters=2000, reduction=1e-10)
    pre = solvers.cg_solve(gk, n, rpd, cid, vd, b, max_iters=2000, reduction=1e-10, precond=pc)
    assert plain["converged"] and pre["converged"] and pre["rel_residual"] <= 1e-10
    assert pre["iterations"] < 0.5 * plain["iterations"]
    assert matgen.rel_err(host(pre["x"]), host(plain["x"])) < 1e-7
