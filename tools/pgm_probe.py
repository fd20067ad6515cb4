"""What multigrid::Pgm costs on the device and what hierarchies it gives.

    python tools/pgm_probe.py [--repeat 5] [--small] [--out profiles/pgm_probe.md]

Matrices: the 5-point Poisson matrix of a 1000 x 1000 grid, the 7-point one of 108^3, and tests/golden/ani4.mtx
(--small: 200 x 200 and 24^3 in their place, for a quick look).

1. Generate, whole: gkomi.solvers.pgm (both calls of gkomi_pgm_generate_f64_i32, allocations included) in both modes,
   next to gkomi.solvers.fixed_coarsening on every second row -- the only coarsening the library had before.  Host
   clock around the blocking call, warmed once, median of --repeat runs with the smallest and largest next to it.
2. Generate, per step, through the kernel entry points on the weight matrix the library builds (compute_absolute,
   transpose, spgeam, extract_diagonal): device events around each call, warmed once, median of --repeat, next to the
   bytes the step must move at the least (what it reads once plus what it writes once).  The matching loop is run to the
   state the driver reaches; find_strongest_neighbor and match_edge are timed on the first round, where every row is
   unaggregated.
3. The hierarchy Multigrid builds with pgm_factory (max_levels 10, min_coarse_rows 64): rows and nonzeros per level,
   operator complexity = sum of nonzeros over levels / nonzeros of the finest.
4. Cg to a residual reduction of 1e-10 (at most 2000 iterations), preconditioned by one V-cycle (two Jacobi sweeps,
   relaxation 0.9, zero guess, Identity on the coarsest level) over Pgm in both modes and over FixedCoarsening on every
   second row, and by scalar Jacobi alone: iterations and host time around the blocking solve, generate not included."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "repo-8852-ginkgo_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np
import torch

import gkomi
import matgen
from gkomi import formats, solvers

SPLIT = 4


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host_timed(fn, repeat):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def event_timed(setup, fn, repeat):
    """setup() restores the inputs (not timed), fn() is the step"""
    out = []
    for k in range(repeat + 1):
        setup()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k:
            out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out), min(out), max(out)


def fmt(t, unit=""):
    return f"{t[0]:.1f}{unit} ({t[1]:.1f} .. {t[2]:.1f})"


def matrices(small):
    import multigrid_util as mu
    g2, g3 = (200, 24) if small else (1000, 108)
    yield f"5-point {g2} x {g2}", matgen.poisson_2d_5pt(g2)
    yield f"7-point {g3}^3", matgen.poisson_3d_7pt(g3)
    m = mu.read_mtx("ani4.mtx")
    yield "ani4", (m[0], m[2], m[3], m[4])


def steps(gk, n, rp, ci, v, repeat, say):
    s = torch.cuda.current_stream().cuda_stream
    nnz = int(v.numel())
    i32 = lambda k, fill=0: torch.full((k,), fill, dtype=torch.int32, device="cuda:0")
    absv = torch.empty_like(v)
    rows = []
    rows.append(("compute_absolute", event_timed(lambda: None, lambda: gk.csr_compute_absolute_f64_i32(s, nnz, v, absv), repeat), 16 * nnz))
    t = {}
    rows.append(("transpose", event_timed(lambda: None, lambda: t.update(m=solvers._transpose(gk, n, rp, ci, absv)), repeat), 2 * 12 * nnz + 8 * n))
    trp, tci, tv = t["m"]
    half = dev(np.array([0.5]))
    w = {}

    def spgeam():
        sb = gk.csr_spgeam_workspace_bytes(n)
        ws = torch.empty(sb + 8, dtype=torch.uint8, device="cuda:0")
        wrp = i32(n + 1)
        cnt = ctypes.c_int64(0)
        call = lambda cc, cv: gk.csr_spgeam_f64_i32(s, n, n, half, nnz, rp, ci, absv, half, n, n, nnz, trp, tci, tv, wrp, cc, cv,
                                                    ctypes.addressof(cnt), ws, sb)
        call(None, None)
        wci, wv = i32(cnt.value), torch.empty(cnt.value, dtype=torch.float64, device="cuda:0")
        call(wci, wv)
        w.update(rp=wrp, ci=wci, v=wv, nnz=cnt.value)
    rows.append(("spgeam (both calls)", event_timed(lambda: None, spgeam, repeat), 3 * 12 * nnz + 12 * n))
    diag = torch.empty(n, dtype=torch.float64, device="cuda:0")
    rows.append(("extract_diagonal", event_timed(lambda: None, lambda: gk.csr_extract_diagonal_f64_i32(s, n, w["rp"], w["ci"], w["v"], diag), repeat),
                 4 * w["nnz"] + 12 * n))
    agg, strongest, counter = i32(n, -1), i32(n, -1), i32(1)

    def fresh():
        agg.fill_(-1)
        strongest.fill_(-1)
        counter.zero_()
    find = lambda: gk.pgm_find_strongest_neighbor_f64_i32(s, n, w["nnz"], w["rp"], w["ci"], w["v"], diag, agg, strongest, counter, 4)
    rows.append(("find_strongest_neighbor, round 1", event_timed(fresh, find, repeat), 12 * w["nnz"] + 4 * w["nnz"] + 16 * n))

    def found():
        fresh()
        find()
    rows.append(("match_edge, round 1", event_timed(found, lambda: gk.pgm_match_edge_i32(s, n, strongest, agg), repeat), 12 * n))
    # to the state the driver reaches after its rounds (defaults: 15 rounds, ratio 0.05)
    fresh()
    left = n
    for it in range(15):
        find()
        gk.pgm_match_edge_i32(s, n, strongest, agg)
        out = ctypes.c_int64(0)
        gk.pgm_count_unagg_i32(s, n, agg, ctypes.addressof(out), torch.zeros(8, dtype=torch.uint8, device="cuda:0"), 4)
        prev, left = left, out.value
        if left == 0 or left == prev or left < 0.05 * n:
            break
    say(f"matching: {it + 1} rounds, {left} of {n} rows left for assign_to_exist_agg")
    matched = agg.clone()
    ab = gk.pgm_assign_workspace_bytes(n)
    aws = torch.empty(ab + 8, dtype=torch.uint8, device="cuda:0")
    mid = i32(n)
    restore = lambda: agg.copy_(matched)
    rows.append(("assign_to_exist_agg, deterministic", event_timed(restore, lambda: gk.pgm_assign_to_exist_agg_f64_i32(
        s, n, w["nnz"], w["rp"], w["ci"], w["v"], diag, agg, mid, aws, ab), repeat), 16 * w["nnz"] + 16 * n))
    rounds = (n - 1).bit_length()
    rows.append((f"assign_to_exist_agg, default ({rounds} jumping rounds)", event_timed(restore, lambda: gk.pgm_assign_to_exist_agg_f64_i32(
        s, n, w["nnz"], w["rp"], w["ci"], w["v"], diag, agg, None, aws, ab), repeat), 16 * w["nnz"] + 16 * n + rounds * 12 * n))
    assigned = agg.clone()
    rb = gk.pgm_renumber_workspace_bytes(n)
    rws = torch.empty(rb + 8, dtype=torch.uint8, device="cuda:0")
    num = ctypes.c_int64(0)
    rows.append(("renumber", event_timed(lambda: agg.copy_(assigned), lambda: gk.pgm_renumber_i32(s, n, agg, ctypes.addressof(num), rws, rb), repeat), 20 * n))
    sb = gk.pgm_sort_workspace_bytes(max(n, nnz))
    sws = torch.empty(sb + 8, dtype=torch.uint8, device="cuda:0")
    r_rows, r_cols = i32(n), i32(n)

    def pairs():
        r_rows.copy_(agg)
        r_cols.copy_(torch.arange(n, dtype=torch.int32, device="cuda:0"))
    rows.append(("sort_agg (64 key bits)", event_timed(pairs, lambda: gk.pgm_sort_agg_i32(s, n, r_rows, r_cols, sws, sb), repeat), 16 * n))
    c_rows, c_cols, c_vals = i32(nnz), i32(nnz), torch.empty_like(v)
    rows.append(("map_row + map_col", event_timed(lambda: None, lambda: (gk.pgm_map_row_i32(s, n, rp, agg, c_rows),
                                                                         gk.pgm_map_col_i32(s, nnz, ci, agg, c_cols)), repeat), 16 * nnz + 8 * n))
    mapped = (c_rows.clone(), c_cols.clone())

    def unsorted():
        c_rows.copy_(mapped[0])
        c_cols.copy_(mapped[1])
        c_vals.copy_(v)
    rows.append(("sort_row_major (64 key bits)", event_timed(unsorted, lambda: gk.pgm_sort_row_major_f64_i32(s, nnz, c_rows, c_cols, c_vals, sws, sb), repeat),
                 2 * 16 * nnz))
    cb = gk.pgm_coarse_coo_workspace_bytes(nnz)
    cws = torch.empty(cb + 8, dtype=torch.uint8, device="cuda:0")
    cnnz = ctypes.c_int64(0)
    rows.append(("count_unrepeated_nnz", event_timed(lambda: None, lambda: gk.pgm_count_unrepeated_nnz_i32(
        s, nnz, c_rows, c_cols, ctypes.addressof(cnnz), cws, cb), repeat), 8 * nnz))
    o_rows, o_cols, o_vals = i32(cnnz.value), i32(cnnz.value), torch.empty(cnnz.value, dtype=torch.float64, device="cuda:0")
    rows.append(("compute_coarse_coo", event_timed(lambda: None, lambda: gk.pgm_compute_coarse_coo_f64_i32(
        s, nnz, c_rows, c_cols, c_vals, cnnz.value, o_rows, o_cols, o_vals, cws, cb), repeat), 16 * nnz + 16 * cnnz.value))
    say("")
    say("| step | us: median (min .. max) | bytes it must move | GB/s at the median |")
    say("|---|---|---|---|")
    for name, t, nbytes in rows:
        say(f"| {name} | {fmt(t)} | {nbytes} | {nbytes / t[0] / 1e3:.0f} |")
    say("")


def hierarchy(gk, A, level_factory):
    jac = lambda a: solvers.jacobi_generate(gk, a.nrows, a.row_ptrs, a.col_idxs, a.vals, max_block_size=1)
    return solvers.Multigrid(gk, A, [level_factory], pre_smoother=[jac], smoother_iters=2, max_levels=10, min_coarse_rows=64,
                             default_initial_guess="zero", max_iters=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gk = gkomi.lib()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say("# Pgm on the device: generate time, hierarchies, Cg with a Pgm V-cycle")
    say("")
    say(f"`python tools/pgm_probe.py --repeat {args.repeat}{' --small' if args.small else ''}` on {torch.cuda.get_device_name(0)}; "
        "method in the tool's docstring.")
    for name, (n, rp, ci, v) in matrices(args.small):
        rpd, cid, vd = dev(rp.astype(np.int32)), dev(ci.astype(np.int32)), dev(v.astype(np.float64))
        nnz = int(vd.numel())
        say("")
        say(f"## {name}: {n} rows, {nnz} nonzeros")
        say("")
        say("| generate | ms: median (min .. max) | coarse rows | coarse nonzeros |")
        say("|---|---|---|---|")
        kinds = {"Pgm, default": lambda: solvers.pgm(gk, n, rpd, cid, vd, strategy=SPLIT),
                 "Pgm, deterministic": lambda: solvers.pgm(gk, n, rpd, cid, vd, deterministic=True, strategy=SPLIT),
                 "FixedCoarsening, every second row": lambda: solvers.fixed_coarsening(
                     gk, n, rpd, cid, vd, torch.arange(0, n, 2, dtype=torch.int32, device="cuda:0"), strategy=SPLIT)}
        for kind, make in kinds.items():
            t = host_timed(make, args.repeat)
            lvl = make()
            say(f"| {kind} | {fmt(t)} | {lvl.get_coarse_op().nrows} | {lvl.get_coarse_op().nnz} |")
        say("")
        steps(gk, n, rpd, cid, vd, args.repeat, say)
        A = formats.Csr(gk, n, n, rpd, cid, vd, SPLIT)
        b = torch.ones(n, dtype=torch.float64, device="cuda:0")
        factories = {"Pgm, default": solvers.pgm_factory(gk), "Pgm, deterministic": solvers.pgm_factory(gk, deterministic=True),
                     "FixedCoarsening, every second row": solvers.fixed_coarsening_factory(
                         gk, lambda a: torch.arange(0, a.nrows, 2, dtype=torch.int32, device="cuda:0"))}
        say("| preconditioner of Cg | levels: rows (nonzeros) | operator complexity | iterations | converged | solve ms |")
        say("|---|---|---|---|---|---|")
        for kind, factory in factories.items():
            mg = hierarchy(gk, A, factory)
            ops = [A] + [lvl.get_coarse_op() for lvl in mg.get_mg_level_list()]
            t0 = time.perf_counter()
            out = solvers.cg_solve(gk, n, rpd, cid, vd, b, max_iters=2000, reduction=1e-10, precond=mg)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            say(f"| V-cycle over {kind} | {' -> '.join(f'{o.nrows} ({o.nnz})' for o in ops)} | {sum(o.nnz for o in ops) / nnz:.2f} | "
                f"{out['iterations']} | {'yes' if out['converged'] else 'no'} | {ms:.1f} |")
        jac = solvers.jacobi_generate(gk, n, rpd, cid, vd, max_block_size=1)
        for kind, pre in (("scalar Jacobi", jac), ("none", None)):
            t0 = time.perf_counter()
            out = solvers.cg_solve(gk, n, rpd, cid, vd, b, max_iters=2000, reduction=1e-10, precond=pre)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            say(f"| {kind} | - | 1.00 | {out['iterations']} | {'yes' if out['converged'] else 'no'} | {ms:.1f} |")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
