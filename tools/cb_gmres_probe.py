"""Times solver::CbGmres against solver::Gmres (unchanged by this feature: the anchor) on the 108^3 convection-diffusion
system at krylov_dim 30 and 100: iterations and wall time to 1e-10 and the time per iteration, per storage precision.
One warm-up solve, then the median of `--repeat` solves, each timed on the host around the blocking driver call.

    python tools/cb_gmres_probe.py [--grid 108] [--repeat 3] [--out profiles/cb_gmres_probe.md]

Then one Arnoldi step alone (gkomi_cb_gmres_finish_arnoldi_f64, its seven launches between two device events) at the
last step of a GMRES(30) cycle, on an orthonormal basis that the kernels built themselves and a fresh random vector:
the bytes the launches that do work must move (dots: the stored vectors once, next once per batch; update: the stored
vectors once, next read and written; finalize: next read and written, one vector stored), over the time, against a
device copy of 1 GiB timed the same way in the same run.  That is the rate of the whole step: its launch gaps and the
re-adding of the partials are in the time, so the dots kernel alone runs at least that fast.

Not measured here: ani4, and the dots kernel on its own (that needs a kernel trace)."""
import argparse
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
from gkomi import solvers


def timed(fn, repeat):
    fn()
    times, res = [], None
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times), res


def event_ms(fn, repeat, before=lambda: None):
    """median device time of fn over `repeat` runs, in ms"""
    out = []
    for _ in range(repeat + 1):
        before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out[1:])


def step_rates(gk, n, kd, repeat):
    """[(storage, passes, ms, bytes)] of the last Arnoldi step of a cycle, per storage precision"""
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    fresh = lambda: torch.randn((n, 1), dtype=torch.float64, device="cuda:0", generator=gen)
    s = torch.cuda.current_stream().cuda_stream
    batch = np.zeros(1, np.int64)
    rows = []
    for storage, sid in solvers.CB_GMRES_STORAGES.items():
        gk.cb_gmres_geometry(sid, np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(1, np.int64), batch)
        item = gk.cb_gmres_basis_bytes(n, 1, 0, sid) // n
        basis = torch.zeros(gk.cb_gmres_basis_bytes(n, 1, kd, sid), dtype=torch.uint8, device="cuda:0")
        scal = torch.ones((kd + 1, 1), dtype=torch.float64, device="cuda:0")
        hess = torch.zeros((kd + 1, kd), dtype=torch.float64, device="cuda:0")
        buf, an = torch.zeros((kd + 1, 1), dtype=torch.float64, device="cuda:0"), torch.zeros((3, 1), dtype=torch.float64, device="cuda:0")
        rn, rnc = torch.zeros(1, dtype=torch.float64, device="cuda:0"), torch.zeros((kd + 1, 1), dtype=torch.float64, device="cuda:0")
        fin, reorth = torch.zeros(1, dtype=torch.int64, device="cuda:0"), torch.zeros(1, dtype=torch.int64, device="cuda:0")
        stop = torch.zeros(1, dtype=torch.uint8, device="cuda:0")
        nws = gk.cb_gmres_step_workspace_bytes(1, kd)
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda:0")
        nxt = fresh()
        gk.cb_gmres_restart_f64(s, n, 1, kd, sid, fresh(), rn, rnc, an, basis, scal, nxt, fin, 0, ws, nws)
        step = lambda it: gk.cb_gmres_finish_arnoldi_f64(s, n, 1, kd, sid, nxt, basis, scal, hess[:, it:], kd, buf, an, it, stop,
                                                         reorth, ws, nws)
        for it in range(kd - 1):
            nxt.copy_(fresh())
            step(it)
        ms = event_ms(lambda: step(kd - 1), repeat, before=lambda: nxt.copy_(fresh()))
        passes = int(reorth.cpu()[0])
        sweep = kd * n * item * 2 + (-(-kd // int(batch[0])) + 2) * n * 8
        rows.append((storage, passes, ms, (1 + passes) * sweep + 2 * n * 8 + n * item))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=108)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cb_gmres_probe.md"))
    args = ap.parse_args()
    gk = gkomi.lib()
    n, rp, ci, v = matgen.at_like(args.grid, 0.5)
    b = np.cos(0.3 * np.arange(n))
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    rpd, cid, vd, bd = d(rp), d(ci), d(v), d(b)
    rows = []
    for kd in (30, 100):
        med, lo, hi, res = timed(lambda: solvers.gmres_solve(gk, n, rpd, cid, vd, bd, krylov_dim=kd, max_iters=5000,
                                                             reduction=1e-10), args.repeat)
        rows.append((kd, "Gmres (anchor)", res["iterations"], res["converged"], med, lo, hi, "-"))
        for storage in solvers.CB_GMRES_STORAGES:
            med, lo, hi, res = timed(lambda: solvers.cb_gmres_solve(gk, n, rpd, cid, vd, bd, krylov_dim=kd, storage=storage,
                                                                    max_iters=5000, reduction=1e-10), args.repeat)
            mb = gk.cb_gmres_basis_bytes(n, 1, kd, solvers.CB_GMRES_STORAGES[storage]) / 1e6
            rows.append((kd, f"CbGmres {storage}", res["iterations"], res["converged"], med, lo, hi, f"{mb:.0f}"))
    lines = [f"# CB-GMRES probe: {args.grid}^3 convection-diffusion (n = {n}, nnz = {len(ci)}), reduction 1e-10", "",
             f"`python tools/cb_gmres_probe.py --grid {args.grid} --repeat {args.repeat}` on {torch.cuda.get_device_name(0)}, "
             f"{gk.version().decode()}; median (min .. max) of {args.repeat} solves after one warm-up, host wall clock "
             "around the blocking call.", "",
             "| krylov_dim | solver | iterations | converged | ms per solve | us per iteration | basis MB |",
             "|---|---|---|---|---|---|---|"]
    for kd, name, its, conv, med, lo, hi, mb in rows:
        lines.append(f"| {kd} | {name} | {its} | {conv} | {med * 1e3:.1f} ({lo * 1e3:.1f} .. {hi * 1e3:.1f}) | "
                     f"{med * 1e6 / max(its, 1):.1f} | {mb} |")
    x, y = torch.empty(1 << 27, dtype=torch.float64, device="cuda:0"), torch.empty(1 << 27, dtype=torch.float64, device="cuda:0")
    copy_gbs = 2 * (1 << 30) / event_ms(lambda: y.copy_(x), 10) / 1e6
    lines += ["", "## One Arnoldi step alone: finish_arnoldi at step 29 of GMRES(30), device events, median of 20", "",
              f"Device copy of 1 GiB in the same run: {copy_gbs:.0f} GB/s (read + write).", "",
              "| storage | re-orthogonalisation passes | us per step | MB the step must move | GB/s | of the copy rate |", "|---|---|---|---|---|---|"]
    for storage, passes, ms, nbytes in step_rates(gk, n, 30, 20):
        gbs = nbytes / ms / 1e6
        lines.append(f"| {storage} | {passes} | {ms * 1e3:.1f} | {nbytes / 1e6:.0f} | {gbs:.0f} | {gbs / copy_gbs:.2f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
