"""Mixed-precision iterative refinement against double CG: time to ||b - A x|| / ||b|| <= 1e-10 on the 5-point 1000^2
system (P2) and on a 7-point 3-D grid too big for the single-launch CG (192^3 by default), and the time per iteration of
the fused float CG against the double three-launch CG, next to the byte model of csrc/mixed.hip.  Timings: HIP events
around synchronised work, the best of --reps runs after a warm-up.  Writes a markdown note (--out).

  python tools/mpir_probe.py --out profiles/mpir_probe.md [--n3 192] [--reps 3] [--iter-only]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "repo-8852-ginkgo_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gkomi  # noqa: E402
import gkomi.solvers as solvers  # noqa: E402
import matgen  # noqa: E402

gk = gkomi.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def timed(f, reps):
    f()  # warm-up: code objects, workspaces
    torch.cuda.synchronize()
    best, out = None, None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = f()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return best, out


def true_rel(n, rp, ci, v, b, x):
    y = torch.zeros(n, 1, dtype=torch.float64, device="cuda")
    gk.csr_spmv_f64_i32(stream(), n, n, 1, int(v.numel()), rp, ci, v, x.reshape(n, 1), 1, y, 1, None, None, 0, -1)
    return float(torch.linalg.norm(b.reshape(n, 1) - y) / torch.linalg.norm(b))


def per_iteration(n, rp, ci, v, b, iters, reps):
    """us per iteration at a fixed iteration count (reduction 0 never fires): double three-launch, fused float"""
    gk.cg_persistent_enable(0)
    t64, _ = timed(lambda: solvers.cg_solve(gk, n, rp, ci, v, b, max_iters=iters, reduction=0.0), reps)
    vf = v.float()
    bf = b.float()
    nb = gk.cg_fused_workspace_bytes_f32(n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    info = np.zeros(4)

    def f32():
        x = torch.zeros(n, dtype=torch.float32, device="cuda")
        gk.cg_solve_fused_f32_i32(stream(), n, int(v.numel()), rp, ci, vf, bf, x, iters, 0.0, 0, ws, nb, info)
        return int(info[0])

    t32, it32 = timed(f32, reps)
    gk.cg_persistent_enable(1)
    assert it32 == iters
    return t64 * 1e3 / iters, t32 * 1e3 / iters


def to_solution(name, n, rp, ci, v, b, reps, lines):
    goal = 1e-10
    rows = []
    for label, mode in (("double CG, three launches", 0), ("double CG, persistent where it applies", 1)):
        gk.cg_persistent_enable(mode)
        before = gk.cg_persistent_solves()
        ms, res = timed(lambda: solvers.cg_solve(gk, n, rp, ci, v, b, max_iters=20000, reduction=goal), reps)
        used = gk.cg_persistent_solves() > before
        rel = true_rel(n, rp, ci, v, b, res["x"])
        rows.append((label + (" (ran persistent)" if used else (" (not applicable)" if mode == 1 else "")), ms, res["iterations"],
                     "-", rel, res["converged"]))
    gk.cg_persistent_enable(1)
    for inner in (1e-1, 1e-2, 1e-3):
        ms, res = timed(lambda: solvers.ir_mixed(gk, n, rp, ci, v, b, max_iters=100, reduction=goal, inner_max_iters=5000,
                                                 inner_reduction=inner), reps)
        rel = true_rel(n, rp, ci, v, b, res["x"])
        rows.append((f"MPIR, inner reduction {inner:g}", ms, res["iterations"], f"{res['inner_iterations']} "
                     f"({res['inner_capped']} capped)", rel, res["converged"]))
    lines.append(f"\n### {name}: time to ||b - A x|| / ||b|| <= 1e-10\n")
    lines.append("| solver | ms | outer / CG iterations | inner iterations | true rel. residual | converged |")
    lines.append("|---|---:|---:|---:|---:|---|")
    for label, ms, it, inner, rel, conv in rows:
        lines.append(f"| {label} | {ms:.2f} | {it} | {inner} | {rel:.2e} | {conv} |")
    print("\n".join(lines[-len(rows) - 3:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n3", type=int, default=192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--iter-only", action="store_true", help="only the per-iteration timing on P2 (for a kernel trace)")
    a = ap.parse_args()
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    lines = ["# Mixed-precision IR against double CG (tools/mpir_probe.py)", ""]
    systems = [("P2, 5-point 1000^2", matgen.poisson_2d_5pt(1000))]
    if not a.iter_only:
        systems.append((f"7-point {a.n3}^3", matgen.poisson_3d_7pt(a.n3)))
    for k, (name, (n, rp, ci, v)) in enumerate(systems):
        rpd, cid, vd = d(rp.astype(np.int32)), d(ci.astype(np.int32)), d(v)
        b = d(np.cos(0.001 * np.arange(n)) + 0.5)
        if k == 0:
            t64, t32 = per_iteration(n, rpd, cid, vd, b, a.iters, a.reps)
            nnz = len(v)
            by64 = 12 * nnz + 4 * (n + 1) + 11 * 8 * n
            by32 = 8 * nnz + 4 * (n + 1) + 11 * 4 * n
            lines.append(f"## Time per CG iteration, {name} (n = {n}, nnz = {nnz}), {a.iters} iterations\n")
            lines.append("| iteration | us | byte model | model bytes / time |")
            lines.append("|---|---:|---:|---:|")
            lines.append(f"| double, three launches | {t64:.2f} | {by64 / 1e6:.0f} MB | {by64 / t64 / 1e6:.2f} TB/s |")
            lines.append(f"| float, fused | {t32:.2f} | {by32 / 1e6:.0f} MB | {by32 / t32 / 1e6:.2f} TB/s |")
            lines.append(f"\nfloat / double time: **{t32 / t64:.2f}x** (byte model {by32 / by64:.2f}x)\n")
            print("\n".join(lines), flush=True)
        if not a.iter_only:
            to_solution(f"{name} (n = {n})", n, rpd, cid, vd, b, a.reps, lines)
        del rpd, cid, vd, b
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
