"""Dense::apply (gkomi_dense_gemm_f64) and Dense::transpose on shapes a user would run, against torch.matmul (rocBLAS,
what the reference's own HIP backend calls) on the same operands in the same run.  HIP-event times after warm-up,
median of --reps.  For every shape: the ordered kernel (mode 1), the split (mode 2) where k is longer than one chunk,
what the automatic mode plans, and the ratio to rocBLAS.  The ordered kernels issue a multiply and an add where rocBLAS
fuses, and sum in the reference's order; the ratio is a measurement, not a gate.  For the bandwidth-bound shapes the
bytes that have to move over the time, against the 6.29 TB/s a device copy reaches.  The second table varies the number
of workgroups of the ordered launch and k: the numbers behind the two thresholds of the automatic rule.

  python tools/dense_gemm_probe.py --out profiles/dense_gemm_probe.md [--reps 5]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "repo-8852-ginkgo_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gkomi  # noqa: E402
from gkomi import formats  # noqa: E402

COPY_TBS = 6.29
PLAN = {1: "tile", 2: "narrow", 3: "split"}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)) * 1e3   # us


def operands(m, n, k):
    g = torch.Generator(device="cuda").manual_seed(m + 3 * n + 7 * k)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)  # noqa: E731
    return rnd(m, k), rnd(k, n), torch.empty((m, n), dtype=torch.float64, device="cuda")


def measure(gk, m, n, k, reps, with_ordered=True):
    a, b, c = operands(m, n, k)
    d = formats.Dense(gk, a)
    out = {"plan": PLAN[int(gk.dense_gemm_plan(m, n, k, 0))]}
    big = int(gk.dense_gemm_split_chunk())
    out["ordered"] = timed(lambda: d.apply(b, c, mode=1), reps) if with_ordered else None
    out["split"] = timed(lambda: d.apply(b, c, mode=2), reps) if k > big else None
    out["blas"] = timed(lambda: torch.matmul(a, b, out=c), reps)
    ref = torch.matmul(a, b)
    d.apply(b, c, mode=0)
    scale = torch.matmul(a.abs(), b.abs())
    out["err"] = float(((c - ref).abs() / scale).max())   # in units of the sum of absolute terms
    return out


def fmt(us):
    return "-" if us is None else (f"{us:.1f}" if us < 1e4 else f"{us:.0f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    gk = gkomi.lib()
    big = int(gk.dense_gemm_split_chunk())
    lines = ["# Dense::apply and Dense::transpose against rocBLAS (tools/dense_gemm_probe.py)", "",
             f"fp64, standard-normal operands, HIP-event times after one warm-up call, median of {a.reps}; `torch.matmul` on the "
             f"same operands in the same run.  Split chunk L = {big}.  ordered = mode 1 (tile kernel for n > 16, narrow "
             "kernel else), split = mode 2, auto = what mode 0 plans.  G/s: 2 m n k over the time of the automatic choice, "
             "in 1e9 (a multiply and an add counted as two).  TB/s: 8 (m k + k n + m n) bytes over that time; the guide's "
             f"device copy reaches {COPY_TBS} TB/s.  err: max |auto - rocBLAS| / (|a| |b|).", "",
             "| shape | m | n | k | ordered us | split us | auto | rocBLAS us | auto / rocBLAS | G/s | TB/s | of copy rate | err |",
             "|---|---:|---:|---:|---:|---:|---|---:|---:|---:|---:|---:|---:|"]
    shapes = [("square 1024", 1024, 1024, 1024, True), ("square 4096", 4096, 4096, 4096, True), ("square 8192", 8192, 8192, 8192, True),
              ("narrow", 1000000, 16, 16, True), ("Gram", 16, 16, 1000000, True), ("GEMV 8192^2", 8192, 1, 8192, True)]
    for name, m, n, k, with_ordered in shapes:
        r = measure(gk, m, n, k, a.reps if m * n * k < 1 << 36 else 2, with_ordered)
        auto = r["split"] if r["plan"] == "split" else r["ordered"]
        nbytes = 8.0 * (m * k + k * n + m * n)
        tbs = nbytes / auto * 1e-6
        lines.append(f"| {name} | {m} | {n} | {k} | {fmt(r['ordered'])} | {fmt(r['split'])} | {r['plan']} | {fmt(r['blas'])} | "
                     f"{auto / r['blas']:.2f} | {2.0 * m * n * k / auto * 1e-3:.0f} | {tbs:.2f} | {tbs / COPY_TBS:.2f} | {r['err']:.1e} |")
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    # transpose
    n = 8192
    src = torch.randn(n, n, dtype=torch.float64, device="cuda")
    d = formats.Dense(gk, src)
    us = timed(lambda: d.transpose(), a.reps)
    us_t = timed(lambda: src.t().contiguous(), a.reps)
    tbs = 16.0 * n * n / us * 1e-6
    lines += ["", f"Transpose {n} x {n}: {us:.1f} us = {tbs:.2f} TB/s read + written ({tbs / COPY_TBS:.2f} of the copy rate; the time "
              f"includes allocating the result); `t().contiguous()` of torch: {us_t:.1f} us.", ""]
    print(lines[-2], flush=True)
    # the automatic rule: workgroups of the ordered launch x k
    lines += ["## Ordered against split by workgroups of the ordered launch and k", "",
              "n = 16 (narrow kernel, 256 rows per workgroup) and n = 64 (tile kernel, 64 x 64 per workgroup); "
              "split / ordered below 1 means the split is faster.", "",
              "| kernel | m | n | k | ordered workgroups | chunks | ordered us | split us | split / ordered | auto |",
              "|---|---:|---:|---:|---:|---:|---:|---:|---:|---|"]
    for kernel, n, rows in (("narrow", 16, 256), ("tile", 64, 64)):
        for wgs in (1, 16, 64, 128, 256, 1024):
            for k in (2 * big, 4 * big, 16 * big, 64 * big):
                m = wgs * rows
                if m * k > 1 << 28:     # a stays below 2 GB
                    continue
                r = measure(gk, m, n, k, 3)
                lines.append(f"| {kernel} | {m} | {n} | {k} | {wgs} | {-(-k // big)} | {fmt(r['ordered'])} | {fmt(r['split'])} | "
                             f"{r['split'] / r['ordered']:.2f} | {r['plan']} |")
                print(lines[-1], flush=True)
                torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
