"""Fbcsr apply against the automatic Csr apply on the same block matrix: kron(2-D 5-point Poisson stencil, dense SPD
bs x bs) for bs in {2, 3, 4, 7}, sized so that the CSR form takes about 80 MB and about 200 MB.  Both formats are timed
in the same run with the same library: cold (every timed apply works on another copy of the matrix and the vectors,
the copies together larger than twice the 256 MB Infinity Cache) and warm (the same copy again and again), HIP events
around each apply (cold) or around --warm-reps applies (warm), median of --reps.  Next to the times: the ratio the
byte model predicts and the achieved bytes per second.  Writes a markdown note (--out).

  python tools/fbcsr_probe.py --out profiles/fbcsr_probe.md [--mb 80 200] [--bs 2 3 4 7] [--reps 15]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "repo-8852-ginkgo_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gkomi  # noqa: E402
import matgen  # noqa: E402
from gkomi import formats  # noqa: E402

LLC_BYTES = 256 << 20


def block_system(gk, g, bs):
    """(Fbcsr, Csr) of kron(poisson_2d_5pt(g), S), S dense SPD bs x bs; built on the device from the stencil's CSR form"""
    n, rp, ci, v = matgen.poisson_2d_5pt(g)
    s = np.fromfunction(lambda i, j: 1.0 / (1.0 + abs(i - j)), (bs, bs)) + bs * np.eye(bs)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    # block z = v[z] * S, column-major
    vals = (d(v.astype(np.float64))[:, None] * d(s.T.reshape(1, bs * bs))).reshape(-1).contiguous()
    fb = formats.Fbcsr(gk, n, n, bs, d(rp.astype(np.int32)), d(ci.astype(np.int32)), vals)
    csr = fb.to_csr()   # columns of every row ascending: the same summation order
    return fb, csr


def clone_fbcsr(m):
    return formats.Fbcsr(m.gk, m.nbrows, m.nbcols, m.bs, m.row_ptrs.clone(), m.col_idxs.clone(), m.vals.clone())


def clone_csr(m):
    return formats.Csr(m.gk, m.nrows, m.ncols, m.row_ptrs.clone(), m.col_idxs.clone(), m.vals.clone(), m.strategy, m.split)


def median_us(samples):
    return float(np.median(samples)) * 1e3


def time_cold(copies, vectors, reps):
    """one apply per event pair, each on the copy that was touched longest ago"""
    for m, (b, x) in zip(copies, vectors):   # warm-up: code objects, srow, statistics of every copy
        m.apply(b, x)
    torch.cuda.synchronize()
    out = []
    for r in range(reps):
        m, (b, x) = copies[r % len(copies)], vectors[r % len(copies)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m.apply(b, x)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return median_us(out)


def time_warm(m, b, x, reps, inner):
    for _ in range(3):
        m.apply(b, x)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            m.apply(b, x)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return median_us(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--mb", type=float, nargs="+", default=[80.0, 200.0], help="size of the CSR form in MB")
    ap.add_argument("--bs", type=int, nargs="+", default=[2, 3, 4, 7])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm-reps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    gk = gkomi.lib()
    lines = ["# Fbcsr apply against the automatic Csr apply (tools/fbcsr_probe.py)", "",
             f"kron(5-point stencil on a g x g grid, dense SPD bs x bs); one right-hand side; median of {a.reps} HIP-event timings.  "
             "Cold: every timed apply reads another copy of the matrix and of b (copies > 2 x the 256 MB Infinity Cache in total); "
             f"warm: {a.warm_reps} applies of one copy per timing.  Bytes: Fbcsr (8 bs^2 + 4) per block + 4 per block row, Csr 12 per "
             "nonzero + 4 per row, both + 8 per row for b and for c.  Model ratio = Fbcsr bytes / Csr bytes.  Both formats, same library, same run.",
             "", "| bs | g | rows | nonzeros | CSR MB | Fbcsr MB | Fbcsr cold us | Csr cold us | cold ratio | Fbcsr warm us | Csr warm us | warm ratio | "
             "model ratio | Fbcsr cold TB/s | Fbcsr warm TB/s | Csr cold TB/s | Csr warm TB/s | bits equal |",
             "|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---|"]
    for mb in a.mb:
        for bs in a.bs:
            g = int(round((mb * 1e6 / (12.0 * 5.0 * bs * bs)) ** 0.5))
            fb, csr = block_system(gk, g, bs)
            n = fb.nrows
            fb_bytes = fb.storage_bytes() + 16 * n
            csr_bytes = csr.storage_bytes() + 16 * n
            ncopies = int(2 * LLC_BYTES // fb_bytes) + 2
            fbs = [fb] + [clone_fbcsr(fb) for _ in range(ncopies - 1)]
            csrs = [csr] + [clone_csr(csr) for _ in range(ncopies - 1)]
            b0 = torch.from_numpy(np.cos(0.001 * np.arange(n)).reshape(n, 1)).cuda()
            vec = [(b0.clone(), torch.zeros(n, 1, dtype=torch.float64, device="cuda")) for _ in range(ncopies)]
            # alternate the two formats
            fb_cold = time_cold(fbs, vec, a.reps)
            csr_cold = time_cold(csrs, vec, a.reps)
            fb_cold = min(fb_cold, time_cold(fbs, vec, a.reps))
            csr_cold = min(csr_cold, time_cold(csrs, vec, a.reps))
            fb_warm = time_warm(fb, *vec[0], a.reps, a.warm_reps)
            csr_warm = time_warm(csr, *vec[0], a.reps, a.warm_reps)
            y1, y2 = torch.zeros_like(vec[0][1]), torch.zeros_like(vec[0][1])
            fb.apply(b0, y1)
            csr.apply(b0, y2)
            same = bool(torch.equal(y1.view(torch.int64), y2.view(torch.int64)))
            tbs = lambda nbytes, us: nbytes / us * 1e-6  # noqa: E731
            lines.append(f"| {bs} | {g} | {n} | {csr.nnz} | {csr.storage_bytes() / 1e6:.1f} | {fb.storage_bytes() / 1e6:.1f} | {fb_cold:.1f} | "
                         f"{csr_cold:.1f} | {fb_cold / csr_cold:.3f} | {fb_warm:.1f} | {csr_warm:.1f} | {fb_warm / csr_warm:.3f} | "
                         f"{fb_bytes / csr_bytes:.3f} | {tbs(fb_bytes, fb_cold):.2f} | {tbs(fb_bytes, fb_warm):.2f} | "
                         f"{tbs(csr_bytes, csr_cold):.2f} | {tbs(csr_bytes, csr_warm):.2f} | {'yes' if same else 'NO'} |")
            print(lines[-1], flush=True)
            del fbs, csrs, vec, fb, csr
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
