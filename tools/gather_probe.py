#!/usr/bin/env python3
"""What the layout of the gather of b costs the cold nonzero-split SpMV on the 1000^2 5-pt matrix: the kernel as built
(tools/gather_probe.hip, GKOMI_GATHER_PROBE = 0) against the same kernel with every gather instruction's addresses
replaced by lane-linear stand-ins (= 1: 8 lines of 64 B per instruction, still waiting on the loaded columns; wrong
results, only the time counts).  Cold as bench.py times it: 8 rotating copies of the matrix (640 MB > the 256 MiB
Infinity Cache), HIP events around `--steps` launches, the variants alternating in one process.  The product's own
automatic apply is timed beside them.  More builds of the probe (another kernel source) can be added with
--lib name=path.  Diagnostic only; build with tools/gather_probe.sh."""
import argparse, ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "repo-8852-ginkgo_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import gkomi, matgen

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, default=1000)
ap.add_argument("--steps", type=int, default=400)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--lib", action="append", default=[], help="name=path of another build of tools/gather_probe.hip")
args = ap.parse_args()

gk = gkomi.lib()
n, rp, ci, v = matgen.poisson_2d_5pt(args.grid)
nnz = int(rp[-1]); tile = 1536; over = 4   # bench.py passes a row-length hint of 5: over = 4
assert int(gk.csr_srow_tile_for(nnz)) == tile
d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
s = torch.cuda.current_stream().cuda_stream
copies = []
for _ in range(8):
    c = [d(rp), d(ci), d(v), d(np.sin(0.01 * np.arange(n)).reshape(n, 1)), torch.empty((n, 1), dtype=torch.float64, device="cuda")]
    srow = torch.empty(int(gk.csr_srow_entries(nnz, tile)), dtype=torch.int32, device="cuda")
    gk.csr_make_srow_i32(s, n, nnz, c[0], tile, srow, srow.numel())
    copies.append(c + [srow])

libs = {}
for name, path in [("product layout", os.path.join(ROOT, "tools", "bin", "libgather_probe0.so")),
                   ("product layout, lane-linear stand-in", os.path.join(ROOT, "tools", "bin", "libgather_probe1.so"))] + \
        [tuple(a.split("=", 1)) for a in args.lib]:
    lib = ctypes.CDLL(path)
    lib.probe_launch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6 + [ctypes.c_int]
    libs[name] = lib


def launcher(name):
    if name == "library, automatic":
        return lambda c: gk.csr_spmv_srow_f64_i32(s, n, n, 1, nnz, c[0], c[1], c[2], c[3], 1, c[4], 1, None, None,
                                                  0, 5, c[5], tile)
    lib = libs[name]

    def one(c):
        rc = lib.probe_launch(s, n, nnz, c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(), c[3].data_ptr(),
                              c[4].data_ptr(), c[5].data_ptr(), over)
        assert rc == 0, rc
    return one


def timed(name):
    one = launcher(name)
    for i in range(40):
        one(copies[i % 8])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(args.steps):
        one(copies[i % 8])
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.steps


names = ["library, automatic"] + list(libs)
res = {k: [] for k in names}
print(f"{args.grid}^2 5-pt, {n} rows, {nnz} nonzeros, tile {tile}, over {over}; cold over 8 copies, "
      f"us per launch over {args.steps} launches")
for r in range(args.rounds):
    for k in names:
        res[k].append(timed(k))
    print(f"round {r}: " + "  ".join(f"{k}: {res[k][-1]:.2f}" for k in names), flush=True)
base = float(np.median(res["product layout"]))
for k in names:
    m = float(np.median(res[k]))
    print(f"{k:45s} median {m:6.2f}  min {min(res[k]):6.2f}  max {max(res[k]):6.2f}  vs product layout {m / base:.3f}")
