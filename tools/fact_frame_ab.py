#!/usr/bin/env python3
"""A/B of the level-scheduled numeric phases (csrc/fact_levels.hpp: exact ILU(0), IC(0), the ParILUT and the ParICT
sweep) against another build of the library, and of that build against a second build of the same source, which gives
the noise.  Writes profiles/fact_frame_ab.md.

    python tools/fact_frame_ab.py path/to/parent/libgkomi.so path/to/parent_again/libgkomi.so [--rounds 3] [--reps 7]

Each library runs in a fresh child process (GKOMI_LIB selects it; the tree's own build runs without), the three in
alternation, `--rounds` times.  A child analyses every matrix once per call and then times the numeric call alone:
wall clock around a synchronized call, best of `--reps`, the values restored (outside the timed window) before each.
ParILUT and ParICT sweep L' / U' = the lower / upper part of A's own pattern, so no selection kernel runs.  IC and
ParICT get xu.spd_version of the matrix.  Matrices: ani4, a 300 x 300 5-point grid (wide levels, 8 lanes per row),
a tridiagonal matrix of 20000 rows (one narrow run), arrow(1100) and wide_level_with_long_rows(1300, 20, ..) (the
workgroup kernels, row in LDS and in memory).  A child also hashes every result, so the table says whether the three
builds computed the same bits.

Reading: per matrix and call the median over the rounds of each library; `spread` = largest minus smallest time
of the two parent builds over all rounds; the branch is "within" where its median is at most `spread` away from the
parent's median."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "repo-8852-ginkgo_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import ilu_exact_util as xu  # noqa: E402
import matgen  # noqa: E402

CALLS = ("ILU(0)", "IC(0)", "ParILUT sweep", "ParICT sweep")


def sorted_csr(n, rp, ci, v):
    for r in range(n):
        b, e = rp[r], rp[r + 1]
        o = np.argsort(ci[b:e], kind="stable")
        ci[b:e], v[b:e] = ci[b:e][o], v[b:e][o]
    return rp, ci, v


def matrices():
    kind, nr, nc, rows, cols, vals = matgen.read_mtx(os.path.join(ROOT, "tests", "golden", "ani4.mtx"))
    grid = matgen.poisson_2d_5pt(300)
    return {
        "ani4": sorted_csr(nr, *matgen.coo_to_csr(nr, rows, cols, vals)),
        "grid 300 x 300": sorted_csr(*grid),
        "tridiagonal 20000": xu.tridiagonal(20000),
        "arrow(1100)": xu.arrow(1100),
        "wide_level_with_long_rows(1300, 20)": xu.wide_level_with_long_rows(1300, 20, [1100, 600]),
    }


def split(rp, ci, v, unit_lower):
    """(L', U'): the entries at or below / at or above the diagonal of sorted rows that store their diagonal"""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    out = []
    for keep in (ci <= rows, ci >= rows):
        ptrs = np.zeros(len(rp), np.int32)
        ptrs[1:] = np.cumsum(np.bincount(rows[keep], minlength=len(rp) - 1))
        out.append((ptrs, ci[keep].astype(np.int32), v[keep].astype(np.float64)))
    if unit_lower:
        out[0][2][out[0][1] == rows[ci <= rows]] = 1.0
    return out


def child(data, reps):
    import torch

    import gkomi
    from gkomi import solvers
    gk = gkomi.lib()
    dev = lambda m: tuple(torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in m)
    z = np.load(data)
    names = sorted({k.split("|")[0] for k in z.files})
    res = {"device": torch.cuda.get_device_name(0), "library": gk.path, "ms": {}, "bits": {}}

    def timed(call, outs):
        keep = [o.clone() for o in outs]
        best = float("inf")
        for _ in range(reps + 1):   # the first one warms up
            for o, k in zip(outs, keep):
                o.copy_(k)
            torch.cuda.synchronize()
            t = time.perf_counter()
            call()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t)
        h = hashlib.sha1()
        for o in outs:
            h.update(o.cpu().numpy().tobytes())
        return best * 1e3, h.hexdigest()[:12]

    for name in names:
        a = tuple(z[f"{name}|a{i}"] for i in range(3))
        s = tuple(z[f"{name}|s{i}"] for i in range(3))
        n = len(a[0]) - 1
        ad, sd = dev(a), dev(s)
        got = {}
        an = solvers.FactorizationAnalysis(gk, n, ad[0], ad[1])
        work = ad[2].clone()
        got["ILU(0)"] = timed(lambda: an.compute_lu(ad[0], ad[1], work), [work])
        an = solvers.FactorizationAnalysis(gk, n, sd[0], sd[1])
        work = sd[2].clone()
        got["IC(0)"] = timed(lambda: an.ic_compute(sd[0], sd[1], work), [work])
        l, u = (dev(m) for m in split(*a, unit_lower=True))
        sweep = solvers.ParIlutSweep(gk, n, l, u)
        got["ParILUT sweep"] = timed(lambda: sweep.compute(ad), [l[2], u[2]])
        l = dev(split(*s, unit_lower=False)[0])
        ict = solvers.ParIctSweep(gk, n, l)
        got["ParICT sweep"] = timed(lambda: ict.compute(sd), [l[2]])
        for call, (ms, bits) in got.items():
            res["ms"][f"{name}|{call}"] = ms
            res["bits"][f"{name}|{call}"] = bits
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent", nargs="?")
    ap.add_argument("parent_again", nargs="?")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--child", help="(internal) the matrices; time the library GKOMI_LIB selects and print the result")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps)
    if not args.parent or not args.parent_again:
        ap.error("two builds of the parent are needed")
    libs = [("parent", os.path.abspath(args.parent)), ("parent again", os.path.abspath(args.parent_again)), ("branch", None)]
    mats = matrices()
    runs = {tag: [] for tag, _ in libs}
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "matrices.npz")
        arrays = {}
        for name, m in mats.items():
            s = xu.spd_version(m)
            for i in range(3):
                arrays[f"{name}|a{i}"], arrays[f"{name}|s{i}"] = m[i], s[i]
        np.savez(data, **arrays)
        for rnd in range(args.rounds):
            for tag, path in libs:
                env = dict(os.environ)
                env.pop("GKOMI_LIB", None)
                if path:
                    env["GKOMI_LIB"] = path
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", data, "--reps", str(args.reps)],
                                   env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
                if r.returncode != 0 or not line:
                    print(r.stdout[-4000:])
                    print(f"round {rnd}, {tag}: the child ended with {r.returncode}; nothing more is started")
                    return 1
                runs[tag].append(json.loads(line[0][7:]))
                print(f"round {rnd}, {tag}: done", flush=True)
    first = runs["branch"][0]
    lines = ["# The level-scheduled frame against its parent (`tools/fact_frame_ab.py`)", "",
             f"{first['device']}; {args.rounds} rounds of three fresh processes in alternation (parent, a second build of the",
             f"same parent, branch); per process the best of {args.reps} wall-clock times around a synchronized numeric call, the",
             "analysis done once before and the values restored outside the timed window.  Columns: the median over the",
             "rounds, in ms.  spread: largest minus smallest time of the two parent builds over all rounds.  within: the",
             "branch's median is at most `spread` away from the parent's.  bits: the three builds gave the same values.", "",
             "| matrix | call | parent | parent again | branch | spread | within | bits |", "|---|---|---|---|---|---|---|---|"]
    outside = 0
    for name in mats:
        for call in CALLS:
            key = f"{name}|{call}"
            ms = {tag: [r["ms"][key] for r in runs[tag]] for tag in runs}
            med = {tag: statistics.median(x) for tag, x in ms.items()}
            both = ms["parent"] + ms["parent again"]
            spread = max(both) - min(both)
            within = abs(med["branch"] - med["parent"]) <= spread
            outside += not within
            same = len({r["bits"][key] for tag in runs for r in runs[tag]}) == 1
            lines.append(f"| {name} | {call} | {med['parent']:.4f} | {med['parent again']:.4f} | {med['branch']:.4f} | "
                         f"{spread:.4f} | {'yes' if within else 'NO'} | {'same' if same else 'DIFFER'} |")
    lines += ["", f"{outside} of {len(mats) * len(CALLS)} cells outside the parent's own spread."]
    text = "\n".join(lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "fact_frame_ab.md"), "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
