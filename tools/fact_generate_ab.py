#!/usr/bin/env python3
"""Wall time of every factorization's generate against the parent revision, in both host layers, on one library.
Generate is host-paced (allocations, blocking reads of counts, one analysis per sweep), so this is where a helper
that allocates inside a loop or synchronizes once more would show.  Writes profiles/fact_generate_ab.md.

    python tools/fact_generate_ab.py PARENT_SOLVERS_PY MIRROR_PARENT MIRROR_BRANCH [--rounds 3] [--reps 3]

PARENT_SOLVERS_PY: the parent's gkomi/solvers.py (git show REV:repo-8852-ginkgo_amd/gkomi/solvers.py > file).
MIRROR_PARENT, MIRROR_BRANCH: tools/fact_generate_mirror_time.cpp compiled against the parent's header and against
the tree's (the command is in that file).

Three arms run in alternation, each in a fresh child process, `--rounds` times: the parent, the parent a second time
(the noise), the branch.  A Python child loads its solvers.py beside the tree's package and times every generate
function: wall clock around a synchronized call, best of `--reps` after one warm-up.  Matrices: 1138_bus and a
300 x 300 5-point grid (those of profiles/par_ilut_probe.md and par_ict_probe.md; both symmetric positive definite, so
the IC family runs on them as they are), and par_ilu_generate(iterations=0) on matgen.at_like(108), the number
bench.py reports as parilu_generate_incl_trs_analysis_ms.  A mirror child is the timing program on the first two.

Reading: per cell the median over the rounds of each arm; `spread` = largest minus smallest time of the two parent
arms over all rounds; a cell is "within" where the branch's median is at most `spread` away from the parent's."""
import argparse
import importlib.util
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

import matgen  # noqa: E402

GENERATES = ("par_ilu_generate", "par_ic_generate", "ilu_generate", "ic_generate", "par_ilut_generate", "par_ict_generate")
BUS = os.path.join(ROOT, "tests", "golden", "1138_bus.mtx")


def matrices():
    import par_ilut_util as pu
    n, rp, ci, v = matgen.poisson_2d_5pt(300)
    return {"1138_bus": pu.RECORDED_CASES["1138_bus"](), "grid 300 x 300": (rp, ci, v)}


def child(path, reps):
    import torch

    import gkomi
    spec = importlib.util.spec_from_file_location("gkomi._solvers_timed", path)
    solvers = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(solvers)
    gk = gkomi.lib()
    dev = lambda m: tuple(torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in m)
    res = {"device": torch.cuda.get_device_name(0), "ms": {}}

    def timed(call):
        best = float("inf")
        for _ in range(reps + 1):   # the first one warms up
            torch.cuda.synchronize()
            t = time.perf_counter()
            p = call()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t)
            del p
        return best * 1e3

    for name, m in matrices().items():
        md = dev(m)
        n = len(m[0]) - 1
        for fn in GENERATES:
            res["ms"][f"{name}|{fn}"] = timed(lambda: getattr(solvers, fn)(gk, n, *md))
    n, rp, ci, v = matgen.at_like(108)
    md = dev((rp, ci, v))
    res["ms"]["at_like(108)|par_ilu_generate(iterations=0)"] = timed(lambda: solvers.par_ilu_generate(gk, n, md[0].clone(), md[1], md[2], iterations=0))
    print("RESULT " + json.dumps(res))


def write_mtx(path, m):
    rp, ci, v = m
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    with open(path, "w") as f:
        f.write(f"%%MatrixMarket matrix coordinate real general\n{len(rp) - 1} {len(rp) - 1} {len(ci)}\n")
        f.writelines(f"{r + 1} {c + 1} {float(x):.17g}\n" for r, c, x in zip(rows, ci, v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_solvers", nargs="?")
    ap.add_argument("mirror_parent", nargs="?")
    ap.add_argument("mirror_branch", nargs="?")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", help="(internal) the solvers.py to load and time")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps)
    if not (args.parent_solvers and args.mirror_parent and args.mirror_branch):
        ap.error("the parent's solvers.py and the two builds of the timing program are needed")
    tree = os.path.join(ROOT, "repo-8852-ginkgo_amd", "gkomi", "solvers.py")
    arms = [("parent", os.path.abspath(args.parent_solvers), os.path.abspath(args.mirror_parent)),
            ("parent again", os.path.abspath(args.parent_solvers), os.path.abspath(args.mirror_parent)),
            ("branch", tree, os.path.abspath(args.mirror_branch))]
    runs = {"Python": {tag: [] for tag, _, _ in arms}, "mirror": {tag: [] for tag, _, _ in arms}}
    device = "?"
    with tempfile.TemporaryDirectory() as tmp:
        mtx = []
        for name, m in matrices().items():
            path = os.path.join(tmp, name.replace(" ", "_") + ".mtx")
            write_mtx(path, m)
            mtx.append(f"{name}={path}")
        for rnd in range(args.rounds):
            for tag, solvers_py, mirror in arms:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", solvers_py, "--reps", str(args.reps)],
                                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
                if r.returncode != 0 or not line:
                    print(r.stdout[-4000:])
                    print(f"round {rnd}, {tag}: the Python child ended with {r.returncode}; nothing more is started")
                    return 1
                got = json.loads(line[0][7:])
                device = got["device"]
                runs["Python"][tag].append(got["ms"])
                r = subprocess.run([mirror, str(args.reps), *mtx], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                if r.returncode != 0:
                    print(r.stdout[-4000:])
                    print(f"round {rnd}, {tag}: the mirror child ended with {r.returncode}; nothing more is started")
                    return 1
                runs["mirror"][tag].append({ln.rsplit(" ", 1)[0]: float(ln.rsplit(" ", 1)[1]) for ln in r.stdout.splitlines() if "|" in ln})
                print(f"round {rnd}, {tag}: done", flush=True)
    lines = ["# Generate of every factorization against its parent, both host layers (`tools/fact_generate_ab.py`)", "",
             f"{device}; one library; {args.rounds} rounds of three fresh processes per layer in alternation (parent, the parent a",
             f"second time, branch); per process the best of {args.reps} wall-clock times around a synchronized generate after one",
             "warm-up.  Columns: the median over the rounds, in ms.  spread: largest minus smallest time of the two parent arms",
             "over all rounds.  within: the branch's median is at most `spread` away from the parent's.", "",
             "| layer | matrix | generate | parent | parent again | branch | spread | within |", "|---|---|---|---|---|---|---|---|"]
    outside = cells = 0
    for layer, by_tag in runs.items():
        for key in by_tag["branch"][0]:
            ms = {tag: [r[key] for r in rs] for tag, rs in by_tag.items()}
            med = {tag: statistics.median(x) for tag, x in ms.items()}
            both = ms["parent"] + ms["parent again"]
            spread = max(both) - min(both)
            within = abs(med["branch"] - med["parent"]) <= spread
            outside += not within
            cells += 1
            name, fn = key.split("|")
            lines.append(f"| {layer} | {name} | {fn} | {med['parent']:.3f} | {med['parent again']:.3f} | {med['branch']:.3f} | "
                         f"{spread:.3f} | {'yes' if within else 'NO'} |")
    lines += ["", f"{outside} of {cells} cells outside the parent's own spread."]
    text = "\n".join(lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "fact_generate_ab.md"), "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
