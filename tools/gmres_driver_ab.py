#!/usr/bin/env python3
"""The GMRES and CB-GMRES drivers against the parent revision's library: the same bits, the same time.

    python tools/gmres_driver_ab.py PARENT_LIB [--out profiles/gmres_driver_ab.md] [--rounds 3] [--reps 3]

PARENT_LIB: libgkomi.so of the parent commit, built outside the tree (git worktree add DIR REV; make -C
DIR/repo-8852-ginkgo_amd).  Both libraries are driven through the C ABI by the tree's gkomi/solvers.py (GKOMI_LIB picks
the library), each in fresh child processes; a child that fails ends the script.

Bits: every case of cases() is solved by the parent, by the parent a second time and by the branch; a case is equal
where x agrees byte for byte and every host_info entry (iterations, converged, both norms per column, forced_resets of
CB-GMRES) bit for bit.  The environment switches of gmres.hip are read per process or per solve, so the cases come in
three groups with a child each.  A case on which the parent disagrees with itself is reported and compared again with
GKOMI_GMRES_PERSISTENT=0.

Time: whole solves, wall clock around the blocking call; three arms (parent, parent again, branch) in alternation over
`--rounds` rounds, a fresh process each, per process the best of `--reps` solves after one warm-up.  Reading as in
profiles/fact_generate_ab.md: per cell the median over the rounds of each arm; spread = largest minus smallest time of
the two parent arms over all rounds; within = the branch's median is at most `spread` away from the parent's."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "repo-8852-ginkgo_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import matgen  # noqa: E402

GROUPS = {"default": {}, "sweep": {"GKOMI_GMRES_ARNOLDI": "sweep"}, "no single launch": {"GKOMI_GMRES_PERSISTENT": "0"}}
STORAGES = ("keep", "reduce1", "reduce2", "integer", "ireduce1", "ireduce2")
BASELINES = ("rhs_norm", "initial_resnorm", "absolute")


def case(solver, system, kd, nrhs=1, storage=None, baseline="rhs_norm", max_iters=2000, reduction=1e-10, jacobi=0,
         ell=False, xoff=0, group="default"):
    c = dict(solver=solver, system=system, kd=kd, nrhs=nrhs, storage=storage, baseline=baseline, max_iters=max_iters,
             reduction=reduction, jacobi=jacobi, ell=ell, xoff=xoff, group=group)
    parts = [solver + (f" {storage}" if storage else ""), system, f"m={kd}", f"nrhs={nrhs}", baseline]
    parts += [f"max_iters={max_iters}, to {reduction:g}"] if max_iters < 2000 else []
    parts += [f"block-Jacobi({jacobi})"] if jacobi else []
    parts += ["ELL callback"] if ell else []
    parts += ["x at an 8-byte offset"] if xoff else []
    parts += [group] if group != "default" else []
    c["name"] = ", ".join(parts)
    return c


def cases():
    out = []
    # GMRES, one column, a launch per basis vector (n < 64 x CUs)
    for system in ("cd8", "cd7", "poisson 37x41"):
        out += [case("gmres", system, kd, baseline=bl) for kd in (5, 30) for bl in BASELINES]
    out += [case("gmres", "cd8", 5, max_iters=8, reduction=1e-30), case("gmres", "cd8", 30, xoff=1)]
    # GMRES, one launch per Arnoldi step (n >= 64 x CUs): narrow and wide loads, both sweeps, and switched off
    for group in GROUPS:
        out += [case("gmres", system, kd, group=group) for system in ("cd27", "cd28") for kd in (10, 30)]
    # GMRES, the reference sequence for three columns; an operator behind a callback
    out += [case("gmres", "cd8", 30, nrhs=3), case("gmres", "cd8", 30, nrhs=3, jacobi=8), case("gmres", "cd8", 30, ell=True)]
    # CB-GMRES; m = 5 has a forced limit of 0, and the solves to 1e-10 from rhs_norm go through forced resets
    for system in ("cd8", "cd7"):
        out += [case("cb_gmres", system, kd, nrhs=nrhs, storage=st, baseline=bl)
                for st in STORAGES for nrhs in (1, 3) for kd in (5, 10, 30) for bl in BASELINES[:2]]
    out += [case("cb_gmres", "cd8", 5, storage="reduce1", max_iters=8, reduction=1e-30),
            case("cb_gmres", "cd8", 20, storage="reduce1", jacobi=8), case("cb_gmres", "cd8", 30, storage="reduce1", ell=True)]
    out += [case("gmres", "empty", 3, max_iters=2), case("cb_gmres", "empty", 3, storage="keep", max_iters=2)]
    return out


TIMED = [case("gmres", "cd108", 30, max_iters=5000), case("cb_gmres", "cd108", 30, storage="reduce1", max_iters=5000),
         case("cb_gmres", "cd108", 30, storage="keep", max_iters=5000), case("gmres", "cd8", 30),
         case("cb_gmres", "cd8", 30, storage="reduce1")]


def system(name):
    if name == "empty":
        return 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0)
    if name.startswith("poisson"):
        return matgen.poisson_2d_5pt(37, 41)
    return matgen.at_like(int(name[2:]), 0.5)   # convection_diffusion_3d(g) of tests/test_gmres_precond_gpu.py


class Problems:
    """device operands of the systems, made once per child"""

    def __init__(self, gk):
        import torch
        self.gk, self.torch, self.made = gk, torch, {}
        self.dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def get(self, c):
        from gkomi import formats, solvers
        key = (c["system"], c["nrhs"], c["jacobi"], c["ell"])
        if key not in self.made:
            n, rp, ci, v = system(c["system"])
            csr = tuple(self.dev(a) for a in (rp, ci, v))
            i = np.arange(n, dtype=np.float64)
            b = np.stack([np.cos(0.3 * i + 0.7 * col) for col in range(c["nrhs"])], axis=1)
            pre = solvers.jacobi_generate(self.gk, n, *csr, max_block_size=c["jacobi"], nrhs=c["nrhs"]) if c["jacobi"] else None
            ell = formats.Ell.from_csr(formats.Csr(self.gk, n, n, *csr)) if c["ell"] else None
            self.made[key] = (n, csr, self.dev(b), pre, ell)
        return self.made[key]

    def solve(self, c):
        from gkomi import solvers
        torch = self.torch
        n, csr, b, pre, ell = self.get(c)
        x = torch.zeros(n * c["nrhs"] + c["xoff"], dtype=torch.float64, device="cuda:0")[c["xoff"]:].reshape(n, c["nrhs"])
        common = dict(x=x, krylov_dim=c["kd"], max_iters=c["max_iters"], reduction=c["reduction"], baseline=c["baseline"],
                      precond=pre)
        if c["solver"] == "cb_gmres":
            return solvers.cb_gmres_solve(self.gk, n, *(csr if ell is None else (None, None, None)), b, storage=c["storage"],
                                          matrix=ell, **common)
        if ell is not None:
            return solvers.solve_op(self.gk, "gmres", ell, b, **common)
        return solvers.gmres_solve(self.gk, n, *csr, b, **common)


def child(mode, group, reps):
    import torch

    import gkomi
    problems = Problems(gkomi.lib())
    out = {"device": torch.cuda.get_device_name(0), "cases": {}}
    for c in (TIMED if mode == "time" else [c for c in cases() if c["group"] == group]):
        if mode == "time":
            best = float("inf")
            for _ in range(reps + 1):   # the first one warms up
                torch.cuda.synchronize()
                t = time.perf_counter()
                problems.solve(c)
                torch.cuda.synchronize()
                best = min(best, time.perf_counter() - t)
            out["cases"][c["name"]] = best * 1e3
            continue
        res = problems.solve(c)
        torch.cuda.synchronize()
        info = [float(res["iterations"]), float(res["converged"]), *res["residual_norm"], *res["baseline_norm"],
                float(res.get("forced_resets", 0))]
        out["cases"][c["name"]] = {"x": hashlib.sha256(res["x"].cpu().numpy().tobytes()).hexdigest(),
                                   "info": [float(t).hex() for t in info], "iterations": res["iterations"],
                                   "forced_resets": res.get("forced_resets", 0)}
    print("RESULT " + json.dumps(out))


def run_child(lib, mode, group, reps, extra_env=None):
    """the child's result, or None after printing what it said: the caller starts nothing more"""
    env = dict(os.environ, GKOMI_LIB=lib, **GROUPS[group], **(extra_env or {}))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--group", group, "--reps", str(reps)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print(r.stdout[-4000:])
        print(f"{mode}, {group}, {lib}: the child ended with {r.returncode}; nothing more is started")
        return None
    return json.loads(line[0][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_lib", nargs="?")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmres_driver_ab.md"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", help="(internal) bits or time")
    ap.add_argument("--group", default="default", help="(internal)")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.group, args.reps)
    if not args.parent_lib:
        ap.error("the parent's libgkomi.so is needed")
    arms = [("parent", os.path.abspath(args.parent_lib)), ("parent again", os.path.abspath(args.parent_lib)),
            ("branch", os.path.join(ROOT, "repo-8852-ginkgo_amd", "lib", "libgkomi.so"))]
    device = "?"

    # ---- bits -----------------------------------------------------------------------------------------------------
    bits = {tag: {} for tag, _ in arms}
    for group in GROUPS:
        for tag, lib in arms:
            got = run_child(lib, "bits", group, args.reps)
            if got is None:
                return 1
            device = got["device"]
            bits[tag].update(got["cases"])
            print(f"bits, {group}, {tag}: {len(got['cases'])} cases", flush=True)
    lines = ["# GMRES and CB-GMRES drivers against the parent's library (`tools/gmres_driver_ab.py`)", "",
             f"{device}.  Every case through the C ABI on the parent's library, on it a second time and on the branch's, a",
             "fresh process each.  cdG: the convection-diffusion system on a G^3 grid, b = cos(0.3 i) (column c: cos(0.3 i +",
             "0.7 c)); m: the restart length.  equal bits: x byte for byte; equal host_info: every entry bit for bit.", "",
             "| case | iterations | forced resets | equal bits | equal host_info |", "|---|---|---|---|---|"]
    unstable = [name for name in bits["parent"] if bits["parent"][name] != bits["parent again"][name]]
    equal = 0
    for name, par in bits["parent"].items():
        if name in unstable:
            continue
        br = bits["branch"][name]
        eq_x, eq_info = br["x"] == par["x"], br["info"] == par["info"]
        equal += eq_x and eq_info
        lines.append(f"| {name} | {par['iterations']} | {par['forced_resets']} | {'yes' if eq_x else 'NO'} | "
                     f"{'yes' if eq_info else 'NO'} |")
    total = len(bits["parent"])
    if unstable:
        # the parent is not reproducible on these: a finding about the parent; the same systems without the single launch
        again = {}
        for tag, lib in arms:
            got = run_child(lib, "bits", "default", args.reps, {"GKOMI_GMRES_PERSISTENT": "0"})
            if got is None:
                return 1
            again[tag] = got["cases"]
        for name in unstable:
            base = name.replace(", sweep", "").replace(", no single launch", "")
            par, par2, br = (again[tag][base] for tag, _ in arms)
            eq_x, eq_info = br["x"] == par["x"] == par2["x"], br["info"] == par["info"] == par2["info"]
            equal += eq_x and eq_info
            lines.append(f"| {name}: THE PARENT DISAGREES WITH ITSELF; compared with GKOMI_GMRES_PERSISTENT=0 | "
                         f"{par['iterations']} | {par['forced_resets']} | {'yes' if eq_x else 'NO'} | {'yes' if eq_info else 'NO'} |")
    resets = sum(1 for r in bits["parent"].values() if r["forced_resets"] > 0)
    lines += ["", f"{equal} of {total} cases equal", "", f"{resets} of the parent's cases report forced resets."]

    # ---- time -----------------------------------------------------------------------------------------------------
    ms = {tag: [] for tag, _ in arms}
    for rnd in range(args.rounds):
        for tag, lib in arms:
            got = run_child(lib, "time", "default", args.reps)
            if got is None:
                return 1
            ms[tag].append(got["cases"])
            print(f"time, round {rnd}, {tag}: done", flush=True)
    lines += ["", "## Whole solves, wall clock", "",
              f"{args.rounds} rounds of three fresh processes in alternation (parent, the parent a second time, branch); per process",
              f"the best of {args.reps} solves after one warm-up, wall clock around the synchronized call.  Columns: the median over",
              "the rounds, in ms.  spread: largest minus smallest time of the two parent arms over all rounds.  within: the",
              "branch's median is at most `spread` away from the parent's.", "",
              "| solve | parent | parent again | branch | spread | within |", "|---|---|---|---|---|---|"]
    outside = 0
    for c in TIMED:
        t = {tag: [r[c["name"]] for r in rs] for tag, rs in ms.items()}
        med = {tag: statistics.median(x) for tag, x in t.items()}
        both = t["parent"] + t["parent again"]
        spread = max(both) - min(both)
        within = abs(med["branch"] - med["parent"]) <= spread
        outside += not within
        lines.append(f"| {c['name']} | {med['parent']:.3f} | {med['parent again']:.3f} | {med['branch']:.3f} | {spread:.3f} | "
                     f"{'yes' if within else 'NO'} |")
    lines += ["", f"{outside} of {len(TIMED)} cells outside the parent's own spread."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0 if equal == total else 1


if __name__ == "__main__":
    sys.exit(main())
