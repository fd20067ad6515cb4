"""The two ways the host follows a fused solve (pace_fused_solve, csrc/internal.hpp) give the same solve: the host_watch
line, and -- GKOMI_HOST_WATCH=0 -- a blocking look every check_every iterations.  The device decides everything and
the host only watches, so x is compared bit for bit and host_info exactly.  The variable is read once per host thread:
tools/host_watch_solves.py runs in two child processes, once with it and once without."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVERS = ["cg", "cg_jacobi", "bicgstab", "fcg", "cgs", "cg_f32", "ir_mixed"]
RUNS = ["ce1", "ce4", "cap3"]  # check_every 1 and 4 to convergence; max_iters = 3: the last launch stops the solve


def run_child(out, host_watch_off):
    env = dict(os.environ)
    env.pop("GKOMI_HOST_WATCH", None)
    if host_watch_off:
        env["GKOMI_HOST_WATCH"] = "0"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "host_watch_solves.py"), str(out)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    except subprocess.TimeoutExpired:
        pytest.exit("host_watch_solves.py hung: nothing more is started on this GPU", returncode=1)
    if r.returncode < 0:    # died of a signal (a GPU fault aborts the process): stop the session, start nothing more
        pytest.exit(f"host_watch_solves.py died of signal {-r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-2000:]}", returncode=1)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"solves {len(SOLVERS) * len(RUNS)}" in r.stdout
    return dict(np.load(out))


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_watch")
    return run_child(d / "watched.npz", False), run_child(d / "polled.npz", True)


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("solver", SOLVERS)
def test_polling_gives_the_watched_solve(both, solver, run):
    watched, polled = both
    tag = f"{run}_{solver}"
    iw, ip = watched[tag + "_info"], polled[tag + "_info"]
    print(tag, "host_info watched", iw.tolist(), "polled", ip.tolist())
    assert iw[0] >= 0 and (run != "cap3" or (iw[0] == 3 and iw[1] == 0.0))  # the cap stopped the capped solves
    assert run == "cap3" or iw[1] == 1.0                                    # ... and the others converged
    assert iw.tobytes() == ip.tobytes()  # iterations, converged, tau, orig_tau
    assert watched[tag + "_x"].tobytes() == polled[tag + "_x"].tobytes()
