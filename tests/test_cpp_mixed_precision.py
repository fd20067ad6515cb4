"""Mixed precision in the C++ host mirror (repo-8852-ginkgo_amd/include/ginkgo/ginkgo.hpp): the reference's
examples/mixed-precision-ir/mixed-precision-ir.cpp compiles and links unchanged (read where it lies when the reference
tree is mounted; never copied), Dense precision conversion on a host executor ends in NotCompiled like every other
kernel, and on the GPU examples/mixed_precision_ir solves a Poisson system by the hand-written refinement loop and by
Ir<double> over Cg<float>, the latter through the native driver."""
import os
import re
import subprocess

import numpy as np
import pytest

import matgen

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "repo-8852-ginkgo_amd")
EX = os.path.join(PKG, "examples")
REF_EXAMPLE = "/root/reference/examples/mixed-precision-ir/mixed-precision-ir.cpp"


def _compile(src, out):
    return subprocess.run(["g++", "-std=c++14", "-Wall", f"-I{PKG}/include", str(src), "-o", str(out), f"-L{PKG}/lib", "-lgkomi",
                           f"-Wl,-rpath,{PKG}/lib"], capture_output=True, text=True)


@pytest.mark.skipif(not os.path.exists(REF_EXAMPLE), reason="reference tree not mounted")
def test_reference_mixed_precision_ir_source_compiles_unchanged(tmp_path):
    out = tmp_path / "ref_mixed_precision_ir"
    r = _compile(REF_EXAMPLE, out)
    assert r.returncode == 0, r.stderr
    assert os.path.exists(out)


HOST_CONVERT = r"""
#include <ginkgo/ginkgo.hpp>
#include <iostream>
int main()
{
    auto exec = gko::ReferenceExecutor::create();
    auto d = gko::matrix::Dense<double>::create(exec, gko::dim<2>(4, 1));
    auto f = gko::matrix::Dense<float>::create(exec);
    int caught = 0;
    try { d->convert_to(f.get()); } catch (const gko::NotCompiled&) { caught |= 1; }
    try { f->convert_to(d.get()); } catch (const gko::NotCompiled&) { caught |= 2; }
    auto c = gko::matrix::Csr<double, int>::create(exec);
    auto cf = gko::matrix::Csr<float, int>::create(exec);
    try { c->convert_to(cf.get()); } catch (const gko::NotCompiled&) { caught |= 4; }
    std::cout << "caught " << caught << std::endl;
    return caught == 7 ? 0 : 1;
}
"""


def test_conversion_on_host_executor_raises_not_compiled(tmp_path):
    src = tmp_path / "host_convert.cpp"
    src.write_text(HOST_CONVERT)
    out = tmp_path / "host_convert"
    r = _compile(src, out)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(out)], capture_output=True, text=True)
    assert run.returncode == 0 and "caught 7" in run.stdout, run.stdout + run.stderr


def _write_mtx(path, n, rp, ci, v):
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write(f"{n} {n} {len(v)}\n")
        for r in range(n):
            for k in range(rp[r], rp[r + 1]):
                f.write(f"{r + 1} {ci[k] + 1} {float(v[k])!r}\n")


@pytest.mark.gpu
def test_mixed_precision_ir_example_on_hip(tmp_path):
    r = subprocess.run(["make", "-C", EX], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    (tmp_path / "data").mkdir()
    n, rp, ci, v = matgen.poisson_2d_5pt(80)
    _write_mtx(tmp_path / "data" / "A.mtx", n, rp, ci, v)
    run = subprocess.run([os.path.join(EX, "bin", "mixed_precision_ir"), "hip", "1e-12", "1e-2"], cwd=tmp_path,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    pat = r"{}: outer iterations (-?\d+), inner iterations (-?\d+), true residual (\S+)"
    lo, li, lr = re.search(pat.format("loop"), run.stdout).groups()
    io, ii, irr = re.search(pat.format("ir"), run.stdout).groups()
    assert float(lr) <= 1e-12 and float(irr) <= 1e-12
    assert abs(int(lo) - int(io)) <= 1
    # the recognised Ir path ran the native driver: it reports the inner iterations it summed on the device
    assert int(ii) > 0 and abs(int(ii) - int(li)) <= max(2 * int(lo), int(0.1 * int(li)))
