// Runs the sparse-sparse shims of shims/hip/matrix/csr_kernels.hip.cpp (csr::spgemm, advanced_spgemm, spgeam) on the
// device, each once (spgemm_cases.hpp).  Prints one "ran <kernel> ok|WRONG" line per kernel like shim_smoke2.cpp and
// returns the number of wrong ones.
#include "spgemm_cases.hpp"
#include <cstdio>

static int wrong = 0;
static void ran(const char* name, bool ok)
{
    std::printf("ran %s %s\n", name, ok ? "ok" : "WRONG");
    if (!ok) ++wrong;
}

int main()
{
    auto hip = gko::HipExecutor::create(0, gko::ReferenceExecutor::create());
    spgemm_cases::run(hip, ran);
    return wrong;
}
