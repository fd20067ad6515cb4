"""Every strided entry point of the C ABI on padded, offset views of its operands.

An operand of include/gkomi.h is (pointer, stride) with stride >= ncols, the pointer aligned only
to the element size, and the stride - ncols padding values of a row are never read and never
written.  The rest of the suite checks values; it passes one stride to every operand of a call and
buffers that come straight from the allocator.  Here every case of tests/view_cases.py runs under
the layouts of tests/view_util.py -- its own stride per operand, odd and even, bases 4, 8 and 12
bytes off a 16-byte boundary, one operand aligned and the others not -- inside poisoned buffers:

  * every non-live element of every buffer, inputs included, is still the poison afterwards;
  * the live results equal the oracle's (or the suite's restatement's) on the same bytes with the
    same strides: bit for bit, or within the existing test's bound where the suite has one (COO and
    Hybrid atomics, the split GEMM, the reductions -- those against the exactly rounded sum);
  * for bit-exact entry points the live bits under every layout equal those of the contiguous,
    aligned control L0, whichever kernel the launcher's dispatch picks.

The case ids name the entry point, the shape and the layout; view_cases.py names the dispatch
predicate each group is there for.  tests/test_views_inventory.py keeps the registry complete."""
import pytest
import torch   # noqa: F401 -- before the library is loaded (the gk fixture): both then share torch's HIP runtime

import view_cases
from view_util import check_case, run_device

pytestmark = pytest.mark.gpu

PARAMS = [(cid, lname) for cid, c in view_cases.CASES.items() for lname in c.layouts]
_L0, _STATE = {}, {}


@pytest.mark.parametrize("cid,lname", PARAMS, ids=[f"{c}-{l}" for c, l in PARAMS])
def test_layout(gk, oracle, cid, lname):
    def run(case, prep):
        extra = None
        if case.state is not None:
            if case.id not in _STATE:
                _STATE[case.id] = case.state(gk, prep.args)
            extra = _STATE[case.id]
        try:
            return run_device(gk, case.fn, prep, extra)
        except Exception as e:
            # a failed HIP call (a positive code of the C ABI, or torch's own error): nothing more may run on this device
            if getattr(e, "code", 0) > 0 or "HIP error" in str(e):
                pytest.exit(f"{cid} {lname}: {e}", returncode=3)
            raise
    check_case(view_cases.CASES[cid], lname, oracle, run, _L0)


@pytest.mark.parametrize("fn", ["coo_spmv_sorted_f64_i32", "coo_spmv2_sorted_f64_i32"])
def test_sorted_coo_refuses_misaligned_matrix_arrays_before_any_launch(gk, oracle, fn):
    """The sorted COO kernels load vals in 16-byte and the index arrays in 8-byte pairs: alignment of the MATRIX arrays is
    a documented precondition there (GKOMI_ENOTSUPPORTED, include/gkomi.h), unlike that of b and c, which the sweep above
    moves freely.  The refusal comes before anything is launched: c, its padding and the workspace stay as they were."""
    import gkomi
    from view_util import LAYOUTS, Prepared, assert_padding, call_values
    case = view_cases.CASES[f"{fn}-rand532x231-advanced-3"]
    args = case.build(oracle)
    for name in ("row_idxs", "col_idxs", "vals"):
        args[name].offset = True
    try:
        prep = Prepared(args, LAYOUTS["L1a"], -1)
    finally:
        for name in ("row_idxs", "col_idxs", "vals"):
            args[name].offset = False
    dbuf = {k: torch.from_numpy(b).to("cuda:0") for k, b in prep.bufs.items()}
    nbytes = args["workspace"].size(gk)
    ws = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device="cuda:0")
    resolve = lambda k: (ws, nbytes) if k == "workspace" else dbuf[k][prep.geom[k][0]:]
    values, _ = call_values(fn, prep, resolve, torch.cuda.current_stream().cuda_stream)
    with pytest.raises(gkomi.GkomiError) as e:
        getattr(gk, fn)(*values)
    assert e.value.code == -2
    torch.cuda.synchronize()
    got = {k: t.cpu().numpy() for k, t in dbuf.items()}
    assert_padding(prep, got)
    assert all(got[k].tobytes() == prep.bufs[k].tobytes() for k in got) and bool((ws == 0x5a).all())
