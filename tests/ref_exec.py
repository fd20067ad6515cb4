"""The reference library's own ReferenceExecutor as a child process -- TEST
INFRASTRUCTURE.

oracle/_ref/ref_driver (built by oracle/ref.mk from oracle/ref_driver.cpp and
the reference's sources) runs a batch of cases and returns their result
arrays.  Arrays travel as raw IEEE bytes both ways, so results can be compared
bit for bit.  One process serves a whole batch: collect the cases of a module
with Batch.add(), run them once, index the results by the returned number.
"""
import hashlib
import importlib
import json
import os
import re
import struct
import subprocess
import tempfile
import zlib

import numpy as np

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(REPO_ROOT, "oracle")
DRIVER = os.path.join(ORACLE_DIR, "_ref", "ref_driver")

_CODES = {np.dtype(np.float64): 0, np.dtype(np.float32): 1, np.dtype(np.int32): 2,
          np.dtype(np.int64): 3, np.dtype(np.uint8): 4}
_DTYPES = {v: k for k, v in _CODES.items()}

# format numbers of the driver's `fmt` parameter
CSR, ELL, SELLP, HYBRID, COO, FBCSR, DENSE = range(7)
# the words of the cases as the numbers the driver's parameters carry: word("cycle", "w") == 2
WORDS = {"baseline": ("rhs_norm", "initial_resnorm", "absolute"),
         "storage": ("keep", "reduce1", "reduce2", "integer", "ireduce1", "ireduce2"),
         "isai": ("lower", "upper", "general", "spd"),
         "cycle": ("v", "f", "w"),
         "mid_case": ("both", "post_smoother", "pre_smoother", "standalone"),
         "coarsest": ("identity", "direct", "cg"),
         "guess": ("zero", "rhs", "provided"),
         "smoother": ("null", "eye", "jacobi"),
         "mg_level": ("halve", "all_rows", "pgm")}


def word(kind, w):
    return WORDS[kind].index(w)


def words(kind, ws):
    """a list of words of any length (None: "null") as the i32 array the driver takes"""
    return np.array([word(kind, "null" if w is None else w) for w in ws], np.int32)


def reference_dir():
    """Where `make -C oracle` looks for the reference (its GINKGO_REF)."""
    out = subprocess.run(["make", "-s", "-C", ORACLE_DIR, "--no-print-directory", "ref-where"],
                         capture_output=True, text=True)
    return out.stdout.strip()


def driver():
    """Path of the driver; builds it when the reference is there and it is not.
    Raises when there is no driver: callers decide whether that may skip."""
    if not os.path.exists(DRIVER):
        subprocess.run(["make", "-C", ORACLE_DIR, "ref"], capture_output=True)
    if not os.path.exists(DRIVER):
        raise FileNotFoundError(f"{DRIVER} is missing: build() compiles it from the reference")
    return DRIVER


def have_driver():
    try:
        driver()
    except FileNotFoundError:
        return False
    return True


def read_recording(path, packed_input):
    """The driver output kept by Batch.record() for this very input."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"GKRR":
        raise ValueError(f"{path} is no recording of ref_driver output")
    if data[4:36] != hashlib.sha256(packed_input).digest():
        raise ValueError(f"{path} was recorded for other inputs: record it again where the driver is built")
    (parts,) = struct.unpack_from("<I", data, 36)
    body = data[40:]
    for k in range(1, parts):
        with open(_part(path, k), "rb") as f:
            body += f.read()
    return zlib.decompress(body)


PART_BYTES = 900_000     # a committed file stays below 1 MiB: a longer recording continues in <name>.<k><ext>


def _part(path, k):
    root, ext = os.path.splitext(path)
    return f"{root}.{k}{ext}"


def may_skip():
    """Skipping is allowed only where neither the reference nor oracle/_ref/ exists."""
    return not os.path.isdir(os.path.join(ORACLE_DIR, "_ref")) and not os.path.isdir(reference_dir())


def _s(b):
    return struct.pack("<I", len(b)) + b


class Batch:
    def __init__(self):
        self.cases = []

    def add(self, verb, arrays=None, **params):
        """Queue one case; returns its index into run()'s result list."""
        arrs = {}
        for k, a in (arrays or {}).items():
            a = np.ascontiguousarray(a)
            if a.dtype not in _CODES:
                raise TypeError(f"{verb}: array {k} has dtype {a.dtype}")
            arrs[k] = a
        self.cases.append((verb, {k: float(v) for k, v in params.items()}, arrs))
        return len(self.cases) - 1

    def pack(self):
        """The driver's input for the queued cases, as bytes."""
        out = [b"GKRI" + struct.pack("<I", len(self.cases))]
        for verb, params, arrs in self.cases:
            out.append(_s(verb.encode()) + struct.pack("<I", len(params)))
            for k, v in params.items():
                out.append(_s(k.encode()) + struct.pack("<d", v))
            out.append(struct.pack("<I", len(arrs)))
            for k, a in arrs.items():
                out.append(_s(k.encode()) + struct.pack("<BQ", _CODES[a.dtype], a.size))
                out.append(a.tobytes())
        return b"".join(out)

    def run_raw(self):
        """The driver's output bytes for the queued cases: one driver process."""
        exe = driver()
        with tempfile.TemporaryDirectory() as tmp:
            fin, fout = os.path.join(tmp, "in"), os.path.join(tmp, "out")
            with open(fin, "wb") as f:
                f.write(self.pack())
            r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"ref_driver exited with {r.returncode}: {r.stderr[-2000:]}")
            with open(fout, "rb") as f:
                return f.read()

    def run(self, recording=None):
        """Run all queued cases in one driver process.  Each result is a dict
        name -> 1-D ndarray; a failed case is a dict with only "error".

        recording: a file written by record().  Where there is no driver (a
        machine without the reference and without oracle/_ref/), the results
        the driver wrote for exactly these inputs are read from it instead; a
        recording made for other inputs is an error, never a silent match."""
        if recording is not None and not have_driver():
            return self.unpack(read_recording(recording, self.pack()))
        return self.unpack(self.run_raw())

    def record(self, path):
        """Run the driver and keep its output bytes, keyed by the input's hash."""
        raw = self.run_raw()
        body = zlib.compress(raw, 9)
        chunks = [body[i:i + PART_BYTES] for i in range(0, len(body), PART_BYTES)] or [b""]
        head = b"GKRR" + hashlib.sha256(self.pack()).digest() + struct.pack("<I", len(chunks))
        for k, chunk in enumerate(chunks):
            with open(_part(path, k) if k else path, "wb") as f:
                f.write((head if k == 0 else b"") + chunk)
        return raw

    def unpack(self, data):
        assert data[:4] == b"GKRO"
        pos = 4

        def take(fmt):
            nonlocal pos
            v = struct.unpack_from(fmt, data, pos)
            pos += struct.calcsize(fmt)
            return v

        def take_str():
            nonlocal pos
            (n,) = take("<I")
            s = data[pos:pos + n].decode()
            pos += n
            return s

        (ncases,) = take("<I")
        assert ncases == len(self.cases)
        results = []
        for i in range(ncases):
            (status,) = take("<I")
            msg = take_str()
            (narr,) = take("<I")
            res = {}
            for _ in range(narr):
                name = take_str()
                code, count = take("<BQ")
                dt = _DTYPES[code]
                res[name] = np.frombuffer(data, dt, count, pos).copy()
                pos += count * dt.itemsize
            if status:
                res = {"error": f"{self.cases[i][0]}: {msg}"}
            results.append(res)
        return results


def csr_arrays(m, n, rp, ci, v, pre="", vdt=np.float64, idt=np.int32):
    """Arrays and parameters of a Csr argument of the driver."""
    return ({pre + "rp": np.asarray(rp, idt), pre + "ci": np.asarray(ci, idt),
             pre + "v": np.asarray(v, vdt)}, {pre + "m": m, pre + "n": n})


def dense_arrays(name, a, stride=None, fill=None):
    """A 2-D array as a Dense argument; stride > columns pads each row with `fill`."""
    a = np.asarray(a)
    rows, cols = a.shape
    stride = cols if stride is None else stride
    buf = np.full((rows, stride), a.dtype.type(-77.0) if fill is None else fill, a.dtype)
    buf[:, :cols] = a
    return ({name: buf.reshape(-1)}, {name + "_rows": rows, name + "_cols": cols, name + "_stride": stride})


def bits_equal(a, b):
    """The comparison rule: same shape and dtype, NaN matches NaN regardless
    of sign and payload, everything else as integers (so -0.0 != +0.0)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    ia = a.view(np.int64 if a.dtype == np.float64 else np.int32)
    ib = b.view(ia.dtype)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(ia[~na], ib[~nb]))


def assert_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype} != {want.dtype}"
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    if not bits_equal(got, want):
        g, w = got.reshape(-1), want.reshape(-1)
        if g.dtype.kind == "f":
            bad = ~((g.view(f"i{g.itemsize}") == w.view(f"i{w.itemsize}")) | (np.isnan(g) & np.isnan(w)))
        else:
            bad = g != w
        i = int(np.flatnonzero(bad)[0])
        hexs = (lambda x: float(x).hex()) if g.dtype.kind == "f" else str
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.size} differ, first at {i}: "
                             f"got {hexs(g[i])}, reference {hexs(w[i])}")


# ---- the JSON fixtures recorded from the driver (tests/golden/<family>_ref.json) and the one rule that compares
# an array with what such a fixture keeps of it

FAMILIES = ("par_ilut", "par_ict", "isai", "cb_gmres", "multigrid", "pgm")
LONG = 32   # arrays up to this many entries are kept in full, longer ones as their count, digest and first entries
_HEX = re.compile(r"-?0x[0-9a-f.]+p[+-]\d+$")


def unhex(items):
    return np.array([float.fromhex(t) for t in items], np.float64)


def csr_parts(m):
    """a Csr given as (row_ptrs, col_idxs, vals) or as a dict of these"""
    return m if isinstance(m, dict) else dict(zip(("row_ptrs", "col_idxs", "vals"), m))


def digest(rec):
    """SHA-256 of the bytes of an array as it is (little-endian int32 / float64), of a Csr those of row_ptrs,
    col_idxs and vals one after the other"""
    parts = [rec] if isinstance(rec, np.ndarray) else [csr_parts(rec)[k] for k in ("row_ptrs", "col_idxs", "vals")]
    return hashlib.sha256(b"".join(np.ascontiguousarray(p).tobytes() for p in parts)).hexdigest()


def as_record(a):
    """what a fixture keeps of an array: doubles as hexadecimal floats (the committed files spell them as C's %a
    does, a file written again as Python does: compare by value), integers as they are; a long array as the
    SHA-256 of its bits (float64 / int64, little-endian) with its count and its first four entries"""
    a = np.ascontiguousarray(a).reshape(-1)
    integers = a.dtype.kind != "f"
    bits = a.astype("<i8" if integers else "<f8")
    if a.size <= LONG:
        return [int(t) for t in bits] if integers else [float(t).hex() for t in bits]
    return {"count": int(a.size), "sha256": hashlib.sha256(bits.tobytes()).hexdigest(),
            "head": [int(t) for t in bits[:4]] if integers else [float(t).hex() for t in bits[:4]]}


def _same_items(items, a):
    """a list of integers or of hexadecimal floats holds the array's values: doubles by their bits, never by spelling"""
    a = np.asarray(a).reshape(-1)
    if len(items) != a.size:
        return False
    if a.dtype.kind == "f":
        return all(isinstance(t, str) for t in items) and bits_equal(unhex(items), a.astype(np.float64))
    return [int(t) for t in a] == list(items)


def matches(rec, got, integers=None):
    """`got` is the recorded array, bit for bit.  rec is what as_record() keeps, or -- the layout of the par_ilut,
    par_ict and isai fixtures -- {"sha256": digest(got)} with "items" for a short array and "nnz" for a Csr, which
    `got` then gives as (row_ptrs, col_idxs, vals).  integers: take `got` as integers (default: by its dtype)."""
    if isinstance(rec, dict) and "count" not in rec:
        if digest(got) != rec["sha256"]:
            return False
        if "nnz" in rec:
            parts = csr_parts(got)
            return rec["nnz"] == len(parts["vals"]) and \
                ("items" not in rec or (set(rec["items"]) == set(parts)
                                        and all(_same_items(rec["items"][k], parts[k]) for k in parts)))
        return "items" not in rec or _same_items(rec["items"], got)
    got = np.ascontiguousarray(got).reshape(-1)
    if integers is None:
        integers = got.dtype.kind != "f"
    got = got.astype(np.int64 if integers else np.float64)
    if isinstance(rec, dict):
        return rec["count"] == got.size and rec["sha256"] == as_record(got)["sha256"] and _same_items(rec["head"], got[:4])
    return _same_items(rec, got)


def fixture_difference(fresh, committed, at=""):
    """where two fixtures differ, or None: the same keys both ways, lists of the same length, every leaf equal --
    a double written as a hexadecimal float by its value, whichever way it is spelled"""
    if isinstance(fresh, dict) and isinstance(committed, dict):
        if set(fresh) != set(committed):
            return f"{at}: keys {sorted(set(fresh) ^ set(committed))[:6]} are on one side only"
        pairs = [(f"{at}/{k}", fresh[k], committed[k]) for k in fresh]
    elif isinstance(fresh, (list, tuple)) and isinstance(committed, (list, tuple)):
        if len(fresh) != len(committed):
            return f"{at}: {len(fresh)} entries, committed {len(committed)}"
        pairs = [(f"{at}[{i}]", a, b) for i, (a, b) in enumerate(zip(fresh, committed))]
    else:
        both_hex = isinstance(fresh, str) and isinstance(committed, str) and _HEX.match(fresh) and _HEX.match(committed)
        same = float.fromhex(fresh).hex() == float.fromhex(committed).hex() if both_hex else \
            type(fresh) is type(committed) and fresh == committed
        return None if same else f"{at}: {fresh!r}, committed {committed!r}"
    return next((d for d in (fixture_difference(a, b, p) for p, a, b in pairs) if d is not None), None)


def recorded(family):
    """The fixture of a family as the driver gives it now, in one driver process.  <family>_util.py has the rest:
    queue_cases(batch) -> where each case's result is, case_arrays(results, where) -> {case: {what: ndarray}} under
    the fixture's names, fixture_from(arrays) and, where the file has a layout of its own, dump_fixture(fixture, path)."""
    util = importlib.import_module(family + "_util")
    batch = Batch()
    where = util.queue_cases(batch)
    results = batch.run()
    failed = [r["error"] for r in results if "error" in r]
    assert not failed, failed[:3]
    return util.fixture_from(util.case_arrays(results, where))


def difference_from_driver(family, committed):
    """where a committed fixture differs from what the driver gives now, or None.  The committed "source" is not
    compared, it names the program that wrote those bytes; the one a file written now would carry must name the
    driver and the verb"""
    fresh = recorded(family)
    if f"oracle/ref_driver.cpp, verb {family}," not in fresh["source"]:
        return f"source: {fresh['source']!r} does not name the driver and its verb"
    return fixture_difference({**fresh, "source": committed["source"]}, committed)


def record(family, path=None):
    """Write a family's fixture again (never to make a test pass: the driver and the committed file must agree):
    python -c "import sys; sys.path.insert(0, 'tests'); import ref_exec; ref_exec.record('pgm')" """
    path = path or os.path.join(REPO_ROOT, "tests", "golden", family + "_ref.json")
    util = importlib.import_module(family + "_util")
    if hasattr(util, "dump_fixture"):
        return util.dump_fixture(recorded(family), path)
    with open(path, "w") as f:
        json.dump(recorded(family), f, separators=(",", ":"))
        f.write("\n")
