"""The reference library's own ReferenceExecutor as a child process -- TEST
INFRASTRUCTURE.

oracle/_ref/ref_driver (built by oracle/ref.mk from oracle/ref_driver.cpp and
the reference's sources) runs a batch of cases and returns their result
arrays.  Arrays travel as raw IEEE bytes both ways, so results can be compared
bit for bit.  One process serves a whole batch: collect the cases of a module
with Batch.add(), run them once, index the results by the returned number.
"""
import hashlib
import os
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
