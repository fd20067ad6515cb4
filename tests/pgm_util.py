"""multigrid::Pgm in numpy / plain Python, twice.

`generate(m, ...)` is the reference executor statement for statement (core/multigrid/pgm.cpp:147-236 over
reference/multigrid/pgm_kernels.cpp:67-348, csr::transpose, csr::spgeam by reference/components/csr_spgeam.hpp:58-104
and csr::extract_diagonal): literal sequential loops over the rows, in place on agg, a stable sort and left-to-right
sums for the coarse matrix.  Python floats are IEEE doubles and every statement rounds once, so the results are the
reference executor's bit for bit; tests/golden/pgm_ref.json (recorded by the verb pgm of oracle/ref_driver.cpp) pins
that.

`generate(m, ..., parallel=True)` is the form the device kernels compute: every sweep reads a snapshot of agg taken
when it starts, match_edge likewise, and the default assign_to_exist_agg is the static choice p(r) of every row
followed by ceil(log2 n) rounds of pointer jumping.  tests/test_pgm_reference.py holds the two equal on every case and
on seeded random matrices -- the order-independence argument of DESIGN.md 4.27, tested.

Also the cases both test files and the driver share, the driver's input and the fixture writer."""
import os

import numpy as np

import multigrid_util as mu
import ref_exec

HERE = os.path.dirname(os.path.abspath(__file__))
csr = mu.csr


# ---- the pieces of W ------------------------------------------------------------------------------------

def compute_absolute(m):
    return m[0], m[1], m[2], m[3], np.abs(m[4])


def spgeam(alpha, a, beta, b):
    """csr::spgeam (reference/matrix/csr_kernels.cpp:313-357): the two-pointer merge of csr_spgeam.hpp:73-103, each
    value alpha * a + beta * b with a literal 0.0 for the missing side"""
    sentinel = np.iinfo(np.int32).max
    a_ci, a_v, b_ci, b_v = a[3].tolist(), a[4].tolist(), b[3].tolist(), b[4].tolist()
    rp, cols, vals = [0], [], []
    for row in range(a[0]):
        a_begin, a_end, b_begin, b_end = int(a[2][row]), int(a[2][row + 1]), int(b[2][row]), int(b[2][row + 1])
        skip = False
        for _ in range((a_end - a_begin) + (b_end - b_begin)):
            if skip:
                skip = False
                continue
            a_col = a_ci[a_begin] if a_begin < a_end else sentinel
            b_col = b_ci[b_begin] if b_begin < b_end else sentinel
            a_val = a_v[a_begin] if a_begin < a_end else 0.0
            b_val = b_v[b_begin] if b_begin < b_end else 0.0
            col = min(a_col, b_col)
            cols.append(col)
            vals.append(alpha * (a_val if a_col == col else 0.0) + beta * (b_val if b_col == col else 0.0))
            a_begin += a_col <= b_col
            b_begin += b_col <= a_col
            skip = a_col == b_col
        rp.append(len(cols))
    return csr(a[0], a[1], rp, cols, vals)


def extract_diagonal(m):
    """csr::extract_diagonal (reference/matrix/csr_kernels.cpp:1016-1034): 0 where no diagonal entry is stored, the
    first one where several are"""
    d = np.zeros(min(m[0], m[1]))
    for r in range(len(d)):
        for k in range(m[2][r], m[2][r + 1]):
            if m[3][k] == r:
                d[r] = m[4][k]
                break
    return d


def weight_matrix(m):
    """W = 0.5 |A| + 0.5 |A|^T and its diagonal (pgm.cpp:177-186)"""
    a = compute_absolute(m)
    w = spgeam(0.5, a, 0.5, mu.transpose(a))
    return w, extract_diagonal(w)


def _tie_greater(aw, ac, bw, bc):
    """std::tie(aw, ac) > std::tie(bw, bc)"""
    return (bw < aw) or (not (aw < bw) and bc < ac)


class _W:
    """a weight matrix as plain lists, for the row loops below"""

    def __init__(self, w, diag):
        self.n = w[0]
        self.rp, self.ci, self.v, self.d = w[2].tolist(), w[3].tolist(), w[4].tolist(), np.asarray(diag).tolist()

    def weight(self, idx, row, col):
        return self.v[idx] / max(abs(self.d[row]), abs(self.d[col]))


# ---- the kernels, sequential (the reference's loops) -----------------------------------------------------

def find_strongest_neighbor(w, agg, strongest, read=None):
    """pgm_kernels.cpp:192-241, in place on agg and strongest; -> rows absorbed.  read: the array the loop reads agg
    from -- agg itself (the reference), or a snapshot (the parallel form)"""
    read = agg if read is None else read
    absorbed = 0
    for row in range(w.n):
        max_weight_unagg, max_weight_agg, strongest_unagg, strongest_agg = 0.0, 0.0, -1, -1
        if read[row] == -1:
            for idx in range(w.rp[row], w.rp[row + 1]):
                col = w.ci[idx]
                if col == row:
                    continue
                weight = w.weight(idx, row, col)
                if read[col] == -1 and _tie_greater(weight, col, max_weight_unagg, strongest_unagg):
                    max_weight_unagg, strongest_unagg = weight, col
                elif read[col] != -1 and _tie_greater(weight, col, max_weight_agg, strongest_agg):
                    max_weight_agg, strongest_agg = weight, col
            if strongest_unagg == -1 and strongest_agg != -1:
                agg[row] = read[strongest_agg]
                absorbed += 1
            elif strongest_unagg != -1:
                strongest[row] = strongest_unagg
            else:
                strongest[row] = row
    return absorbed


def match_edge(strongest, agg, read=None):
    """pgm_kernels.cpp:67-86, in place on agg"""
    read = agg if read is None else read
    for i in range(len(agg)):
        if read[i] == -1:
            neighbor = strongest[i]
            if neighbor != -1 and strongest[neighbor] == i and i <= neighbor:
                agg[i] = i
                agg[neighbor] = i


def count_unagg(agg):
    return sum(1 for a in agg if a == -1)


def assign_to_exist_agg(w, agg, deterministic):
    """pgm_kernels.cpp:247-293: reads agg, writes agg (default) or a copy that replaces it (deterministic)"""
    out = list(agg) if deterministic else agg
    for row in range(w.n):
        if agg[row] != -1:
            continue
        max_weight_agg, strongest_agg = 0.0, -1
        for idx in range(w.rp[row], w.rp[row + 1]):
            col = w.ci[idx]
            if col == row:
                continue
            weight = w.weight(idx, row, col)
            if agg[col] != -1 and _tie_greater(weight, col, max_weight_agg, strongest_agg):
                max_weight_agg, strongest_agg = weight, col
        out[row] = agg[strongest_agg] if strongest_agg != -1 else row
    agg[:] = out


def jump_rounds(n):
    return (n - 1).bit_length() if n > 1 else 0


def assign_to_exist_agg_parallel(w, agg, deterministic, info=None):
    """what the device computes: the deterministic form is the loop above on a snapshot; the default form is the
    static choice of every row, then jump_rounds(n) rounds of next'[r] = next[next[r]] between two buffers"""
    snapshot = list(agg)
    if deterministic:
        assign_to_exist_agg(w, agg, True)
        return
    nxt = list(range(w.n))
    for row in range(w.n):
        if snapshot[row] != -1:
            continue
        best_w, best_c = 0.0, -1
        for idx in range(w.rp[row], w.rp[row + 1]):
            col = w.ci[idx]
            if col == row:
                continue
            if snapshot[col] != -1 or col < row:
                weight = w.weight(idx, row, col)
                if _tie_greater(weight, col, best_w, best_c):
                    best_w, best_c = weight, col
        if best_c != -1:
            nxt[row] = best_c
    if info is not None:
        depth = 0
        for row in range(w.n):
            d, r = 0, row
            while nxt[r] != r:
                r, d = nxt[r], d + 1
            depth = max(depth, d)
        info["chain_depth"] = depth
    for _ in range(jump_rounds(w.n)):
        nxt = [nxt[nxt[r]] for r in range(w.n)]
    agg[:] = [snapshot[r] if snapshot[r] != -1 else r for r in nxt]


def renumber(agg):
    """pgm_kernels.cpp:105-124 -> num_agg"""
    num = len(agg)
    agg_map = [0] * (num + 1)
    for i in range(num):
        agg_map[agg[i]] = 1
    total = 0
    for i in range(num + 1):          # components::prefix_sum, exclusive
        agg_map[i], total = total, total + agg_map[i]
    for i in range(num):
        agg[i] = agg_map[agg[i]]
    return agg_map[num]


def agg_to_restrict(num_agg, agg):
    """pgm.cpp:85-98: the pairs (agg[i], i) sorted, the rows turned into row pointers"""
    pairs = sorted(zip(agg, range(len(agg))))
    rp = np.zeros(num_agg + 1, np.int64)
    for r, _ in pairs:
        rp[r + 1] += 1
    return np.cumsum(rp).astype(np.int32), np.asarray([c for _, c in pairs], np.int32)


def sort_row_major(rows, cols, vals):
    """pgm_kernels.cpp:299-308: std::stable_sort by (row, col)"""
    order = sorted(range(len(rows)), key=lambda k: (rows[k], cols[k]))     # sorted() is stable
    return [rows[k] for k in order], [cols[k] for k in order], [vals[k] for k in order]


def compute_coarse_coo(rows, cols, vals):
    """pgm_kernels.cpp:313-345"""
    c_rows, c_cols, c_vals = [], [], []
    if not rows:
        return c_rows, c_cols, c_vals
    curr_row, curr_col, temp_val = rows[0], cols[0], vals[0]
    for idxs in range(1, len(rows)):
        if curr_row != rows[idxs] or curr_col != cols[idxs]:
            c_rows.append(curr_row)
            c_cols.append(curr_col)
            c_vals.append(temp_val)
            curr_row, curr_col, temp_val = rows[idxs], cols[idxs], vals[idxs]
            continue
        temp_val += vals[idxs]
    c_rows.append(curr_row)
    c_cols.append(curr_col)
    c_vals.append(temp_val)
    return c_rows, c_cols, c_vals


def generate_coarse(fine, num_agg, agg):
    """pgm.cpp:101-141: map_row, map_col, sort_row_major, compute_coarse_coo, Coo -> Csr"""
    nr, _, rp, ci, v = fine
    rows = [agg[r] for r in range(nr) for _ in range(rp[r], rp[r + 1])]
    cols = [agg[c] for c in ci.tolist()]
    rows, cols, vals = sort_row_major(rows, cols, v.tolist())
    c_rows, c_cols, c_vals = compute_coarse_coo(rows, cols, vals)
    crp = np.zeros(num_agg + 1, np.int64)
    for r in c_rows:
        crp[r + 1] += 1
    longest = run = 0
    for k in range(len(rows)):
        run = run + 1 if k and (rows[k], cols[k]) == (rows[k - 1], cols[k - 1]) else 1
        longest = max(longest, run)
    return csr(num_agg, num_agg, np.cumsum(crp), c_cols, c_vals), longest


EXITS = ("nothing left", "no new match", "ratio", "max_iterations")


class PgmLevel:
    """the result of generate: agg, num_agg, the restriction's sparsity, the coarse and the fine Csr, and what
    happened on the way (info)"""

    def __init__(self, fine, agg, num_agg, restrict, coarse, info):
        self.fine, self.num_agg, self.coarse, self.info = fine, num_agg, coarse, info
        self.agg = np.asarray(agg, np.int32)
        self.restrict_row_ptrs, self.restrict_col_idxs = restrict

    def level(self):
        """as a multigrid_util.Level: R and P as unit-valued Csr matrices (SparsityCsr's and RowGatherer's applies add
        the same terms in the same order: 0 + 1 b summed in column order, alpha e + beta x)"""
        n = self.fine[0]
        restrict = csr(self.num_agg, n, self.restrict_row_ptrs, self.restrict_col_idxs, np.ones(n))
        prolong = csr(n, self.num_agg, np.arange(n + 1), self.agg, np.ones(n))
        return mu.Level(self.fine, restrict, self.coarse, prolong)


def generate(m, max_iterations=15, max_unassigned_ratio=0.05, deterministic=False, skip_sorting=False, parallel=False):
    """Pgm::generate (pgm.cpp:147-236) -> PgmLevel"""
    fine = m if skip_sorting else mu.sort_by_column_index(m)
    n = fine[0]
    w = _W(*weight_matrix(fine))
    agg, strongest = [-1] * n, [-1] * n
    num_unagg = num_unagg_prev = n
    info = dict(iterations=0, absorbed=0, exit=3, chain_depth=0)
    for i in range(max_iterations):
        before = list(agg) if parallel else None
        info["absorbed"] += find_strongest_neighbor(w, agg, strongest, before)
        match_edge(strongest, agg, list(agg) if parallel else None)
        num_unagg = count_unagg(agg)
        info["iterations"] = i + 1
        if num_unagg == 0 or num_unagg == num_unagg_prev or num_unagg < max_unassigned_ratio * n:
            info["exit"] = 0 if num_unagg == 0 else (1 if num_unagg == num_unagg_prev else 2)
            break
        num_unagg_prev = num_unagg
    info["left"] = num_unagg
    if num_unagg != 0:
        if parallel:
            assign_to_exist_agg_parallel(w, agg, deterministic, info)
        else:
            assign_to_exist_agg(w, agg, deterministic)
    num_agg = renumber(agg)
    coarse, info["longest_run"] = generate_coarse(fine, num_agg, agg)
    return PgmLevel(fine, agg, num_agg, agg_to_restrict(num_agg, agg), coarse, info)


# ---- matrices ---------------------------------------------------------------------------------------------

def from_dense_pattern(n, entries):
    """entries: {(row, col): value} -> Csr with sorted rows"""
    rows = [[] for _ in range(n)]
    for (r, c), v in sorted(entries.items()):
        rows[r].append((c, v))
    rp = np.cumsum([0] + [len(r) for r in rows])
    return csr(n, n, rp, [c for r in rows for c, _ in r], [v for r in rows for _, v in r])


def reference_5x5():
    """reference/test/multigrid/pgm_kernels.cpp:136-151"""
    return mu.sort_by_column_index(mu.unsorted_5x5())


def grid(nx, ny, nine_point=False):
    """a uniform stencil on an nx x ny grid: 4 (8) on the diagonal, -1 to the 4 (8) neighbours"""
    e = {}
    for y in range(ny):
        for x in range(nx):
            r = y * nx + x
            e[(r, r)] = 8.0 if nine_point else 4.0
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if (dx or dy) and (nine_point or not (dx and dy)) and 0 <= x + dx < nx and 0 <= y + dy < ny:
                        e[(r, (y + dy) * nx + x + dx)] = -1.0
    return from_dense_pattern(nx * ny, e)


def grid27(nx, ny, nz):
    """the uniform 27-point stencil on an nx x ny x nz grid: 26 on the diagonal, -1 to every neighbour"""
    e = {}
    at = lambda x, y, z: (z * ny + y) * nx + x
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                r = at(x, y, z)
                e[(r, r)] = 26.0
                for dz in (-1, 0, 1):
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            if (dx or dy or dz) and 0 <= x + dx < nx and 0 <= y + dy < ny and 0 <= z + dz < nz:
                                e[(r, at(x + dx, y + dy, z + dz))] = -1.0
    return from_dense_pattern(nx * ny * nz, e)


def path(n):
    e = {}
    for r in range(n):
        e[(r, r)] = 2.0
        if r:
            e[(r, r - 1)] = e[(r - 1, r)] = -1.0
    return from_dense_pattern(n, e)


def diagonal(n):
    return from_dense_pattern(n, {(r, r): 1.0 + 0.25 * (r % 7) for r in range(n)})


def blocks_2x2(nblocks):
    e = {}
    for b in range(nblocks):
        i, j = 2 * b, 2 * b + 1
        e[(i, i)], e[(j, j)], e[(i, j)], e[(j, i)] = 3.0, 4.0, -1.0 - 0.125 * (b % 5), -0.5
    return from_dense_pattern(2 * nblocks, e)


def random_matrix(n, per_row, seed, symmetric):
    """n rows, a diagonal and per_row off-diagonal entries per row drawn from a seeded generator; symmetric: the
    pattern (not the values) is made symmetric.  Values are multiples of 1/8 so that ties do occur."""
    rng = np.random.default_rng(seed)
    e = {}
    for r in range(n):
        e[(r, r)] = float(rng.integers(8, 24)) / 4
        for c in rng.choice(n, size=min(per_row, n), replace=False):
            if c != r:
                e[(r, int(c))] = -float(rng.integers(1, 16)) / 8
    if symmetric:
        for (r, c) in list(e):
            e.setdefault((c, r), -float(rng.integers(1, 16)) / 8)
    return from_dense_pattern(n, e)


def star_plus_ring(n):
    """row 0 is a hub joined to every third row (more than 64 entries for n = 200), the others form a ring"""
    e = {(r, r): 6.0 + (r % 3) for r in range(n)}
    for r in range(1, n):
        nxt = r + 1 if r + 1 < n else 1
        e[(r, nxt)] = e[(nxt, r)] = -1.0 - 0.25 * (r % 4)
        if r % 3 == 0 or r < 8:
            e[(0, r)], e[(r, 0)] = -0.5 - 0.125 * (r % 5), -0.75
    return from_dense_pattern(n, e)


# name -> (matrix maker, generate's keyword arguments); deterministic is run both ways by the tests
CASES = {
    "reference_5x5": (reference_5x5, dict(max_iterations=2, max_unassigned_ratio=0.1, skip_sorting=True)),
    "unsorted_5x5": (mu.unsorted_5x5, dict(max_iterations=2, max_unassigned_ratio=0.1)),
    "n1": (lambda: diagonal(1), {}),
    "diagonal_300": (lambda: diagonal(300), {}),
    "blocks_2x2": (lambda: blocks_2x2(150), {}),
    "grid5_17x19": (lambda: grid(17, 19), {}),
    "path_301_it1": (lambda: path(301), dict(max_iterations=1)),
    "random_300_sym": (lambda: random_matrix(300, 3, 5, True), {}),
    "random_300_unsym": (lambda: random_matrix(300, 3, 6, False), {}),
    "star_ring_200": (lambda: star_plus_ring(200), {}),
    "grid9_40x40": (lambda: grid(40, 40, True), {}),
    "1138_bus": (lambda: mu.read_mtx("1138_bus.mtx"), {}),
    "ani4": (lambda: mu.read_mtx("ani4.mtx"), {}),
    "ani4_unsorted": (lambda: mu.shuffled_rows(mu.read_mtx("ani4.mtx")), {}),
    "grid5_17x19_skip": (lambda: grid(17, 19), dict(skip_sorting=True)),
    "grid5_17x19_it0": (lambda: grid(17, 19), dict(max_iterations=0)),
    # weight matrices with 9 to 16 and with more than 16 entries per row on average: the 16- and the 64-lane sub-wave
    "random_300_w10": (lambda: random_matrix(300, 5, 7, True), {}),
    "random_300_w10_it1": (lambda: random_matrix(300, 5, 7, True), dict(max_iterations=1)),
    "grid27_5x6x7": (lambda: grid27(5, 6, 7), {}),
    "random_280_w24_it1": (lambda: random_matrix(280, 12, 9, True), dict(max_iterations=1)),
}


def subwave_width(n, nnz):
    """the lanes per row the device kernels pick for a weight matrix (csrc/pgm.hip): by the integer mean row length"""
    mean = nnz // n if n > 0 else 0
    return 4 if mean <= 4 else 8 if mean <= 8 else 16 if mean <= 16 else 64


def case_subwave_width(name):
    fine = case_matrix(name) if CASES[name][1].get("skip_sorting") else mu.sort_by_column_index(case_matrix(name))
    w, _ = weight_matrix(fine)
    return subwave_width(w[0], len(w[3]))

_cache = {}


def case_matrix(name):
    if name not in _cache:
        _cache[name] = CASES[name][0]()
    return _cache[name]


def restated(name, deterministic=False, parallel=False):
    """computed once per (case, mode, form) and shared; callers must not modify it"""
    key = (name, bool(deterministic), bool(parallel))
    if key not in _cache:
        _cache[key] = generate(case_matrix(name), deterministic=deterministic, parallel=parallel, **CASES[name][1])
    return _cache[key]


def level_records(lvl):
    out = {"agg": lvl.agg, "num_agg": [lvl.num_agg], "restrict/row_ptrs": lvl.restrict_row_ptrs,
           "restrict/col_idxs": lvl.restrict_col_idxs, "fine/col_idxs": lvl.fine[3]}
    out["coarse/row_ptrs"], out["coarse/col_idxs"], out["coarse/vals"] = lvl.coarse[2], lvl.coarse[3], lvl.coarse[4]
    return out


INTEGER_RECORDS = ("agg", "num_agg", "row_ptrs", "col_idxs", "iterations", "levels")


def record_matches(rec, what, got):
    return ref_exec.matches(rec, got, integers=what.endswith(INTEGER_RECORDS))


# ---- whole solves: Multigrid with Pgm on every level -------------------------------------------------------

def pgm_level_factory(**kw):
    return lambda m: generate(m, **kw).level()


STENCIL_PGM = dict(max_iterations=2, max_unassigned_ratio=0.1)     # reference/test/solver/multigrid_kernels.cpp:265-289


def stencil3():
    """the 3 x 3 system of SolvesStencilSystemBy{V,W,F}Cycle (reference/test/solver/multigrid_kernels.cpp:274-275)"""
    return path(3)


SOLVE_MATRICES = {"ani4": lambda: mu.read_mtx("ani4.mtx"), "1138_bus": lambda: mu.read_mtx("1138_bus.mtx"),
                  "stencil3": stencil3}

# whole applies in the words of multigrid_util.SOLVE_CASES, every level coarsened by Pgm with the parameters under "pgm"
SOLVE_CASES = {}
for _cy in mu.CYCLES:
    SOLVE_CASES[f"ani4/{_cy}/pgm"] = dict(mu._case(matrix="ani4", mg_level=["pgm"], cycle=_cy, max_levels=3), pgm={})
    SOLVE_CASES[f"stencil3/{_cy}/pgm"] = dict(
        mu._case(matrix="stencil3", mg_level=["pgm"], cycle=_cy, max_levels=2, min_coarse_rows=1, mid_case="both",
                 relax=1.0, iters=1, guess="provided", max_iters=4), pgm=STENCIL_PGM)
SOLVE_CASES["1138_bus/v/pgm_residual_norm"] = dict(
    mu._case(matrix="1138_bus", mg_level=["pgm"], max_levels=4, max_iters=300, reduction=0.5), pgm=dict(deterministic=True))


def solve_matrix(name):
    if ("solve", name) not in _cache:
        _cache[("solve", name)] = SOLVE_MATRICES[name]()
    return _cache[("solve", name)]


def solve_parts(pgm_factory_for, **others):
    """the `parts` of multigrid_util.restated with "pgm" added; others override (another layer's factories)"""
    parts = {"jacobi": lambda mm: mu._PlainJacobi(mm), "eye": mu.Identity, "direct": mu.Direct, "cg": mu.Cg,
             "identity": None, "pgm": pgm_factory_for}
    parts.update(others)
    return parts


def restated_solve(name):
    c = SOLVE_CASES[name]
    mg, b, x = mu.restated(c, parts=solve_parts(pgm_level_factory(**c["pgm"])), matrix=solve_matrix(c["matrix"]))
    x, it, _ = mg.apply(b, x)
    return {"x": x, "iterations": [it], "levels": [lvl.coarse[0] for lvl in mg.mg_level_list]}


# ---- the cases as ref_driver's verb pgm takes them; as text for examples/pgm_multigrid.cpp ----------------

def _pgm_parameters(kw, deterministic):
    return dict(pgm_max_iterations=kw.get("max_iterations", 15),
                pgm_max_unassigned_ratio=kw.get("max_unassigned_ratio", 0.05), pgm_deterministic=deterministic)


def queue_cases(batch):
    """queues every case on a ref_exec.Batch -> {name: index of its result}"""
    where = {}
    for name, (_, kw) in CASES.items():
        arrays, params = ref_exec.csr_arrays(*case_matrix(name))
        for det in (0, 1):
            where[f"{name}/det{det}"] = batch.add("pgm", arrays, op=0, skip_sorting=kw.get("skip_sorting", False),
                                                  **_pgm_parameters(kw, det), **params)
    for name, c in SOLVE_CASES.items():
        arrays, params = mu.solve_arguments(c, solve_matrix(c["matrix"]))
        where[name] = batch.add("pgm", arrays, op=1, **_pgm_parameters(c["pgm"], c["pgm"].get("deterministic", False)),
                                **params)
    return where


case_arrays = mu.case_arrays


def recorder_input():
    """the cases as text, one per line: the stdin of examples/pgm_multigrid.cpp in its `run` mode, which prints what
    the driver returns as "<case> <what> <count> <items...>" lines (parse_example_output)"""
    lines = []
    for name, (_, kw) in CASES.items():
        m = case_matrix(name)
        for det in (0, 1):
            lines.append(f"generate {name}/det{det} {kw.get('max_iterations', 15)} "
                         f"{float(kw.get('max_unassigned_ratio', 0.05)).hex()} {det} {int(kw.get('skip_sorting', False))} "
                         f"{mu._matrix_text(m)}")
    for name, c in SOLVE_CASES.items():
        m = solve_matrix(c["matrix"])
        kw = c["pgm"]
        word = lambda names: " ".join([str(len(names))] + ["null" if t is None else t for t in names])
        lines.append(f"solve {name} {kw.get('max_iterations', 15)} {float(kw.get('max_unassigned_ratio', 0.05)).hex()} "
                     f"{int(kw.get('deterministic', False))} {c['cycle']} {c['mid_case']} {int(c['post_uses_pre'])} "
                     f"{c['max_levels']} {c['min_coarse_rows']} {c['coarsest']} {float(c['relax']).hex()} {c['iters']} "
                     f"{c['guess']} {c['max_iters']} {float(c['reduction'] or 0.0).hex()} {word(c['mg_level'])} "
                     f"{word(c['pre'])} {word(c['mid'])} {word(c['post'])} {mu._matrix_text(m)} "
                     f"{mu._hex(mu.right_hand_side(m[0]))} {mu._hex(mu.initial_guess(m[0]))}")
    return "\n".join(lines) + "\n"


def parse_example_output(text):
    """{case: {what: [items as written]}} from the lines "<case> <what> <count> <items...>" the example prints"""
    out = {}
    for line in text.splitlines():
        name, what, count, *items = line.split()
        assert len(items) == int(count), (name, what)
        out.setdefault(name, {})[what] = items
    return out


def arrays_from_text(records):
    """the parsed lines as the arrays case_arrays gives: integers as int64, doubles from their hexadecimal spelling"""
    return {name: {what: np.array([int(t) for t in items], np.int64) if what.endswith(INTEGER_RECORDS)
                   else ref_exec.unhex(items) for what, items in arrays.items()} for name, arrays in records.items()}


def restated_records():
    out = {f"{name}/det{det}": level_records(restated(name, bool(det))) for name in CASES for det in (0, 1)}
    for name in SOLVE_CASES:
        out[name] = restated_solve(name)
    return out


def fixture_from(records):
    return mu.fixture_from(records, "pgm")


dump_fixture = mu.dump_fixture
