"""Matrices that sit exactly ON the acceptance threshold of the natural-order Gauss-Jordan kernels, a float64 model of the sweep that
says so, and the lists tests/test_accept_cases_cpu.py checks and tests/test_gpu_accept.py runs. numpy only.

The contract: the natural-order kernel keeps a matrix while every multiplier it forms satisfies |m| <= 4 (NaN fails) and hands it to
the pivoting kernel otherwise. Which multipliers it forms (csrc/tile_common.hpp, PanelSolve; csrc/rowlane2_kernels.hip, Rl2Step):

  tile kernels (gj_tile, gj_tile4, the screening pass, the fused solve): the sweep runs on W = A^T (W[i][j] = mem[i n + j]), identity
      padded to 16 NT, in blocks of four pivots. Block rK of tile tK holds the tile-local indices TileGeo<T>::pcol(rK, 0 .. 3):
      4 rK + t in fp64, 4 t + rK in fp32. Per block: the six multipliers of the LU factorisation of D = W[K, K] without pivoting, and
      every entry of -W[rows not in K, K] D^-1. The one-wavefront kernels with FULL n and an even tile count (n = 32, 64) load through
      a symmetric relabelling: padded index p sits in tile 2 (p / 32) + (p & 1) at tile-local index (p % 32) / 2.
  gj_rowlane2 (17 <= n <= 25): the sweep runs on A itself, one pivot at a time in index order: -a_rk / a_kk for every r != k.

The constructions (all in W space, W = the matrix the sweep sees; base = conftest.spd_batch, R + R^T + n I, multipliers <= 0.1):

  type A   row and column i zeroed, W[i][i] = 1/4, one coupling c at (j, i), j AFTER i in the sweep. No step before i touches row or
           column i, so the multiplier of row j at pivot i is c / (1/4) exactly: +-4 for c = +-1, one ulp beyond for c = +-nextafter(1, 2).
           j in i's own block: one of the six LU multipliers (value +c / delta); otherwise an A-operand entry (value -c / delta).
           `sym`: the coupling mirrored to (i, j); the matrix is then bitwise symmetric.
  type B   rows and columns r and i zeroed, r in an EARLIER block than i, [[a, b], [c, d]] on (r, i). Step r has multiplier c / a = 1/2
           (2 for the transposed form), step i the pivot d - c b / a and the multiplier -b / pivot on the already pivoted row r.
           symmetric form  a = 1, b = c = +-1/2, d = 3/8: pivot 1/8, multiplier -+4; b = c = +-nextafter(1/2, 1) goes beyond.
           one-sided form  a = 1, b = +-2, c = +-1/2, d = 3/2: pivot 1/2, multiplier -+4; b = +-nextafter(2, 3) goes beyond.
           `BT`: the transpose of a one-sided matrix that goes beyond 4. Its largest multiplier is nextafter(2, 3): it must be ACCEPTED,
           which pins the orientation of the sweep.

Every entry involved is a power of two or one ulp off it, so the fp32 kernels see the same values, and a reciprocal refined by one
Newton step is exact on a power of two. A case is (kind, i, other index, variant); the variant names the tested value:
"+4", "-4" (accept), ">+4", "<-4" (reject)."""
import collections
import functools
import re

import numpy as np

from conftest import pkg, spd_batch

TAU = 4.0
NP_DTYPES = {"f64": np.float64, "f32": np.float32}
EPS = {"f64": 2.0 ** -52, "f32": 2.0 ** -23}
VARIANTS = ("+4", "-4", ">+4", "<-4")
REJECTED = {"+4": False, "-4": False, ">+4": True, "<-4": True}
COND_CAP = 1e4
N_BASES = 8
LIST_CAP = 1500
WORK_CAP = 1.2e9   # batch * N^3 of one list: what keeps the float64 model of all lists well under a minute
LIST_FLOOR = 128   # enough for every tile row on both sides of a pivot and the LU slots of three blocks at 16 x 16 tiles

# the sizes of the lists, literal so that importing this module (test collection) does not load the library; sizes() derives them from
# the route and tests/test_accept_cases_cpu.py compares the two
SIZES = {"f64": (17, 25, 26, 32, 33, 48, 49, 64, 65, 80, 97, 112, 129, 144, 192),
         "f32": (17, 25, 26, 32, 33, 48, 49, 64, 65, 80, 81, 96, 113, 128, 129, 144, 256)}

# how a padded index p maps to (tile, tile-local index) and how a tile-local index maps to (block, pivot number): csrc/tile_common.hpp
BLK = {"f64": lambda c: c >> 2, "f32": lambda c: c & 3}
PIV = {"f64": lambda c: c & 3, "f32": lambda c: c >> 2}
PCOL = {"f64": lambda rK, t: 4 * rK + t, "f32": lambda rK, t: 4 * t + rK}

# family: rowlane2 / tile / tile4; w: pivots per block; N: padded size; blocks[b] = the padded indices of block step b in pivot order
# (blocks of identity padding alone are not run and not listed); tile[p], local[p], step[p], pivno[p] for p < N; transposed: W = A^T
Geo = collections.namedtuple("Geo", "dtype n name family w N blocks tile local step pivno transposed")
# kind: "A" / "B" / "BT"; i: the pivot at which the tested multiplier is formed; other: the row that carries it (A: the coupled row j,
# B: the already pivoted row r); sym: the matrix is bitwise symmetric; base: which base matrix; where: "lu" or "aop"
Case = collections.namedtuple("Case", "kind i other variant sym base where")


def api():
    return pkg("api")


def shape_of(name):
    """(family, shape key, template arguments) of a natural-order kernel name; None for any other kernel"""
    m = re.match(r"matinv_(gj_rowlane2|gj_tile4_f\d+|gj_tile_f\d+)<([^>]*)>", name)
    if not m:
        return None
    args = [a.strip() for a in m.group(2).split(",")]
    if m.group(1) == "gj_rowlane2":
        return "rowlane2", ("rowlane2", int(args[1])), args
    if m.group(1).startswith("gj_tile4"):
        nt = int(args[0])
        return "tile4", ("tile4", int(args[2]) if nt <= 8 else "NT"), args
    return "tile", ("tile", int(args[0])), args


@functools.lru_cache(maxsize=None)
def route(dtype):
    """{n: kernel name} of the MATINV_ALGO_GAUSS_JORDAN, KERNEL_AUTO route for every n the natural-order kernels serve"""
    a = api()
    code = a.F64 if dtype == "f64" else a.F32
    out = {}
    for n in range(17, 1025):
        name = a.kernel_name(a.ALGO_GAUSS_JORDAN, code, n, a.KERNEL_AUTO)
        if shape_of(name) is None:
            break
        out[n] = name
    return out


@functools.lru_cache(maxsize=None)
def sizes(dtype):
    """per distinct kernel shape the smallest ragged n and the smallest n that is a multiple of 16 (gj_rowlane2: the smallest n of each
    register width), and the last n of the one-wave-per-tile-column form"""
    by_shape = {}
    for n, name in route(dtype).items():
        by_shape.setdefault(shape_of(name)[1], []).append(n)
    picked = set()
    for key, ns in by_shape.items():
        if key[0] == "rowlane2":
            picked.add(min(ns))
            continue
        picked.add(min(n for n in ns if n % 16))
        full = [n for n in ns if n % 16 == 0]
        if full:
            picked.add(min(full))
        if key[1] == "NT":
            picked.add(max(ns))
    return tuple(sorted(picked))


@functools.lru_cache(maxsize=None)
def geo(dtype, n, solve=False):
    """the sweep of the kernel the route names for (dtype, n); solve: of the fused solve kernel (the one-wavefront tile sweep)"""
    name = route(dtype)[n]
    family, _, args = shape_of(name)
    if solve:
        family, args = "tile", [str((n + 15) // 16), "true" if n % 16 == 0 else "false"]
    if family == "rowlane2":
        N = int(args[1])
        p = np.arange(N)
        blocks = np.arange(n).reshape(n, 1)
        return Geo(dtype, n, name, family, 1, N, blocks, p // 16, p % 16, np.where(p < n, p, -1), np.zeros(N, int), False)
    nt = int(args[0])
    assert nt == (n + 15) // 16
    N = 16 * nt
    p = np.arange(N)
    paired = family == "tile" and args[1] == "true" and nt % 2 == 0  # PAIRED of gj_tile_body / solve_tile_body
    tile = np.where(paired, 2 * (p // 32) + (p & 1), p // 16)
    local = np.where(paired, (p % 32) // 2, p % 16)
    where = {(int(t), int(c)): int(q) for q, t, c in zip(p, tile, local)}
    blocks = []
    for kb in range(4 * nt):
        K = [where[(kb >> 2, PCOL[dtype](kb & 3, t))] for t in range(4)]
        assert all(BLK[dtype](int(local[q])) == (kb & 3) and PIV[dtype](int(local[q])) == t for t, q in enumerate(K))
        if min(K) < n:
            blocks.append(K)
    blocks = np.array(blocks)
    step, pivno = np.full(N, -1), np.zeros(N, int)
    for b, K in enumerate(blocks):
        step[K], pivno[K] = b, np.arange(4)
    assert (step[:n] >= 0).all()
    return Geo(dtype, n, name, family, 4, N, blocks, tile, local, step, pivno, True)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def lu_nopivot(D):
    """(B, w, w) -> (L, D^-1): Doolittle without pivoting, L[:, i, k] the multiplier of row i at pivot k; the inverse by the two
    triangular solves the kernel runs"""
    w = D.shape[1]
    U, L = D.copy(), np.zeros_like(D)
    Y = np.broadcast_to(np.eye(w), D.shape).copy()
    for k in range(w):
        for i in range(k + 1, w):
            L[:, i, k] = U[:, i, k] / U[:, k, k]
            U[:, i, :] -= L[:, i, k, None] * U[:, k, :]
            Y[:, i, :] -= L[:, i, k, None] * Y[:, k, :]
    X = np.zeros_like(D)
    for i in reversed(range(w)):
        acc = Y[:, i, :].copy()
        for j in range(i + 1, w):
            acc -= U[:, i, j, None] * X[:, j, :]
        X[:, i, :] = acc / U[:, i, i, None]
    return L, X


LU_SLOTS = ((1, 0), (2, 0), (3, 0), (2, 1), (3, 1), (3, 2))  # l10 l20 l30 l21 l31 l32, the order PanelSolve tests them in


def sweep(W, g):
    """The natural-order sweep of geometry g on W (B, n, n) float64, the matrices as the kernel sees them. Returns every multiplier:
    lu[B, steps, 6] (block size 4: the LU multipliers of D in the order of LU_SLOTS; zero-width for block size 1) and
    aop[B, steps, N, w] = -W[row, K] D^-1 with the pivot rows, which are exempt, set to zero (row: padded index)."""
    B, n, N, w = W.shape[0], g.n, g.N, g.w
    perm = np.concatenate([g.blocks.reshape(-1), np.setdiff1d(np.arange(N), g.blocks.reshape(-1))])
    P = np.broadcast_to(np.eye(N), (B, N, N)).copy()
    P[:, :n, :n] = W
    P = np.ascontiguousarray(P[:, perm][:, :, perm])
    nb = len(g.blocks)
    lu = np.zeros((B, nb, 6 if w == 4 else 0))
    aop = np.zeros((B, nb, N, w))
    for b in range(nb):
        lo, hi = w * b, w * b + w
        L, Dinv = lu_nopivot(P[:, lo:hi, lo:hi])
        if w == 4:
            lu[:, b] = np.stack([L[:, i, k] for i, k in LU_SLOTS], axis=1)
        A = -P[:, :, lo:hi] @ Dinv
        A[:, lo:hi] = 0.0
        aop[:, b, perm] = A
        R = P[:, lo:hi, hi:].copy()
        P[:, :, hi:] += A @ R          # the pivot rows take += 0 and are replaced below
        P[:, lo:hi, hi:] = Dinv @ R
    return lu, aop


def multipliers(W, g):
    """the same as a list per matrix of (block step, kind, row, column, value), zero entries left out; kind "lu": row / column are the
    padded indices of the two pivots, kind "aop": row the padded index, column the pivot's padded index"""
    lu, aop = sweep(W, g)
    out = []
    for k in range(W.shape[0]):
        items = []
        for b, K in enumerate(g.blocks):
            items += [(b, "lu", int(K[i]), int(K[j]), float(lu[k, b, s])) for s, (i, j) in enumerate(LU_SLOTS[:lu.shape[2]]) if lu[k, b, s] != 0]
            rows, cols = np.nonzero(aop[k, b])
            items += [(b, "aop", int(r), int(K[c]), float(aop[k, b, r, c])) for r, c in zip(rows, cols)]
        out.append(items)
    return out


# ---- the constructions (W space) ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bases(dtype, n):
    """N_BASES base matrices (n, n), rounded to dtype, as float64; symmetric, so W space and A space agree"""
    b = spd_batch(n, N_BASES, seed=7000 + n, dtype=NP_DTYPES[dtype]).astype(np.float64).reshape(N_BASES, n, n)
    b.setflags(write=False)
    return b


def beyond(x, dtype):
    """the next number of dtype beyond x, away from zero"""
    t = NP_DTYPES[dtype]
    return float(np.nextafter(t(x), t(2 * x)))


def build(case, g):
    """the matrix of `case` in W space, float64 holding values of g.dtype exactly"""
    dt = g.dtype
    W = bases(dt, g.n)[case.base].copy()
    i, o = case.i, case.other
    big = REJECTED[case.variant] or case.kind == "BT"
    sign = 1.0 if case.variant in ("+4", ">+4") else -1.0   # of the tested value
    W[i, :] = 0.0
    W[:, i] = 0.0
    if case.kind == "A":
        W[i, i] = 0.25
        c = beyond(1.0, dt) if big else 1.0
        # LU multiplier: +c / delta; A-operand entry: -c / delta
        W[o, i] = sign * c if case.where == "lu" else -sign * c
        if case.sym:
            W[i, o] = W[o, i]
        return W
    W[o, :] = 0.0
    W[:, o] = 0.0
    W[o, o] = 1.0
    if case.sym:
        h = beyond(0.5, dt) if big else 0.5
        W[o, i] = W[i, o] = -sign * h
        W[i, i] = 0.375
    else:
        W[o, i] = -sign * (beyond(2.0, dt) if big else 2.0)
        W[i, o] = -sign * 0.5
        W[i, i] = 1.5
    if case.kind == "BT":
        W = W.T.copy()
    return W


def to_memory(Ws, g):
    """(B, n, n) W-space matrices -> the flat column-major batch the entry points take, in g.dtype"""
    A = Ws if g.transposed else Ws.transpose(0, 2, 1)  # tile kernels: W[i][j] = mem[i n + j]; gj_rowlane2: W = A, mem[c n + r]
    return np.ascontiguousarray(A).reshape(len(Ws), -1).astype(NP_DTYPES[g.dtype])


def expected_reject(case):
    return case.kind != "BT" and REJECTED[case.variant]


# ---- the lists ------------------------------------------------------------------------------------------------------------------------
def sweep_rank(g, p):
    return (int(g.step[p]), int(g.pivno[p]))


def row_in_tile(g, T, want_local, ok):
    """a real index of tile T whose tile-local index is want_local, or the next one (cyclically) that satisfies ok"""
    for d in range(16):
        hits = np.flatnonzero((g.tile[:g.n] == T) & (g.local[:g.n] == (want_local + d) % 16))
        if len(hits) and ok(int(hits[0])):
            return int(hits[0])
    return None


def positions(g):
    """[(priority, kind, i, other, where)]: priority 0 = what every list keeps however far it is thinned (the LU slots of the first, a
    middle and the last real block; every tile row from the first pivot on, its own included; every tile row up to the last pivot's), 1 = the rest"""
    n, w = g.n, g.w
    order = [int(p) for K in g.blocks for p in K if p < n]          # the real indices in sweep order
    tiles = sorted(set(int(t) for t in g.tile[:n]))
    first_tile, last_tile = tiles[0], tiles[-1]
    out = []
    # LU slots
    if w == 4:
        nb = len(g.blocks)
        for b in sorted({0, nb // 2, nb - 1}):
            K = g.blocks[b]
            out += [(0, "A", int(K[k]), int(K[i]), "lu") for i, k in LU_SLOTS if K[i] < n and K[k] < n]
    # pivots: every column of the first tile column, every real column of the last one, one per block elsewhere
    pivots = []
    for b, K in enumerate(g.blocks):
        real = [int(p) for p in K if p < n]
        T = int(g.tile[real[0]])
        pivots += real if T in (first_tile, last_tile) else [real[b % len(real)]]
    if w == 1:
        pivots = order
    for i in pivots:
        o = order.index(i)
        Ti, bi = int(g.tile[i]), int(g.step[i])
        prio_a = 0 if o == 0 else 1
        prio_b = 0 if i == order[-1] else 1
        after = lambda p: g.step[p] > bi           # noqa: E731  (another block: an A-operand entry)
        before = lambda p: g.step[p] < bi          # noqa: E731
        rows_a, rows_b = [], []
        for T in tiles:
            want = (5 * o + 3 * T) % 16
            if T > Ti:
                rows_a.append((prio_a, row_in_tile(g, T, want, after)))
            elif T < Ti:
                rows_b.append((prio_b, row_in_tile(g, T, want, before)))
            else:  # the pivot's own tile: a later and an earlier block of it
                rows_a.append((prio_a, row_in_tile(g, T, want, after)))
                rows_b.append((prio_b, row_in_tile(g, T, want, before)))
        if after(n - 1):
            rows_a.append((prio_a, n - 1))
        if w == 1:  # one row per lane and register half: the neighbours of the pivot make every row the offending one once
            rows_a += [(1, order[o + 1])] if o + 1 < n else []
            rows_b += [(1, order[o - 1])] if o > 0 else []
        seen = set()
        for pr, j in rows_a:
            if j is not None and ("A", j) not in seen:
                seen.add(("A", j))
                out.append((pr, "A", i, j, "aop"))
        for pr, r in rows_b:
            if r is not None and ("B", r) not in seen:
                seen.add(("B", r))
                out.append((pr, "B", i, r, "aop"))
    return out


# the two variants a position gets (one accepted, one rejected), in turn: both signs on both sides of the threshold
PATTERNS = (("+4", "<-4"), ("-4", ">+4"), ("+4", ">+4"), ("-4", "<-4"))


def list_cap(g):
    return int(min(LIST_CAP, max(LIST_FLOOR, WORK_CAP / g.N ** 3)))


@functools.lru_cache(maxsize=None)
def cases(dtype, n, solve=False):
    """the list of (dtype, n): a tuple of Case, accepted and rejected variants interleaved"""
    g = geo(dtype, n, solve)
    pos = positions(g)
    cap = list_cap(g)
    # the symmetric 64 x 64 fp64 input takes an arm of its own: there every position is built in both forms
    both_forms = dtype == "f64" and n == 64
    per_pos = 2 * (2 if both_forms else 1)
    must = [p for p in pos if p[0] == 0]
    rest = [p for p in pos if p[0] != 0]
    room = max(0, cap // per_pos - len(must))
    if len(rest) > room:
        stride = -(-len(rest) // max(room, 1))
        # a stride coprime to 16 and to the tile count walks through every tile-local row and tile row
        while np.gcd(stride, 16) != 1 or (len(set(g.tile[:n])) > 1 and stride % len(set(g.tile[:n])) == 0):
            stride += 1
        rest = rest[::stride] if room else []
    out = []
    for k, (_, kind, i, other, where) in enumerate(must + rest):
        forms = (False, True) if both_forms else ((k // 4) % 2 == 1,)
        for f, sym in enumerate(forms):
            for variant in PATTERNS[(k + f) % 4]:
                out.append(Case(kind, i, other, variant, sym, len(out) % N_BASES, where))
            if kind == "B" and not sym and (k % 3 == 0 or both_forms):
                # the transpose of the one-sided matrix beyond 4: accepted (largest multiplier nextafter(2, 3))
                out.append(Case("BT", i, other, PATTERNS[(k + f) % 4][1], False, len(out) % N_BASES, where))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def matrices(dtype, n, solve=False):
    """(W[B, n, n] float64, flat[B, n*n] in dtype as the entry points read it, reject[B] bool) of the list"""
    g = geo(dtype, n, solve)
    cs = cases(dtype, n, solve)
    W = np.stack([build(c, g) for c in cs])
    flat = to_memory(W, g)
    rej = np.array([expected_reject(c) for c in cs])
    for a in (W, flat, rej):
        a.setflags(write=False)
    return W, flat, rej


def intended(case, g):
    """(block step, kind, row, column) of the tested multiplier and the value it must have exactly (accept variants) or reach
    (reject variants: at least one ulp of the dtype beyond)"""
    sign = 1.0 if case.variant in ("+4", ">+4") else -1.0
    return (int(g.step[case.i]), case.where, case.other, case.i), sign * TAU


def thin(dtype, n, count):
    """`count` evenly spaced members of the list, as indices, accepted and rejected ones alike (the fused solve runs these)"""
    total = len(cases(dtype, n, True))
    return np.unique(np.linspace(0, total - 1, min(count, total)).astype(int))


SOLVE_SIZES = (17, 33, 64)
SOLVE_NRHS = 16


def case_text(c):
    return f"({c.kind}{'s' if c.sym else ''}, pivot {c.i}, row {c.other}, {c.variant})"
