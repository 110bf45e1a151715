"""Matrices whose correct pivot row is known in advance at every elimination step, a numpy model of Gauss-Jordan with partial pivoting
that shows what a search that misses that row costs, and the lists tests/test_pivot_cases_cpu.py checks and
tests/test_gpu_pivot_search.py runs. numpy only.

Construction. For a permutation pi of 0 .. n-1:  A[pi(k), :] = M[k, :],  M = diag(D) + delta R,  |D_k| in [0.5, 2] with random signs,
R with a zero diagonal and off-diagonal magnitudes in [0.5, 1] with random signs (bounded away from 0: a decoy near 0 makes the
second-best candidate, and with it the damage of a wrong choice, arbitrary). At step k exactly one unused row, pi(k), holds a candidate of
order 1, every other candidate is of order delta: a correct search forms no multiplier above about delta, a search that misses row
pi(k) ONCE forms multipliers of about 1 / delta. cond(A) < 5. Every case comes as A and as A^T (column pi(k) of A^T holds its order-1
entry at row k: the pivot order of A^T is pi^-1), because the TILEP kernels eliminate A^T and TILEQ searches columns of the transpose.
det A = parity(pi) prod D_k up to a factor 1 + O(n delta^2), which pins the sign of the log-determinant.

delta (DELTA below) is the member of the ladder 2^-16 .. 2^-28 (fp64) / 2^-8 .. 2^-14 (fp32) at which the smallest error of a
one-step sabotage, in units of the parity bound, is largest (tests/test_pivot_cases_cpu.py: test_delta_is_the_best_of_its_ladder runs
the ladder over every case and step of the sizes LADDER_SIZES, those up to 49 and 100; test_clean_and_sabotaged holds every case of
every size of ALL_SIZES to the conditions at the chosen value).
Measured with the model below, every case of every size of ALL_SIZES, every step k < n - 1 sabotaged in turn (the second-best candidate taken):

    fp64  delta = 2^-28   largest clean error / bound 6.1e-06 (n = 192)   smallest sabotaged error / bound 2.6e+03 (n = 192), median 3e+05
    fp32  delta = 2^-13   largest clean error / bound 1.1e-02 (n = 256)   smallest sabotaged error / bound 227 (n = 8), median 1.3e+04

(bound: max(1e-10, 1e-15 cond n) in fp64, 1e-5 cond in fp32, on the elementwise measure of tests/test_gpu_parity.py). The ladder, on
LADDER_SIZES, smallest sabotaged error / bound: fp64 2^-16 0.013, 2^-18 0.018, 2^-20 0.31, 2^-22 0.46, 2^-24 10,
2^-26 17, 2^-28 2.7e+03; fp32 2^-8 0.77, 2^-9 1.4, 2^-10 1.8, 2^-11 1.4, 2^-12 2.4, 2^-13 227, 2^-14 123. The damage of a wrong
choice grows like 1 / delta; the smallest value of a rung is that of its least sensitive (case, step), and only at the last rungs is
every step caught by a wide margin. The sizes outside LADDER_SIZES run at the chosen value only: that the ranking of the rungs holds
there was not checked. The floor the CPU test asserts is 1/8 and 8; RESEED lists the cases whose D and R had
to be drawn from another seed to meet it (none at these values).

Permutations of a size (perms): the identity (the control: the natural-order kernels accept it), the reversal, cyclic shifts by
1 .. 15, 16 and n - 16, the rotation by 4 inside each 16-row tile, the 4 x 4 transposition inside each tile (the fp32 `trow` order),
single transpositions across tiles and lane groups, three seeded random permutations, and `fill` permutations generated until the
coverage conditions hold (coverage): every pair (k mod 16, pi(k) mod 16), every pair (tile column of k, tile row of pi(k)), every k with
its pivot inside and outside its own block of four rows, both parities. For ragged n the tile-local maps are restricted to the rows
that exist (the images that remain, in their order). Lists of n > THIN_ABOVE keep every THIN_STRIDE-th of the shifts and are filled
up afterwards, so the conditions hold for them as well."""
import collections
import concurrent.futures
import functools
import re

import numpy as np

from conftest import pkg

NP_DTYPES = {"f64": np.float64, "f32": np.float32}
LADDER = {"f64": tuple(2.0 ** -e for e in range(16, 30, 2)), "f32": tuple(2.0 ** -e for e in range(8, 15))}
DELTA = {"f64": 2.0 ** -28, "f32": 2.0 ** -13}
THIN_ABOVE, THIN_STRIDE = 64, 3
FLOOR = 8.0
# (dtype, n, index of the permutation, orientation) -> seed of D and R where seed 0 misses the 1/8 or the 8 (found by
# tests/test_pivot_cases_cpu.py: reseed_table)
RESEED = {}

# literal so that collecting the GPU test does not load the library; sizes() derives them and the CPU test compares
SIZES = {"f64": (2, 8, 9, 16, 17, 25, 26, 32, 33, 48, 49, 64, 65, 80, 97, 112, 128, 129, 144, 192),
         "f32": (2, 8, 9, 16, 17, 25, 26, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128, 129, 144, 256)}
FORCED_SIZES = {"row": (2, 33, 64), "lds": (2, 33, 100), "global": (2, 33, 100), "blocked": (2, 33, 100, 159, 160)}   # both dtypes
FORCED = ("row", "lds", "global", "blocked")
# every size that has a list: what the CPU test holds to the conditions at every step and the GPU workers run
ALL_SIZES = {dt: tuple(sorted(set(SIZES[dt]) | {n for ns in FORCED_SIZES.values() for n in ns})) for dt in SIZES}
LADDER_SIZES = {dt: tuple(n for n in ALL_SIZES[dt] if n <= 49 or n == 100) for dt in SIZES}

Perm = collections.namedtuple("Perm", "label pi")
Case = collections.namedtuple("Case", "label index orient identity")   # orient: "A" or "T"


def api():
    return pkg("api")


# ---- sizes, from the route functions ----------------------------------------------------------------------------------------------------
def _shape(name):
    """one key per kernel shape: the rowlane kernels by register width, gj_tile / gj_tilep by tile count, gj_tile4 as
    _accept_cases.shape_of has it (by wave count, one wave per tile column as one shape), the kernels of several waves by family"""
    import _accept_cases
    natural = _accept_cases.shape_of(name)
    if natural is not None:
        return natural[1]
    m = re.match(r"matinv_(\w+)<([^>]*)>", name)
    family, args = re.sub(r"_f\d+$", "", m.group(1)), [a.strip() for a in m.group(2).split(",")]
    if family == "gj_rowlane":
        return family, int(args[1])
    return (family, int(args[0])) if family == "gj_tilep" else (family,)


@functools.lru_cache(maxsize=None)
def auto_route(dtype):
    """{n: (AUTO kernel name, pivoting kernel name)} for every n whose AUTO Gauss-Jordan route searches pivots in a rowlane or tile
    kernel: up to the last n KERNEL_TILEP serves"""
    a = api()
    code = a.F64 if dtype == "f64" else a.F32
    out = {}
    for n in range(2, 1025):
        auto = a.kernel_name(a.ALGO_GAUSS_JORDAN, code, n, a.KERNEL_AUTO)
        piv = a.kernel_name(a.ALGO_GAUSS_JORDAN, code, n, a.KERNEL_TILEP)
        if not piv and n > 16:
            break
        out[n] = (auto, piv or auto)
    return out


@functools.lru_cache(maxsize=None)
def sizes(dtype):
    """per distinct (AUTO kernel, pivoting kernel behind it) the smallest ragged and the smallest full n (rowlane widths: the smallest
    n), and the last n of the rowlane kernels, of TILEP, TILEP4 and TILEQ"""
    import _accept_cases
    route = auto_route(dtype)
    by_shape = {}
    for n, names in route.items():
        for x in names:
            by_shape.setdefault(_shape(x), []).append(n)
    picked = set(_accept_cases.sizes(dtype))
    for key, ns in by_shape.items():
        ragged = [n for n in ns if n % 16]
        full = [n for n in ns if n % 16 == 0]
        picked.update([min(ragged)] if ragged else [])
        picked.update([min(full)] if full else [])
        if key[0] == "gj_rowlane":
            picked.add(max(ns))
    # the last n of TILEP (one wave), of the kernels of several waves below TILEQ, and of TILEQ
    first_q = min(n for n, names in route.items() if "tileq" in names[1])
    first_p4 = min(n for n, names in route.items() if "gj_tilep_" not in names[1])
    picked.update((first_p4 - 1, first_q - 1, max(route)))
    return tuple(sorted(picked))


@functools.lru_cache(maxsize=None)
def forced_sizes(dtype, family):
    """the first n with more than one row that a forced family serves (each serves n = 1, which has no search), n = 33 (ragged, past
    the 32-column panel of the blocked scheme) and one more that is small enough for a few seconds: 100, or the family's last n where
    that is smaller; BLOCKED also either side of its two-level threshold"""
    a = api()
    code = a.F64 if dtype == "f64" else a.F32
    fam = {"row": a.KERNEL_ROW, "lds": a.KERNEL_LDS, "global": a.KERNEL_GLOBAL, "blocked": a.KERNEL_BLOCKED}[family]
    served = [n for n in range(2, 1025) if a.kernel_name(a.ALGO_GAUSS_JORDAN, code, n, fam)]
    out = {served[0], min(33, served[-1]), min(100, served[-1])}
    if family == "blocked":
        t = min(n for n in served if "update_mfma" in a.kernel_name(a.ALGO_GAUSS_JORDAN, code, n, fam))
        out.update((t - 1, t))
    return tuple(sorted(out))


# ---- permutations ----------------------------------------------------------------------------------------------------------------------
def _restrict(images, n):
    """a map given by its images, restricted to 0 .. n-1: the images that remain, in their order"""
    images = np.asarray(images)[:n]
    return np.argsort(np.argsort(images, kind="stable"), kind="stable")


def _tile_local(n, f):
    """the permutation that applies f (a map of 0 .. 15) inside every 16-row tile, restricted to the rows that exist"""
    pi = np.empty(n, int)
    for t in range(0, n, 16):
        m = min(16, n - t)
        pi[t:t + m] = t + _restrict([f(j) for j in range(16)], m)
    return pi


def parity(pi):
    """+1 / -1"""
    seen, sign = np.zeros(len(pi), bool), 1
    for i in range(len(pi)):
        length = 0
        while not seen[i]:
            seen[i], i, length = True, pi[i], length + 1
        if length and length % 2 == 0:
            sign = -sign
    return sign


def coverage(n, pis):
    """what a list of permutations leaves uncovered, named: {"residue": pairs (k % 16, pi(k) % 16), "tile": pairs (k // 16, pi(k) // 16),
    "inside": the k never pivoted inside their own block of four, "outside": never outside it, "parity": the signs missing}; and
    "absent": the positions n does not have (residues >= n; k whose block of four holds no other row)"""
    res, tile = np.zeros((16, 16), bool), np.zeros((-(-n // 16),) * 2, bool)
    inside, outside, signs = np.zeros(n, bool), np.zeros(n, bool), set()
    k = np.arange(n)
    for pi in pis:
        res[k % 16, pi % 16] = True
        tile[k // 16, pi // 16] = True
        inside |= pi // 4 == k // 4
        outside |= pi // 4 != k // 4
        signs.add(parity(pi))
    have = sorted(set(k % 16))
    return {"residue": [(a, b) for a in have for b in have if not res[a, b]],
            "tile": [(int(a), int(b)) for a, b in zip(*np.nonzero(~tile))],
            "inside": np.flatnonzero(~inside).tolist(),
            "outside": np.flatnonzero(~outside).tolist() if n > 4 else [],
            "parity": sorted({1, -1} - signs) if n > 1 else [],
            "absent": {"residue": [r for r in range(16) if r not in have], "outside": list(range(n)) if n <= 4 else []}}


def _fill(n, miss):
    """one permutation that takes as many of the missing (residue pair, tile pair, outside) positions as fit, the rows left over in rotated order"""
    pi, free = np.full(n, -1), np.ones(n, bool)

    def put(ks, rs):
        for k in ks:
            if pi[k] < 0:
                for r in rs:
                    if free[r]:
                        pi[k], free[r] = r, False
                        return

    for a, b in miss["residue"]:
        put(range(a, n, 16), range(b, n, 16))
    for a, b in miss["tile"]:
        put(range(16 * a, min(n, 16 * a + 16)), range(16 * b, min(n, 16 * b + 16)))
    for k in miss["outside"]:
        put([k], [r for r in range(n) if r // 4 != k // 4])
    for k in miss["inside"]:
        put([k], [r for r in range(n) if r // 4 == k // 4])
    pi[pi < 0] = np.roll(np.flatnonzero(free), 1)  # rotated by one: never the identity
    return pi


@functools.lru_cache(maxsize=None)
def perms(n):
    """the list of a size: tuple of Perm, the identity first"""
    k = np.arange(n)
    out = [Perm("identity", k.copy()), Perm("reversal", k[::-1].copy())]
    shifts = sorted({s for s in list(range(1, 17)) + [n - 16] if 0 < s < n})
    if n > THIN_ABOVE:
        shifts = sorted(set(shifts[::THIN_STRIDE]) | {s for s in (16, n - 16) if 0 < s < n})
    out += [Perm(f"shift{s}", (k + s) % n) for s in shifts]
    out.append(Perm("rot4", _tile_local(n, lambda j: (j + 4) % 16)))
    out.append(Perm("trow", _tile_local(n, lambda j: 4 * (j % 4) + j // 4)))
    # single transpositions: i in one tile, j in another (the last, and every tile in between for i's partner), another lane group
    pairs = []
    for t in range(1, -(-n // 16)):
        i = (5 * t + 1) % 16 + 16 * ((t - 1) // 2)
        j = min(n - 1, 16 * t + (i % 16 + 6) % 16)
        if j // 16 != i // 16 and (j % 16) // 4 == (i % 16) // 4:
            j -= 4
        pairs.append((i, j))
    if n <= 16:
        pairs = [(0, n - 1)] + ([(1, n // 2 + 1)] if n >= 8 else [])
    if n > THIN_ABOVE:
        pairs = pairs[::max(1, len(pairs) // 3)][:3]
    for i, j in pairs:
        pi = k.copy()
        pi[i], pi[j] = j, i
        out.append(Perm(f"swap{i}_{j}", pi))
    rng = np.random.default_rng(4000 + n)
    out += [Perm(f"random{r}", rng.permutation(n)) for r in range(3)]
    for r in range(64):
        miss = coverage(n, [p.pi for p in out[1 if n > 2 else 0:]])  # the identity does not count: the AUTO run leaves it out
        if not any(miss[key] for key in ("residue", "tile", "inside", "outside", "parity")):
            break
        pi = _fill(n, miss)
        if miss["parity"] and not (miss["residue"] or miss["tile"]) and n > 1:
            pi = k.copy()
            pi[0], pi[n - 1] = n - 1, 0
        out.append(Perm(f"fill{r}", pi))
    seen, uniq = set(), []
    for p in out:
        assert sorted(p.pi) == list(range(n)), p.label
        if p.pi.tobytes() not in seen:
            seen.add(p.pi.tobytes())
            uniq.append(p)
    for p in uniq:
        p.pi.setflags(write=False)
    return tuple(uniq)


@functools.lru_cache(maxsize=None)
def cases(n):
    """every permutation as A and as A^T; the identity members first"""
    return tuple(Case(p.label, i, o, p.label == "identity") for i, p in enumerate(perms(n)) for o in ("A", "T"))


# ---- the matrices ----------------------------------------------------------------------------------------------------------------------
def build(dtype, n, index, orient, delta=None, seed=None):
    """(matrix (n, n) in the working dtype, D): the case of perms(n)[index]"""
    delta = DELTA[dtype] if delta is None else delta
    seed = RESEED.get((dtype, n, index, orient), 0) if seed is None else seed
    rng = np.random.default_rng([seed, n, index])
    D = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    R = rng.uniform(0.5, 1.0, (n, n)) * rng.choice([-1.0, 1.0], (n, n))
    np.fill_diagonal(R, 0.0)
    A = np.empty((n, n))
    A[perms(n)[index].pi] = np.diag(D) + delta * R
    if orient == "T":
        A = A.T
    return np.ascontiguousarray(A.astype(NP_DTYPES[dtype])), D


@functools.lru_cache(maxsize=None)
def matrices(dtype, n):
    """(mats[B, n, n] in dtype, flat[B, n*n] as the entry points read it (column-major), order[B, n]: the pivot row of every step,
    sign[B]: the sign of the determinant, identity[B] bool) of cases(n)"""
    cs = cases(n)
    built = [build(dtype, n, c.index, c.orient) for c in cs]
    mats = np.stack([b[0] for b in built])
    flat = np.ascontiguousarray(mats.transpose(0, 2, 1)).reshape(len(cs), -1)
    order = np.stack([perms(n)[c.index].pi if c.orient == "A" else np.argsort(perms(n)[c.index].pi) for c in cs])
    sign = np.array([parity(perms(n)[c.index].pi) * np.prod(np.sign(b[1])) for c, b in zip(cs, built)])
    ident = np.array([c.identity for c in cs])
    for a in (mats, flat, order, sign, ident):
        a.setflags(write=False)
    return mats, flat, order, sign, ident


def case_text(n, c):
    return f"({c.label}{'^T' if c.orient == 'T' else ''}, n={n})"


# ---- error measure and bounds: those of tests/test_gpu_parity.py at the matrix's own condition number -----------------------------------
def reference(mats):
    """(float64 inverses [B, n, n], 2-norm condition numbers) of the float64 image of the matrices as stored"""
    a = np.asarray(mats, dtype=np.float64)
    return np.linalg.inv(a), np.linalg.cond(a)


def bound(dtype, cond, n):
    return np.maximum(1e-10, 1e-15 * cond * n) if dtype == "f64" else 1e-5 * cond


def elementwise(got, want):
    """max |x - y| / max(|y|, 1e-3 max |Y|) per matrix; got, want [B, n, n] (or [B, anything])"""
    got = np.asarray(got, dtype=np.float64).reshape(len(want), -1)
    want = want.reshape(len(want), -1)
    floor = 1e-3 * np.abs(want).max(axis=1, keepdims=True)
    return (np.abs(got - want) / np.maximum(np.abs(want), floor)).max(axis=1)


# ---- the model: Gauss-Jordan with partial pivoting in the working dtype ------------------------------------------------------------------
PANEL = 16


class State:
    """[A | I] of a batch under elimination without row exchanges: L (B, n, n), R (B, n, n), used (B, n), order (B, n), second (B, n):
    second-largest / largest candidate of every step"""

    def __init__(self, mats):
        B, n, _ = mats.shape
        self.L, self.R = mats.copy(), np.broadcast_to(np.eye(n, dtype=mats.dtype), mats.shape).copy()
        self.used, self.order, self.second = np.zeros((B, n), bool), np.zeros((B, n), int), np.zeros((B, n))

    def take(self, idx):
        s = State.__new__(State)
        s.L, s.R, s.used, s.order, s.second = (x[idx].copy() for x in (self.L, self.R, self.used, self.order, self.second))
        return s


def run(state, sab, start=0, snapshots=None):
    """Eliminate columns start .. n-1 of `state` in place, a panel of PANEL columns at a time (the columns outside the panel take the
    panel's steps as one product). The pivot of a step is the largest candidate among the rows not used yet; item b takes the
    SECOND largest at step sab[b] (-1: never). snapshots: a dict that receives a copy of the state before every panel, by column.
    Returns the inverses (B, n, n)."""
    L, R, used, order = state.L, state.R, state.used, state.order
    B, n, _ = L.shape
    ar = np.arange(B)
    for c in range(start, n, PANEL):
        if snapshots is not None:
            snapshots[c] = state.take(ar)
        w = min(PANEL, n - c)
        P = L[:, :, c:c + w].copy()
        T = np.zeros((B, n, w), L.dtype)
        rows = np.zeros((B, w), int)
        for j in range(w):
            cand = np.abs(P[:, :, j]).astype(np.float64)
            cand[used] = -1.0
            p = cand.argmax(axis=1)
            best = cand[ar, p]
            cand[ar, p] = -1.0
            q = cand.argmax(axis=1)
            state.second[:, c + j] = np.maximum(cand[ar, q], 0.0) / best
            wrong = sab == c + j
            p = np.where(wrong, q, p)
            used[ar, p], order[:, c + j], rows[:, j] = True, p, p
            T[ar, p, j] = 1.0
            piv = P[ar, p, j][:, None]
            prow, trow = P[ar, p, :] / piv, T[ar, p, :] / piv
            f = P[:, :, j].copy()
            f[ar, p] = 0.0
            # columns before j of P are eliminated already (zero in every row still unused), columns after j of T are not begun
            P[:, :, j:] -= f[:, :, None] * prow[:, None, j:]
            T[:, :, :j + 1] -= f[:, :, None] * trow[:, None, :j + 1]
            P[ar, p, :], T[ar, p, :] = prow, trow
        at = ar[:, None]
        for X in (L[:, :, c + w:], R):
            if X.shape[2]:
                Y = T @ X[at, rows, :]
                X += Y
                X[at, rows, :] = Y[at, rows, :]
    return R[ar[:, None], order, :]


def clean_and_sabotaged(mats, want, chunk=8, threads=4):
    """(elementwise error of the clean run [B], clean pivot order [B, n], second / best candidate [B, n], elementwise error of the
    sabotaged runs [B, n-1]: step k of item b taking its second-best candidate) against the reference inverses `want`.
    The sabotaged runs of a panel start from the clean state before that panel. Chunks of the batch run on a few threads (the work is
    numpy's, which releases the interpreter lock); the result does not depend on how the batch is cut."""
    B, n, _ = mats.shape
    clean, order, second = np.empty(B), np.empty((B, n), int), np.empty((B, n))
    bad = np.empty((B, max(n - 1, 0)))

    def one(lo):
        st, snaps = State(mats[lo:lo + chunk]), {}
        b = len(st.L)
        clean[lo:lo + b] = elementwise(run(st, np.full(b, -1), snapshots=snaps), want[lo:lo + b])
        order[lo:lo + b], second[lo:lo + b] = st.order, st.second
        for c, snap in snaps.items():
            steps = np.arange(c, min(c + PANEL, n - 1))
            if len(steps):
                fork = snap.take(np.repeat(np.arange(b), len(steps)))
                got = run(fork, np.tile(steps, b), start=c)
                bad[lo:lo + b, steps] = elementwise(got, np.repeat(want[lo:lo + b], len(steps), axis=0)).reshape(b, len(steps))

    def quiet(lo):
        with np.errstate(all="ignore"):  # a sabotaged run may overflow; numpy's error state is per thread
            one(lo)

    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(quiet, range(0, B, chunk)))
    return clean, order, second, bad
