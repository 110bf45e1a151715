"""Batches whose info code is known in advance: which column a kernel has to name for a matrix that is not positive definite
(Cholesky contract: leading minor k+1 not positive -> k+1) or singular (Gauss-Jordan contract: no usable pivot at step k -> k+1).
numpy only. tests/test_info_cases_cpu.py checks the expectations against the CPU oracle, tests/test_gpu_info_codes.py runs every
kernel route on them.

Base matrices: conftest.spd_batch (R + R^T + n I); for Gauss-Jordan spd_batch and general_batch alternate by matrix index, so that
both the natural-order-then-redo path and the direct pivoting path of a launch have to report. Memory order is [k, col, row].

  family  edit                                                 expected info
  C1      M[i,i] = -1,                      i in P(n)          i+1
  C2      M[j,j] = M[k,k] = -1,             (j,k) in Q(n)      j+1
  C3      M[j,k] = M[k,j] = 2 max diag M,   (j,k) in Q(n)      k+1   (every diagonal entry stays positive)
  G1      column i of A zero,               i in P(n)          i+1
  G2      columns j and k of A zero,        (j,k) in Q(n)      j+1 or k+1 (the oracle: j+1)

None of the edits touches the leading block before the expected column, whose pivots are far from zero (at least 0.25 of their
diagonal entry, measured 0.74 at n = 2 and 0.94 from n = 15), and the pivot at the expected column is at most -1 (C1, C2: -1 minus a
square; C3: M[k,k] - (2 max diag)^2 / pivot_j < -3 max diag): the expectation does not depend on the rounding or on the order of the
arithmetic of a kernel. Every batch also carries three untouched base matrices, in its first, a middle and its last slot.
"""
from collections import namedtuple

import numpy as np

from conftest import general_batch, spd_batch

TILE = 16
BOUNDARIES = (32, 64, 96, 128, 256, 512)
ALL_COLUMNS_MAX = 256  # up to here P(n) is every column
MAX_ELEMENTS = 40 * 1024 * 1024  # of one batch: 40 matrices of 1024 x 1024, or about 300 of 256 x 256 with room to spare
TILE_SAMPLE = ((0, 1), (1, 2), (1, 4), (3, 12), (4, 5), (14, 15))  # tile-local pairs kept where Q(n) has to be thinned
CHOL_FAMILIES, GJ_FAMILIES = ("C1", "C2", "C3"), ("G1", "G2")

# a: (batch, n, n) float64 in memory order [k, col, row]; expect: info per matrix (0 for the healthy ones); alt: the other admissible
# code (G2: k+1; equal to expect elsewhere); healthy: the three untouched slots; items: the position or pair of every other slot
Batch = namedtuple("Batch", "a expect alt healthy items")


def positions(n):
    """P(n): the columns at which a single defect is placed"""
    if n <= ALL_COLUMNS_MAX:
        return list(range(n))
    p = {0, 1, n - 2, n - 1}
    for b in BOUNDARIES:
        p.update(x for x in (b - 1, b) if x < n)
    p.update(((n - 1) // m) * m for m in (32, 64, 128))
    out = sorted(p)
    assert len(out) <= 40
    return out


def pairs(n):
    """Q(n): the pairs of columns j < k at which two defects are placed. Every pair inside the first and inside the last (possibly
    ragged) 16-column tile, (j, n-1) for j in 0, 15, 16, n-2, and beyond n = 256 the consecutive elements of P(n) -- as long as the
    batch stays within MAX_ELEMENTS (up to n of about 400). Beyond that size no kernel works on 16-column tiles any more (the MFMA tile
    families end at n = 256) and a batch of 260 matrices would cost seconds per launch: the pairs inside the two tiles are thinned to
    TILE_SAMPLE, which keeps neighbours, a pair across a block of four and pairs on which the two elimination orders differ."""
    first = range(min(TILE, n))
    last = range(TILE * ((n - 1) // TILE), n)  # the last, possibly ragged, tile
    q = {(j, n - 1) for j in (0, 15, 16, n - 2) if 0 <= j < n - 1}
    if n > ALL_COLUMNS_MAX:
        p = positions(n)
        q.update(zip(p, p[1:]))
    full = set(q)
    for tile in (first, last):
        full.update((j, k) for j in tile for k in tile if j < k)
        q.update((tile[0] + j, tile[0] + k) for j, k in TILE_SAMPLE if tile[0] + k < n)
    return sorted(full if (len(full) + 3) * n * n <= MAX_ELEMENTS else q)


def slots(count):
    """(batch, healthy slots, slots of the edited matrices) for `count` edited matrices"""
    batch = count + 3
    healthy = (0, batch // 2, batch - 1)
    return batch, healthy, [k for k in range(batch) if k not in healthy]


def gj_base(n, batch, seed):
    a = spd_batch(n, batch, seed=seed).reshape(batch, n, n).copy()
    a[1::2] = general_batch(n, batch, seed=seed + 1).reshape(batch, n, n)[1::2]
    return a


def build(family, n, seed=None):
    """the batch of one family at size n"""
    items = positions(n) if family in ("C1", "G1") else pairs(n)
    batch, healthy, where = slots(len(items))
    seed = 7000 + 10 * n + (CHOL_FAMILIES + GJ_FAMILIES).index(family) if seed is None else seed
    a = gj_base(n, batch, seed) if family in GJ_FAMILIES else spd_batch(n, batch, seed=seed).reshape(batch, n, n).copy()
    expect, alt = np.zeros(batch, dtype=np.int32), np.zeros(batch, dtype=np.int32)
    d = np.arange(n)
    for s, it in zip(where, items):
        if family == "C1":
            a[s, it, it] = -1.0
            expect[s] = alt[s] = it + 1
        elif family == "C2":
            j, k = it
            a[s, j, j] = a[s, k, k] = -1.0
            expect[s] = alt[s] = j + 1
        elif family == "C3":
            j, k = it
            a[s, j, k] = a[s, k, j] = 2.0 * a[s, d, d].max()
            expect[s] = alt[s] = k + 1
        elif family == "G1":
            a[s, it, :] = 0.0
            expect[s] = alt[s] = it + 1
        elif family == "G2":
            j, k = it
            a[s, j, :] = a[s, k, :] = 0.0
            expect[s], alt[s] = j + 1, k + 1
        else:
            raise ValueError(family)
    return Batch(a, expect, alt, healthy, items)


def split_diagonal(a, dtype, seed):
    """(B, c) in `dtype` with B + diag c = a up to one rounding of the diagonal, c drawn from U(0,1): the inputs of the routes that
    take M = B + diag c. For C1 and C2 the edited B[i,i] is -1 - c[i]."""
    batch, n, _ = a.shape
    c = np.random.default_rng(seed).random((batch, n)).astype(dtype)
    b = a.astype(dtype)
    d = np.arange(n)
    b[:, d, d] -= c
    return b, c


# ---- what the expectations rest on, and the emulation of the two elimination orders (float64, one matrix) ---------------------------
def as_rowcol(m):
    """memory order [col, row] -> [row, col]"""
    return m.T


def natural_pivots(m, upto):
    """the pivots (squares of the Cholesky diagonal) 0 .. upto of the matrix m[row, col] in natural order; the first `upto` must be
    positive"""
    if upto == 0:
        return np.array([m[0, 0]])
    lead = np.linalg.cholesky(m[:upto, :upto])
    y = np.linalg.solve(lead, m[:upto, upto])
    return np.append(np.diag(lead) ** 2, m[upto, upto] - y @ y)


def tile_schur(m, t0, t1):
    """the diagonal block [t0, t1) of m after the elimination of the columns before t0"""
    s = m[t0:t1, t0:t1].copy()
    if t0:
        s -= m[t0:t1, :t0] @ np.linalg.solve(m[:t0, :t0], m[:t0, t0:t1])
    return s


def natural_order(width):
    return list(range(width))


def permuted_order(width):
    """the order in which the fp32 MFMA tile kernels eliminate the columns of a 16-column tile of which `width` are real: block b holds
    the columns b, b + 4, b + 8, b + 12 (TileGeo<float>::pcol)"""
    return [4 * t + b for b in range(4) for t in range(4) if 4 * t + b < width]


def first_failure(s, order):
    """tile-local column of the first non-positive pivot when the columns of the symmetric block s are eliminated in `order` (-1: none)"""
    s = s.copy()
    for p in order:
        piv = s[p, p]
        if not piv > 0:
            return p
        s -= np.outer(s[:, p], s[p, :]) / piv
    return -1
