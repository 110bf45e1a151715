"""The batches of tests/_info_cases.py against the CPU oracle: the expected info codes are the ones a natural-order elimination gives,
in both roundings; the margins that make them independent of the rounding hold; and the pairs have teeth -- an elimination in the
order of the fp32 MFMA tile kernels names another column than the natural order for some of them. No GPU."""
import numpy as np
import pytest

import _info_cases as ic
import oracle

SIZES = (1, 2, 15, 16, 17, 33, 64, 100, 192, 256, 300)
DTYPES = (np.float64, np.float32)


def test_positions_and_pairs():
    for n in (1, 2, 16, 17, 100, 256):
        assert ic.positions(n) == list(range(n))
    for n in (257, 300, 513, 1000, 1024):
        p = ic.positions(n)
        assert len(p) <= 40 and p == sorted(set(p)) and 0 <= p[0] and p[-1] == n - 1
        must = {0, 1, n - 2, n - 1} | {x for b in ic.BOUNDARIES for x in (b - 1, b) if x < n}
        must |= {max(x for x in range(0, n, m)) for m in (32, 64, 128)}
        assert must <= set(p), (n, sorted(must - set(p)))
    assert {960, 992, 896} <= set(ic.positions(1024)) and {288, 256} <= set(ic.positions(300))
    assert ic.pairs(1) == []
    assert ic.pairs(2) == [(0, 1)]
    q = set(ic.pairs(40))
    assert {(j, k) for j in range(16) for k in range(16) if j < k} <= q
    assert {(j, k) for j in range(32, 40) for k in range(32, 40) if j < k} <= q
    assert {(0, 39), (15, 39), (16, 39), (38, 39)} <= q
    p = ic.positions(300)
    assert set(zip(p, p[1:])) <= set(ic.pairs(300))
    for n in SIZES + (384, 512, 1024):
        q = ic.pairs(n)
        assert all(0 <= j < k < n for j, k in q) and q == sorted(set(q))
        assert (len(q) + 3) * n * n <= ic.MAX_ELEMENTS and (len(ic.positions(n)) + 3) * n * n <= ic.MAX_ELEMENTS
        tiles = [(j, k) for t0 in (0, ic.TILE * ((n - 1) // ic.TILE)) for j in range(t0, min(t0 + 16, n)) for k in range(j + 1, min(t0 + 16, n))]
        assert (set(tiles) <= set(q)) == (n <= 384), n
    # where the pairs inside the two tiles are thinned: the sample in both tiles, everything else of Q(n) kept
    p, q = ic.positions(1024), set(ic.pairs(1024))
    assert set(zip(p, p[1:])) | {(0, 1023), (15, 1023), (16, 1023), (1022, 1023)} <= q
    assert {(t0 + j, t0 + k) for t0 in (0, 1008) for j, k in ic.TILE_SAMPLE} <= q


@pytest.mark.parametrize("family", ic.CHOL_FAMILIES + ic.GJ_FAMILIES)
@pytest.mark.parametrize("n", SIZES)
def test_layout_of_a_batch(n, family):
    b = ic.build(family, n)
    batch = len(b.a)
    assert b.healthy == (0, batch // 2, batch - 1) and batch == len(b.items) + 3
    assert not b.expect[list(b.healthy)].any()
    edited = np.delete(np.arange(batch), b.healthy)
    assert (b.expect[edited] > 0).all() and (b.expect <= n).all() and (b.alt >= b.expect).all()
    if family in ic.CHOL_FAMILIES:
        assert np.array_equal(b.a, b.a.transpose(0, 2, 1)), "a Cholesky batch is symmetric"
    if family == "C3":
        d = np.arange(n)
        assert (b.a[:, d, d] > 0).all(), "C3 is indefinite through an off-diagonal entry only"


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("n", SIZES)
def test_oracle_reports_the_expected_codes(n, dtype):
    for family in ic.CHOL_FAMILIES:
        b = ic.build(family, n)
        _, info = oracle.inverse_batched(b.a.astype(dtype).reshape(-1), n, oracle.ALGO_CHOLESKY)
        assert np.array_equal(info, b.expect), (family, [(k, g, w) for k, (g, w) in enumerate(zip(info, b.expect)) if g != w][:10])
    for family in ic.GJ_FAMILIES:
        b = ic.build(family, n)
        _, info = oracle.inverse_batched(b.a.astype(dtype).reshape(-1), n, oracle.ALGO_GJ_PIVOT)
        assert np.array_equal(info, b.expect), (family, [(k, g, w) for k, (g, w) in enumerate(zip(info, b.expect)) if g != w][:10])


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("n", SIZES)
def test_margins_that_make_the_codes_independent_of_rounding(n, dtype):
    """float64 pivots of the (rounded) input: at least 0.25 of their diagonal entry before the expected column, at most -1 at it"""
    smallest = np.inf
    for family in ic.CHOL_FAMILIES:
        b = ic.build(family, n)
        a = b.a.astype(dtype).astype(np.float64)
        for k in range(len(a)):
            m = ic.as_rowcol(a[k])
            e = b.expect[k] - 1 if b.expect[k] else n - 1
            piv = ic.natural_pivots(m, e)
            lead = piv if not b.expect[k] else piv[:-1]
            if len(lead):
                ratio = (lead / np.diag(m)[:len(lead)]).min()
                smallest = min(smallest, ratio)
                assert ratio >= 0.25, (family, k, ratio)
            if b.expect[k]:
                assert piv[-1] <= -1.0, (family, k, piv[-1])
    print(f"  n={n} {np.dtype(dtype).name}: smallest pivot / diagonal before the expected column = {smallest:.3f}")


@pytest.mark.parametrize("n", [n for n in SIZES if n >= 5])
def test_pairs_have_teeth(n):
    """for some pairs of C2 and of C3 the elimination order of the fp32 tile kernels meets its first non-positive pivot at another
    column than the natural order does: a kernel that reports in its own order is caught"""
    for family in ("C2", "C3"):
        b = ic.build(family, n)
        where = np.delete(np.arange(len(b.a)), b.healthy)
        differ = agree = 0
        for k, (j, kk) in zip(where, b.items):
            t0 = ic.TILE * (j // ic.TILE)
            if kk // ic.TILE != j // ic.TILE:
                continue
            t1 = min(t0 + ic.TILE, n)
            s = ic.tile_schur(ic.as_rowcol(b.a[k]), t0, t1)
            nat = ic.first_failure(s, ic.natural_order(t1 - t0))
            per = ic.first_failure(s, ic.permuted_order(t1 - t0))
            assert t0 + nat + 1 == b.expect[k], (family, j, kk, nat)
            assert per >= 0, "the same tile fails in either order"
            differ += per != nat
            agree += per == nat
        print(f"  n={n} {family}: {differ} pairs on which the two orders differ, {agree} on which they agree")
        assert differ > 0 and agree > 0, (family, differ, agree)


def test_split_diagonal_adds_up():
    for dtype in DTYPES:
        b = ic.build("C1", 17)
        B, c = ic.split_diagonal(b.a, dtype, seed=3)
        assert B.dtype == dtype and c.dtype == dtype and ((0 <= c) & (c < 1)).all()
        d = np.arange(17)
        m = B.copy()
        m[:, d, d] += c
        assert np.allclose(m, b.a.astype(dtype), rtol=4 * np.finfo(dtype).eps, atol=0)
        edited = np.delete(np.arange(len(b.a)), b.healthy)
        assert np.allclose(B[edited, b.expect[edited] - 1, b.expect[edited] - 1], -1 - c[edited, b.expect[edited] - 1], rtol=1e-6)
