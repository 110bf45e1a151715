"""CPU half of the threshold coverage (tests/test_gpu_accept.py, tests/_accept_worker.py): the lists of tests/_accept_cases.py are what
the GPU test takes them for. A float64 model of the natural-order sweep shows, for every member, the intended multiplier at the intended
(block step, kind, row, column), exactly +-4 or at least one ulp of the working dtype beyond, and every other multiplier <= 2; every
member is well conditioned and inverted by the CPU oracle's pivoting Gauss-Jordan; the lists cover the positions they claim to; and the
constants and orderings the model copies from csrc/ are still there."""
import os
import re

import numpy as np
import pytest

import _accept_cases as A
import _accept_worker as AW
import oracle
from conftest import as_mats, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-matrix-inversion_amd", "csrc")
LISTS = [(dt, n) for dt in ("f64", "f32") for n in A.SIZES[dt]]
SOLVE_LISTS = [(dt, n) for dt in ("f64", "f32") for n in A.SOLVE_SIZES]


def test_sizes_follow_the_route():
    """fp64: the sizes the lists were designed for; both dtypes: what the worker names and groups"""
    assert A.sizes("f64") == (17, 25, 26, 32, 33, 48, 49, 64, 65, 80, 97, 112, 129, 144, 192)
    assert {dt: A.sizes(dt) for dt in ("f64", "f32")} == A.SIZES
    for dt in ("f64", "f32"):
        assert sorted(AW.EXPECT[dt]) == list(A.sizes(dt)) == sorted(n for g in AW.GROUPS[dt].values() for n in g)
        for n in A.sizes(dt):
            assert A.route(dt)[n].startswith("matinv_" + AW.EXPECT[dt][n]), (dt, n, A.route(dt)[n])
        # the shapes: gj_rowlane2 in both register widths, gj_tile with 2, 3, 4 tiles, gj_tile4 on few waves and on one wave per tile column
        keys = {A.shape_of(A.route(dt)[n])[1] for n in A.sizes(dt)}
        assert {("rowlane2", 24), ("rowlane2", 32), ("tile", 2), ("tile", 3), ("tile", 4), ("tile4", 2), ("tile4", 4), ("tile4", "NT")} <= keys
    assert ("tile4", 1) in {A.shape_of(A.route("f32")[n])[1] for n in A.sizes("f32")}
    import test_gpu_accept as G
    assert sorted(G.GROUPS) == sorted((dt, g) for dt in AW.GROUPS for g in AW.GROUPS[dt])


def check_list(dtype, n, solve):
    g = A.geo(dtype, n, solve)
    cs = A.cases(dtype, n, solve)
    W, flat, rej = A.matrices(dtype, n, solve)
    eps = A.EPS[dtype]
    assert 0 < len(cs) <= A.LIST_CAP and len(cs) * g.N ** 3 <= 4 * A.WORK_CAP
    # the model runs on the float64 image of exactly what the entry point reads
    image = flat.astype(np.float64).reshape(len(cs), n, n)
    seen = image if g.transposed else image.transpose(0, 2, 1)
    assert np.array_equal(seen, W), "a constructed value is not exact in the working dtype"
    assert len({m.tobytes() for m in flat}) == len(cs)
    lu, aop = A.sweep(seen.copy(), g)
    for k, c in enumerate(cs):
        (b, kind, row, col), val = A.intended(c, g)
        assert g.step[row] >= 0 and (g.step[row] == b) == (kind == "lu")
        if kind == "lu":
            s = A.LU_SLOTS.index((int(g.pivno[row]), int(g.pivno[col])))
            got, lu[k, b, s] = lu[k, b, s], 0.0
        else:
            t = int(g.pivno[col])
            got, aop[k, b, row, t] = aop[k, b, row, t], 0.0
        if c.kind == "BT":
            assert abs(got) <= 2.0, (A.case_text(c), got)
        elif A.REJECTED[c.variant]:
            assert got * np.sign(val) >= A.TAU * (1 + eps), (A.case_text(c), got)
        else:
            assert got == val, (A.case_text(c), got)
    worst = np.maximum(np.abs(lu).reshape(len(cs), -1).max(axis=1, initial=0.0), np.abs(aop).reshape(len(cs), -1).max(axis=1))
    for k, c in enumerate(cs):
        # the transpose of a one-sided matrix beyond 4 carries nextafter(2, 3) and nothing larger
        assert worst[k] <= (A.beyond(2.0, dtype) if c.kind == "BT" else 2.0), (A.case_text(c), worst[k])
    assert rej.tolist() == [c.kind != "BT" and A.REJECTED[c.variant] for c in cs]
    return g, cs, flat


@pytest.mark.parametrize("dtype,n", LISTS, ids=lambda v: str(v))
def test_model_shows_the_intended_multiplier_and_nothing_else(dtype, n):
    g, cs, flat = check_list(dtype, n, False)
    a = as_mats(flat.astype(np.float64), n)
    cond = np.linalg.cond(a)
    assert np.isfinite(cond).all() and cond.max() <= A.COND_CAP, float(cond.max())
    want = np.ascontiguousarray(np.linalg.inv(a).transpose(0, 2, 1)).reshape(len(cs), -1)
    got, info = oracle.inverse_batched(flat.astype(np.float64).reshape(-1), n, oracle.ALGO_GJ_PIVOT)
    assert not np.asarray(info).any()
    got = np.asarray(got).reshape(len(cs), -1)
    tol = np.maximum(1e-10, 1e-15 * cond * n)  # tests/test_gpu_parity.py
    for k in range(len(cs)):
        assert rel_err(got[k], want[k], n) < tol[k], A.case_text(cs[k])


@pytest.mark.parametrize("dtype,n", SOLVE_LISTS, ids=lambda v: str(v))
def test_solve_lists(dtype, n):
    """the lists of the fused solve are built for the tile sweep it runs; where the inverse route runs the same sweep they are the same"""
    g, cs, flat = check_list(dtype, n, True)
    assert g.family == "tile" and g.transposed
    if A.geo(dtype, n).family == "tile":
        assert cs == A.cases(dtype, n) and g.blocks.tolist() == A.geo(dtype, n).blocks.tolist()
    keep = A.thin(dtype, n, AW.SOLVE_THIN)
    kept = [cs[k] for k in keep]
    assert len(set(keep.tolist())) == len(keep) <= AW.SOLVE_THIN
    assert {c.variant for c in kept} == set(A.VARIANTS) and {c.kind for c in kept} == {"A", "B", "BT"}
    assert {c.where for c in kept} == {"lu", "aop"}


def test_multipliers_lists_what_the_sweep_forms():
    """the per-matrix form of the model: (block step, kind, row, column, value) of one type A and one type B member, both sweeps"""
    for dtype, n in (("f64", 17), ("f32", 48)):
        g, cs = A.geo(dtype, n), A.cases(dtype, n)
        W, _, _ = A.matrices(dtype, n)
        for kind in ("A", "B"):
            k = next(j for j, c in enumerate(cs) if c.kind == kind and c.where == "aop" and not A.REJECTED[c.variant])
            items = A.multipliers(W[k:k + 1].copy(), g)[0]
            where, val = A.intended(cs[k], g)
            assert where + (val,) in items, (dtype, n, A.case_text(cs[k]))
            assert max(abs(v) for it in items for v in it[4:] if it[:4] != where) <= 0.5
            assert all(g.step[it[3]] == it[0] and it[2] != it[3] for it in items)


def covers(g, cs, what):
    """the coverage claims of tests/_accept_cases.py on a (sub)list"""
    n = g.n
    tiles = sorted(set(int(t) for t in g.tile[:n]))
    both = lambda sel: {True, False} <= {A.REJECTED[c.variant] for c in sel}  # noqa: E731  (an accepted and a rejected variant)
    if g.w == 4:
        nb = len(g.blocks)
        for b in sorted({0, nb // 2, nb - 1}):
            K = g.blocks[b]
            for i, k in A.LU_SLOTS:
                if K[i] < n and K[k] < n:
                    assert both([c for c in cs if c.where == "lu" and c.i == K[k] and c.other == K[i]]), (what, "LU slot", b, i, k)
    for T in tiles[1:]:
        assert both([c for c in cs if c.kind == "A" and c.where == "aop" and g.tile[c.other] == T and g.tile[c.i] < T]), (what, "A", T)
    for T in tiles[:-1]:
        assert both([c for c in cs if c.kind == "B" and g.tile[c.other] == T and g.tile[c.i] > T]), (what, "B", T)
    assert both([c for c in cs if c.kind == "A" and c.other == n - 1]), (what, "row n - 1")
    # the pivot's own tile, another block: what the exemption of the pivot rows must not swallow
    assert both([c for c in cs if c.kind == "B" and g.tile[c.other] == g.tile[c.i]]), (what, "B, own tile")
    if g.w == 4:
        assert both([c for c in cs if c.kind == "A" and c.where == "aop" and g.tile[c.other] == g.tile[c.i]]), (what, "A, own tile")
    assert {c.variant for c in cs} == set(A.VARIANTS), what


@pytest.mark.parametrize("dtype,n", LISTS, ids=lambda v: str(v))
def test_lists_cover_what_they_claim(dtype, n):
    g, cs = A.geo(dtype, n), A.cases(dtype, n)
    covers(g, cs, (dtype, n))
    aop = [c for c in cs if c.where == "aop"]
    # all 16 lanes of a lane group and all four lane groups: the tile-local row of the offending entry, the pivot number of its column
    assert {int(g.local[c.other]) for c in aop} == set(range(16)), sorted({int(g.local[c.other]) for c in aop})
    assert {int(g.pivno[c.i]) for c in aop} == set(range(g.w))
    assert any(c.kind == "BT" for c in cs) and any(c.kind == "B" and not c.sym for c in cs) and any(c.kind == "B" and c.sym for c in cs)
    if len(cs) < A.list_cap(g) - 8:  # not thinned: every column of the first tile column and every real column of the last one is a pivot
        tiles = sorted(set(int(t) for t in g.tile[:n]))
        pivots = {c.i for c in cs}
        assert {p for p in range(n) if g.tile[p] in (tiles[0], tiles[-1])} <= pivots | {int(g.blocks[0][0])} | {int(g.blocks[-1][0])}
    if (dtype, n) == ("f64", 64):  # the symmetric members reach the lower-tile arm, the others the full arm: each side complete
        covers(g, [c for c in cs if c.sym], "symmetric")
        covers(g, [c for c in cs if not c.sym and c.kind != "BT"], "one-sided")


def test_the_orderings_are_the_kernels():
    """the relabelled sweeps: fp64 blocks are four consecutive tile-local indices, fp32 blocks stride four; n = 32 and 64 on one wavefront
    interleave tile pairs by parity"""
    assert A.geo("f64", 48).blocks[:5].tolist() == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15], [16, 17, 18, 19]]
    assert A.geo("f32", 48).blocks[:5].tolist() == [[0, 4, 8, 12], [1, 5, 9, 13], [2, 6, 10, 14], [3, 7, 11, 15], [16, 20, 24, 28]]
    assert A.geo("f64", 64).blocks[:5].tolist() == [[0, 2, 4, 6], [8, 10, 12, 14], [16, 18, 20, 22], [24, 26, 28, 30], [1, 3, 5, 7]]
    assert A.geo("f32", 64).blocks[:5].tolist() == [[0, 8, 16, 24], [2, 10, 18, 26], [4, 12, 20, 28], [6, 14, 22, 30], [1, 9, 17, 25]]
    assert A.geo("f64", 80).blocks[:2].tolist() == [[0, 1, 2, 3], [4, 5, 6, 7]]            # the tile4 family loads plainly
    assert A.geo("f64", 17).blocks.reshape(-1).tolist() == list(range(17)) and not A.geo("f64", 17).transposed
    assert A.geo("f64", 17, True).blocks.tolist() == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15], [16, 17, 18, 19]]
    assert A.geo("f32", 17, True).blocks.tolist() == [[0, 4, 8, 12], [1, 5, 9, 13], [2, 6, 10, 14], [3, 7, 11, 15], [16, 20, 24, 28]]
    assert len(A.geo("f32", 18, True).blocks) == 6 and len(A.geo("f64", 26).blocks) == 7


def returns_of(text, struct, fn):
    """the expression a one-line member function of `struct` returns"""
    body = text[text.index(struct):]
    body = body[:body.index("};")]
    m = re.search(r"\b" + fn + r"\(([^)]*)\)\s*\{\s*return ([^;]*);", body)
    assert m, (struct, fn)
    return m.group(2)


def test_constants_and_orderings_in_the_sources():
    """what the model copies from csrc/: a change there fails here instead of quietly invalidating the model"""
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("tile_common.hpp", "rowlane2_kernels.hip", "tile_impl.hpp", "tile_screen.hpp",
                                                            "solve_tile_impl.hpp", "tile4_impl.hpp")}
    common = src["tile_common.hpp"]
    assert re.search(r"constexpr double TILE_TAU = 4\.0;", common) and A.TAU == 4.0
    assert re.search(r"constexpr double RL2_TAU = 4\.0;", src["rowlane2_kernels.hip"])
    for dt, struct in (("f64", "struct TileGeo<double>"), ("f32", "struct TileGeo<float>")):
        blk, piv, pcol, trow = (returns_of(common, struct, fn) for fn in ("blk", "piv", "pcol", "trow"))
        for c in range(16):
            assert eval(blk, {"c": c}) == A.BLK[dt](c) and eval(piv, {"c": c}) == A.PIV[dt](c)
        for rK in range(4):
            for t in range(4):
                assert eval(pcol, {"rK": rK, "t": t}) == A.PCOL[dt](rK, t)
                assert eval(trow, {"r": rK, "q": t}) == A.PCOL[dt](rK, t)  # the rows of a block carry the indices of its columns
    # the test itself: not-less-or-equal on the magnitude against the inline constant 4.0, in all four forms, and in the gated stage
    for t in ("f64", "f32"):
        assert common.count(f"v_cmp_nle_{t}_e64 vcc, |%1|, 4.0") == 2
    assert 'v_cmp_nle_f64_e64 vcc, |%[" #v "]|, 4.0' in common
    assert "if (!SPD) note_fail_except(bad, v, __ballot(panel_lane));" in common and "const bool panel_lane = G::blk(c) == rK;" in common
    assert common.count("note_fail(bad, l") == 6
    assert "rej = rej || !(rl2_abs(nm_lo) <= (T)RL2_TAU) || !(rl2_abs(nm_hi) <= (T)RL2_TAU);" in src["rowlane2_kernels.hip"]
    # orientation: the tile kernels sweep W = A^T (a lane group reads along a column of A), gj_rowlane2 sweeps A (a lane owns a row)
    for f in ("tile_impl.hpp", "tile_screen.hpp", "solve_tile_impl.hpp", "tile4_impl.hpp"):
        assert "const unsigned lane_off = (unsigned)(G::trow(0, l >> 4) * n + (l & 15));" in src[f], f
    assert "const T *Alo = A + i" in src["rowlane2_kernels.hip"] and "vl = Alo[cc * n], vh = Ahi[cc * n];" in src["rowlane2_kernels.hip"]
    # the relabelling of the one-wavefront kernels with FULL n and an even tile count; the tile4 family has none
    assert "constexpr bool PAIRED = FULL && (NT % 2 == 0);" in src["tile_impl.hpp"]
    assert "constexpr bool PAIRED = ONEWAVE && FULL && (NT % 2 == 0);" in src["tile_screen.hpp"]
    assert "constexpr bool PAIRED = FULL && (NT % 2 == 0) && !SPD;" in src["solve_tile_impl.hpp"]
    assert "PAIRED" not in src["tile4_impl.hpp"]
    for f in ("tile_impl.hpp", "tile_screen.hpp", "solve_tile_impl.hpp"):
        assert "(32 * (ti >> 1) + 2 * G::trow(r, 0) + (ti & 1)) * N" in src[f], f
    # blocks of identity padding alone are not run
    for f in ("tile_impl.hpp", "tile4_impl.hpp", "solve_tile_impl.hpp"):
        assert "if (!FULL && kb > 4 * (NT - 1) && kb - 4 * (NT - 1) >= G::real_blocks(n - 16 * (NT - 1))) continue;" in src[f], f
    assert returns_of(common, "struct TileGeo<double>", "real_blocks") == "(rem + 3) >> 2"
    assert returns_of(common, "struct TileGeo<float>", "real_blocks") == "rem < 4 ? rem : 4"
