"""CPU half of the pivot-search coverage (tests/test_gpu_pivot_search.py, tests/_pivot_worker.py): the lists of tests/_pivot_cases.py
see what they are for. A numpy model of Gauss-Jordan with partial pivoting, in the working dtype, runs every case of every size two
ways: clean (its error must stay below 1/8 of the parity bound) and with ONE step taking the second-best candidate, for every step
k < n - 1 in turn (its error must reach 8 times the bound). The reference is numpy.linalg.inv in float64 on the float64 image of the
matrix as stored, the measure the elementwise one of tests/test_gpu_parity.py in both dtypes, the bounds max(1e-10, 1e-15 cond n)
and 1e-5 cond at the matrix's own condition number. Also: the model's pivot order is pi (pi^-1 for the transpose), numpy's sign of the
determinant is parity(pi) prod sign(D), the candidates of every step are far apart, the coverage counts hold, delta is the best of its
ladder, the sizes follow the route functions, and the CPU oracle inverts every case.

reseed_table() (python tests/test_pivot_cases_cpu.py) prints the entries _pivot_cases.RESEED needs when a case misses a condition."""
import numpy as np
import pytest

import _pivot_cases as P
import oracle
from conftest import rel_err

LISTS = [(dt, n) for dt in ("f64", "f32") for n in P.ALL_SIZES[dt]]


def model(dtype, n, delta=None, seeds=None):
    """(clean error / bound [B], sabotaged error / bound [B, n-1] (NaN or inf count as inf), pivot order, second / best, cond)"""
    cs = P.cases(n)
    if delta is None and seeds is None:
        mats = P.matrices(dtype, n)[0]
    else:
        mats = np.stack([P.build(dtype, n, c.index, c.orient, delta=delta, seed=None if seeds is None else seeds[k])[0] for k, c in enumerate(cs)])
    want, cond = P.reference(mats)
    with np.errstate(all="ignore"):
        clean, order, second, bad = P.clean_and_sabotaged(np.array(mats), want)
    b = P.bound(dtype, cond, n)
    bad = np.where(np.isfinite(bad), bad, np.inf)
    return clean / b, bad / b[:, None], order, second, cond


def test_sizes_follow_the_route():
    a = P.api()
    for dt in ("f64", "f32"):
        assert P.sizes(dt) == P.SIZES[dt]
        route = P.auto_route(dt)
        names = [route[n] for n in P.SIZES[dt]]
        for part in ("gj_rowlane<", "gj_rowlane2<", "gj_tile_", "gj_tile4_", "gj_tilep_", "gj_tilep3_", "gj_tilep4_", "gj_tileqw_"):
            assert any(part in a or part in p for a, p in names), (dt, part)
        # TILEP with 2, 3 and 4 tiles, ragged and full; TILEP4 up to 128; TILEQ from 129 to the last n
        assert {26, 32, 33, 48, 49, 64, 65, 128, 129, max(route)} <= set(P.SIZES[dt])
        assert max(route) == (192 if dt == "f64" else 256)
        for fam in P.FORCED:
            assert P.forced_sizes(dt, fam) == P.FORCED_SIZES[fam]
        code = a.F64 if dt == "f64" else a.F32
        t = min(n for n in range(2, 1025) if "update_mfma" in a.kernel_name(a.ALGO_GAUSS_JORDAN, code, n, a.KERNEL_BLOCKED))
        assert {t - 1, t} <= set(P.FORCED_SIZES["blocked"])
        assert set(P.ALL_SIZES[dt]) == set(P.SIZES[dt]) | {n for fam in P.FORCED for n in P.forced_sizes(dt, fam)}
    import _pivot_worker as W
    for dt in ("f64", "f32"):
        assert sorted(n for g in W.GROUPS[dt].values() for n in g) == list(P.ALL_SIZES[dt])


@pytest.mark.parametrize("n", sorted({n for _, n in LISTS} | {300, 512, 513}))
def test_coverage(n):
    ps = P.perms(n)
    labels = [p.label for p in ps]
    assert labels[0] == "identity" and labels[1] == "reversal"
    if n > 16:  # below, some of the generated permutations coincide (n = 2 has two in all) and are listed once
        assert {"shift1", "shift16", f"shift{n - 16}", "rot4", "trow", "random0", "random1", "random2"} <= set(labels)
        assert any(lb.startswith("swap") for lb in labels)
    assert len({p.pi.tobytes() for p in ps}) == len(ps)
    miss = P.coverage(n, [p.pi for p in ps])
    assert not (miss["residue"] or miss["tile"] or miss["inside"] or miss["outside"] or miss["parity"]), miss
    # what n does not have is named: residues >= n, and a pivot outside its block of four when there is one block
    assert miss["absent"]["residue"] == [r for r in range(16) if r >= n]
    assert miss["absent"]["outside"] == (list(range(n)) if n <= 4 else [])
    # the counts: 16 x 16 residue pairs (those n has), NT x NT tile pairs
    k = np.arange(n)
    pairs = {(int(a), int(b)) for p in ps for a, b in zip(k % 16, p.pi % 16)}
    tiles = {(int(a), int(b)) for p in ps for a, b in zip(k // 16, p.pi // 16)}
    nt = -(-n // 16)
    assert len(pairs) == min(n, 16) ** 2 and len(tiles) == nt * nt
    assert len(ps) <= 64, "the batch is on the order of 40 permutations x 2 orientations"
    # the same without the identity, which the AUTO run leaves out (n = 2 has one other permutation)
    if n > 2:
        rest = P.coverage(n, [p.pi for p in ps[1:]])
        assert not (rest["residue"] or rest["tile"] or rest["inside"] or rest["outside"] or rest["parity"]), rest


@pytest.mark.parametrize("dtype,n", LISTS)
def test_clean_and_sabotaged(dtype, n):
    """every case, every step: none left out"""
    clean, bad, order, second, cond = model(dtype, n)
    mats, flat, want_order, sign, ident = P.matrices(dtype, n)
    assert len(clean) == len(P.cases(n)) and bad.shape == (len(clean), n - 1)
    print(f"{dtype} n={n}: {len(clean)} cases, largest clean / bound {clean.max():.3g}, smallest sabotaged / bound "
          f"{bad.min():.3g}, median {np.median(bad):.3g}, cond <= {cond.max():.3g}")
    assert cond.max() < 5
    assert np.array_equal(order, want_order), "the model's pivot order is not pi"
    assert (clean <= 1 / P.FLOOR).all(), [P.case_text(n, P.cases(n)[k]) for k in np.flatnonzero(clean > 1 / P.FLOOR)]
    low = np.argwhere(bad < P.FLOOR)
    assert not len(low), [(P.case_text(n, P.cases(n)[k]), int(s), float(bad[k, s])) for k, s in low[:8]]
    # every step but the last has a runner-up, a factor of about delta below the pivot: far beyond the 2^-20 relative resolution of the
    # fp64 compare of the top 32 bits
    assert (second[:, :n - 1] > 0).all() and second.max() < 4 * P.DELTA[dtype] < 2.0 ** -8
    a64 = np.asarray(mats, dtype=np.float64)
    assert np.array_equal(np.linalg.slogdet(a64)[0], sign)
    assert ident.sum() == 2 and all(np.array_equal(P.perms(n)[c.index].pi, np.arange(n)) for c in P.cases(n) if c.identity)
    assert len({m.tobytes() for m in flat}) == len(flat) - (1 if n == 1 else 0)


@pytest.mark.parametrize("dtype,n", LISTS)
def test_the_oracle_inverts_every_case(dtype, n):
    mats, flat, _, _, _ = P.matrices(dtype, n)
    want, cond = P.reference(mats)
    got, info = oracle.inverse_batched(flat.astype(np.float64).reshape(-1), n, oracle.ALGO_GJ_PIVOT)
    assert not info.any()
    got = got.reshape(len(mats), n, n).transpose(0, 2, 1)
    assert (P.elementwise(got, want) < 1e-12).all()
    assert rel_err(np.ascontiguousarray(want.transpose(0, 2, 1)), np.ascontiguousarray(got.transpose(0, 2, 1)), n) < 1e-12


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_delta_is_the_best_of_its_ladder(dtype):
    """the chosen delta has the largest worst-case ratio of sabotaged error to bound on its ladder, over every case and step of the sizes LADDER_SIZES (those up to 49, and 100)"""
    worst = {}
    for delta in P.LADDER[dtype]:
        rs = [model(dtype, n, delta=delta) for n in P.LADDER_SIZES[dtype]]
        worst[delta] = (max(r[0].max() for r in rs), min(r[1].min() for r in rs))
        print(f"{dtype} delta 2^{int(np.log2(delta))}: largest clean / bound {worst[delta][0]:.3g}, smallest sabotaged / bound {worst[delta][1]:.3g}")
    assert P.DELTA[dtype] == max(worst, key=lambda d: worst[d][1])
    assert worst[P.DELTA[dtype]][0] <= 1 / P.FLOOR and worst[P.DELTA[dtype]][1] >= P.FLOOR


def reseed_table():
    """the RESEED entries the lists need: for every case that misses a condition at seed 0, the first seed that meets both"""
    table = {}
    for dtype, n in LISTS:
        cs = P.cases(n)
        seeds = [P.RESEED.get((dtype, n, c.index, c.orient), 0) for c in cs]
        for _ in range(20):
            clean, bad, _, _, _ = model(dtype, n, seeds=seeds)
            miss = np.flatnonzero((clean > 1 / P.FLOOR) | (bad.min(axis=1, initial=np.inf) < P.FLOOR))
            if not len(miss):
                break
            for k in miss:
                seeds[k] += 1
        table.update({(dtype, n, c.index, c.orient): s for c, s in zip(cs, seeds) if s})
        print(dtype, n, "ok" if not len(miss) else f"{len(miss)} cases still miss", flush=True)
    print("RESEED =", table)


if __name__ == "__main__":
    reseed_table()
