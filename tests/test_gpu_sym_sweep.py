"""The 64 x 64 fp64 Gauss-Jordan tile kernel classifies every matrix after its loads (csrc/tile_impl.hpp: tile_asymmetry) and
inverts a bitwise-symmetric one on its ten lower tiles (sym_tile_sweep, sym_tile_finish); every other matrix takes the full sweep.
What that could break, and what this file therefore pins at n = 64, the only size the arm serves:

* the arm itself: symmetric SPD and symmetric INDEFINITE batches (no positivity test) against numpy.linalg.inv, nothing handed to
  the pivoting kernel, and an exactly symmetric result;
* the classifier: one matrix per off-diagonal position (i, j) with 0.5 added to that element only. Treated as symmetric, from
  either triangle, such a matrix comes out with a relative error of 7.5e-3 (computed on the CPU), seven orders above the bound, so
  a classifier that misses one position -- tile pair, triangle, register or lane group -- cannot pass;
* the compare is on bits: +0.0 against -0.0 and a one-ulp difference count as asymmetric, a NaN equals itself;
* the routing of rejects out of the arm, with and without the screening pass, to the same bits;
* determinism: the bits of a matrix depend on the matrix alone, not on its place in the batch or on its neighbours' arm.

The expected value is numpy.linalg.inv, the bound the parity tests' rel_err < max(1e-10, 1e-15 cond n). Inputs were checked on the
CPU: R + R^T + n I has cond <= 2.3, R + R^T + 2 n diag(+-1) cond <= 1.8, and unpivoted elimination of either keeps every scalar
multiplier below 0.05, far from tau = 4."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import as_mats, general_batch, pkg, rel_err, spd_batch

pytestmark = pytest.mark.gpu

N = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one child process inverts several batches: argv = (input, inverse, info) triples; MATINV_DEBUG_REJECTS=1 is read at load time
WORKER = r"""
import sys, importlib, numpy as np, torch
sys.path.insert(0, %r)
api = importlib.import_module("cuda-matrix-inversion_amd.api")
args = sys.argv[1:]
for k in range(0, len(args), 3):
    a = np.load(args[k])
    n, batch = 64, a.size // 4096
    assert api.debug_rejects(reset=True) == 0
    d = torch.from_numpy(a).cuda()
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    x = api.inverse_batched(d, n, api.ALGO_GAUSS_JORDAN, info=info, batch=batch)
    torch.cuda.synchronize()
    print("KERNEL", api.kernel_name(api.ALGO_GAUSS_JORDAN, api.F64, n))
    print("REJECTS", api.debug_rejects(reset=True))
    np.save(args[k + 1], x.cpu().numpy())
    np.save(args[k + 2], info.cpu().numpy())
print("WORKER-OK")
""" % ROOT


def run_worker(tmp_path, tag, batches, env_extra):
    """[(inverse, info, rejects)] of the flat batches, inverted in one fresh process"""
    argv, outs = [], []
    for k, a in enumerate(batches):
        src, inv, info = (str(tmp_path / f"{tag}{k}_{w}.npy") for w in ("a", "inv", "info"))
        np.save(src, a)
        argv += [src, inv, info]
        outs.append((inv, info))
    r = subprocess.run([sys.executable, "-c", WORKER] + argv, env=dict(os.environ, **env_extra), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "WORKER-OK" in r.stdout, r.stdout + r.stderr
    kernels = [ln.split(" ", 1)[1] for ln in r.stdout.splitlines() if ln.startswith("KERNEL")]
    rejects = [int(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith("REJECTS")]
    assert len(kernels) == len(rejects) == len(batches)
    assert all(k.startswith("matinv_gj_tile_f64<4, true, true") for k in kernels), kernels
    return [(np.load(inv), np.load(info), rej) for (inv, info), rej in zip(outs, rejects)]


def invert(a):
    """in this process: (inverse, info, the input buffer as it is afterwards)"""
    import torch
    api = pkg("api")
    batch = a.size // (N * N)
    d = torch.from_numpy(a).cuda()
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    x = api.inverse_batched(d, N, api.ALGO_GAUSS_JORDAN, info=info, batch=batch)
    torch.cuda.synchronize()
    return x.cpu().numpy(), info.cpu().numpy(), d.cpu().numpy()


def flat(mats):
    """(batch, n, n) indexed [k, row, col] -> flat column-major batch"""
    return np.ascontiguousarray(np.asarray(mats).transpose(0, 2, 1)).reshape(-1)


def bounds(mats):
    """per matrix: (numpy.linalg.inv as a flat column-major row, the bound)"""
    want = np.linalg.inv(mats)
    cond = np.linalg.cond(mats)
    assert np.isfinite(cond).all() and cond.max() < 1e9
    return flat(want).reshape(-1, N * N), np.maximum(1e-10, 1e-15 * cond * N)


def check_each(got, mats, what):
    want, tol = bounds(mats)
    got = got.reshape(-1, N * N)
    worst = 0.0
    for k in range(len(mats)):
        e = rel_err(got[k], want[k], N)
        worst = max(worst, e / tol[k])
        assert e < tol[k], (what, k, e, tol[k])
    print(f"{what}: {len(mats)} matrices, worst error / bound {worst:.3g}")


def indefinite_batch(batch, seed):
    """R + R^T + 2 n diag(+-1): symmetric, about half of the eigenvalues negative"""
    rng = np.random.default_rng(seed)
    r = rng.random((batch, N, N))
    s = np.where(rng.random((batch, N)) < 0.5, -1.0, 1.0)
    m = r + r.transpose(0, 2, 1)
    m[:, np.arange(N), np.arange(N)] += 2 * N * s
    return m


@pytest.fixture(scope="module")
def two_symmetric_batches(tmp_path_factory):
    spd = as_mats(spd_batch(N, 300, seed=2025), N).copy()
    ind = indefinite_batch(300, seed=2026)
    runs = run_worker(tmp_path_factory.mktemp("sym"), "sym", [flat(spd), flat(ind)], {"MATINV_DEBUG_REJECTS": "1"})
    return {"spd": (spd, runs[0]), "indefinite": (ind, runs[1])}


@pytest.mark.parametrize("family", ["spd", "indefinite"])
def test_symmetric_batch_is_inverted_by_the_arm(two_symmetric_batches, family):
    mats, (got, info, rejects) = two_symmetric_batches[family]
    assert np.array_equal(mats, mats.transpose(0, 2, 1))
    if family == "indefinite":
        neg = (np.linalg.eigvalsh(mats) < 0).sum(axis=1)
        assert neg.min() >= 16 and neg.max() <= 48, (neg.min(), neg.max())
    check_each(got, mats, family)
    assert rejects == 0, rejects
    assert not info.any(), info[info != 0]
    x = got.reshape(-1, N, N)
    assert np.array_equal(x, x.transpose(0, 2, 1)), "the inverse of a symmetric matrix is not exactly symmetric"


def test_one_sided_perturbation_at_every_position():
    base = as_mats(spd_batch(N, 1, seed=77), N)[0]
    pos = [(i, j) for i in range(N) for j in range(N) if i != j]
    assert len(pos) == N * N - N
    mats = np.repeat(base[None], len(pos), axis=0)
    for k, (i, j) in enumerate(pos):
        mats[k, i, j] += 0.5
    a = flat(mats)
    before = a.copy()
    got, info, after = invert(a)
    assert np.array_equal(after.view(np.uint64), before.view(np.uint64)), "the input buffer was written to"
    assert not info.any()
    check_each(got, mats, "one-sided")


def test_bit_level_cases():
    mats = as_mats(spd_batch(N, 6, seed=404), N).copy()
    # 0: a mirror pair +0.0 / -0.0; 1: a pair one ulp apart -- asymmetric by their bits, only the bound applies
    mats[0, 37, 5], mats[0, 5, 37] = 0.0, -0.0
    mats[1, 12, 50] = np.nextafter(mats[1, 50, 12], np.inf)
    assert mats[1, 12, 50] != mats[1, 50, 12]
    # 2: NaN on the diagonal; 3: a mirrored NaN pair off it -- symmetric by their bits, rejected by the acceptance test
    mats[2, 9, 9] = np.nan
    mats[3, 20, 41] = mats[3, 41, 20] = np.nan
    # 4, 5: untouched
    got, info, _ = invert(flat(mats))
    got = got.reshape(-1, N * N)
    fine = [0, 1, 4, 5]
    check_each(got[fine], mats[fine], "bit-level")
    assert not info[fine].any()
    for k in (2, 3):
        assert info[k] != 0, (k, info)
        assert np.isnan(got[k]).all(), k


def built(base, i, delta, j=N - 1):
    """test_gpu_gated_panel.py: pivot i is delta exactly when it is reached, and row j's multiplier there is 1 / delta"""
    m = base.copy()
    m[i, :] = 0.0
    m[:, i] = 0.0
    m[i, i] = delta
    m[i, j] = m[j, i] = 1.0
    return m


def test_rejects_leave_the_arm_with_and_without_screening(tmp_path):
    # The kernel's labels: index m sits in tile row 2 (m >> 5) + (m & 1), tile-local row (m & 31) >> 1. Pivot 0 = first block step,
    # 6 = last pivot of that block, 40 = block step 9 (tile row 2), 9 = block step 5 (tile row 1), 61 = the last block step; the
    # coupled row 63 is in tile row 3, the last row of the last block: another tile row than the pivot but for 61.
    batch = 120
    mats = as_mats(spd_batch(N, batch, seed=555), N).copy()
    plan = [(2, 0, 1e-3), (3, 0, 0.0), (30, 6, 1e-3), (31, 6, 0.0), (50, 40, 1e-3), (51, 40, 0.0), (70, 9, 1e-3), (71, 9, 0.0),
            (118, 61, 1e-3), (119, 61, 0.0)]
    for k, i, delta in plan:
        mats[k] = built(mats[k], i, delta)
    assert np.array_equal(mats, mats.transpose(0, 2, 1))
    a = flat(mats)
    runs = {}
    for screen in ("0", "1"):
        (got, info, rejects), = run_worker(tmp_path, "rej" + screen, [a], {"MATINV_DEBUG_REJECTS": "1", "MATINV_TILE_SCREEN": screen})
        print(f"screen={screen}: rejects {rejects} (expected {len(plan)})")
        assert rejects == len(plan), (screen, rejects)
        assert not info.any()
        check_each(got, mats, "rejects, screen=" + screen)
        runs[screen] = (got, info)
    assert np.array_equal(runs["0"][0], runs["1"][0]) and np.array_equal(runs["0"][1], runs["1"][1])


def test_bits_depend_on_the_matrix_alone():
    sym = as_mats(spd_batch(N, 256, seed=808), N).copy()
    sym[128:] = indefinite_batch(128, seed=809)
    gen = as_mats(general_batch(N, 256, seed=810), N) + N * np.eye(N)  # R + n I: accepted, not symmetric, the full sweep
    ref_sym = invert(flat(sym))[0].reshape(-1, N * N)
    ref_gen = invert(flat(gen))[0].reshape(-1, N * N)
    check_each(ref_gen, gen, "general, dominant")
    # again
    assert np.array_equal(invert(flat(sym))[0].reshape(-1, N * N), ref_sym)
    # shuffled
    perm = np.random.default_rng(811).permutation(len(sym))
    assert np.array_equal(invert(flat(sym[perm]))[0].reshape(-1, N * N), ref_sym[perm])
    # interleaved with matrices that take the other arm
    mixed = np.empty((512, N, N))
    mixed[0::2], mixed[1::2] = sym, gen
    got = invert(flat(mixed))[0].reshape(-1, N * N)
    assert np.array_equal(got[0::2], ref_sym)
    assert np.array_equal(got[1::2], ref_gen)
