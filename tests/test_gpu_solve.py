"""Batched linear solve X = A^-1 B (matinv_solve_batched) on the GPU against np.linalg.solve in float64.

Paths: the fused bordered MFMA tile kernel (16 < n <= 64, nrhs <= 16) with its pivoting row-solve fallback, the row solve of the
PIVOT policy, and the composed path (inverse + batched product) everywhere else. Tolerances as in test_gpu_parity.py:
  fp64 : max |x-y| / max(|y|, 1e-3*max|Y|) < max(1e-10, 1e-15 * cond * n)
  fp32 : ||X-Y||_F / ||Y||_F < 1e-5 * cond          (per matrix)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, as_mats, general_batch, pkg, spd_batch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
api = pkg("api")
GJ, CH = api.ALGO_GAUSS_JORDAN, api.ALGO_CHOLESKY
WORKER = os.path.join(ROOT, "tests", "_solve_worker.py")


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def rhs(n, nrhs, batch, seed, dtype=np.float64):
    return np.random.default_rng(seed).standard_normal(batch * n * nrhs).astype(dtype)


def as_rhs(flat, n, nrhs):
    """flat column-major batch of n x nrhs blocks -> (batch, n, nrhs)"""
    return np.asarray(flat, dtype=np.float64).reshape(-1, nrhs, n).transpose(0, 2, 1)


def gpu_solve(a, b, n, nrhs, algo=GJ, kernel=api.KERNEL_AUTO):
    ta, tb = dev(a), dev(b)
    batch = a.size // (n * n)
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    x = api.solve_batched(ta, tb, n, nrhs, algo, info=info, kernel=kernel)
    torch.cuda.synchronize()
    assert np.array_equal(ta.cpu().numpy(), a, equal_nan=True), "A was modified"
    assert np.array_equal(tb.cpu().numpy(), b, equal_nan=True), "B was modified"
    return x.cpu().numpy(), info.cpu().numpy()


def check_close(x, a, b, n, nrhs, f64, idx=None):
    mats = as_mats(a, n).astype(np.float64)
    bs, got = as_rhs(b, n, nrhs), as_rhs(x, n, nrhs)
    if idx is not None:
        mats, bs, got = mats[idx], bs[idx], got[idx]
    want = np.linalg.solve(mats, bs)
    for k in range(len(want)):
        cond = np.linalg.cond(mats[k])
        if f64:
            floor = 1e-3 * np.abs(want[k]).max()
            err = (np.abs(got[k] - want[k]) / np.maximum(np.abs(want[k]), floor)).max()
            assert err < max(1e-10, 1e-15 * cond * n), (k, err, cond)
        else:
            err = np.linalg.norm(got[k] - want[k]) / np.linalg.norm(want[k])
            assert err < 1e-5 * cond, (k, err, cond)


SIZES = [1, 2, 5, 8, 16, 17, 24, 32, 33, 48, 63, 64, 65, 100, 128, 200]


@pytest.mark.parametrize("n", SIZES)
def test_spd_solve_matches_numpy(n):
    for f64 in (True, False):
        dt = np.float64 if f64 else np.float32
        batch = 5 if n > 64 else 9
        a = spd_batch(n, batch, seed=n, dtype=dt)
        for nrhs in (1, 3, 16, 17):
            b = rhs(n, nrhs, batch, seed=n * nrhs, dtype=dt)
            for algo in (GJ, CH):
                x, info = gpu_solve(a, b, n, nrhs, algo)
                assert not info.any(), (n, nrhs, algo, f64)
                check_close(x, a, b, n, nrhs, f64)


@pytest.mark.parametrize("n", [5, 17, 32, 48, 64, 100])
def test_general_inputs_gauss_jordan(n):
    """U(0,1) matrices: most are rejected by the natural order (row solve / pivoting inverse), and the PIVOT policy."""
    a = general_batch(n, 24, seed=100 + n)
    for nrhs in (1, 7):
        b = rhs(n, nrhs, 24, seed=n + nrhs)
        for policy in (api.GJ_NATURAL_FIRST, api.GJ_PIVOT):
            old = api.set_gj_policy(policy)
            try:
                x, info = gpu_solve(a, b, n, nrhs, GJ)
            finally:
                api.set_gj_policy(old)
            assert not info.any()
            check_close(x, a, b, n, nrhs, True)
    a32 = a.astype(np.float32)
    b32 = rhs(n, 2, 24, seed=7, dtype=np.float32)
    x, info = gpu_solve(a32, b32, n, 2, GJ)
    assert not info.any()
    check_close(x, a32, b32, n, 2, False)


@pytest.mark.parametrize("n", [17, 32, 64, 128])
def test_singular_and_not_spd_report_info(n):
    """the cases of test_gpu_parity.test_singular_and_not_spd_report_info: info equals the inverse's, X NaN exactly there"""
    nrhs = 3
    a = spd_batch(n, 8, seed=3).reshape(8, n, n)
    a[2, 1, :] = 0.0  # column 1 of matrix 2 (memory is [k, col, row])
    a[5] = 0.0
    c = spd_batch(n, 8, seed=4).reshape(8, n, n)
    c[1, n - 1, n - 1] = -1.0
    c[3, 1, :] = 0.0
    c[6] = 0.0
    b = rhs(n, nrhs, 8, seed=5)
    for algo, m, bad in ((GJ, a, [2, 5]), (CH, c, [1, 3, 6])):
        flat = m.reshape(-1)
        x, info = gpu_solve(flat, b, n, nrhs, algo)
        iinfo = torch.full((8,), -7, dtype=torch.int32, device="cuda")
        api.inverse_batched(dev(flat), n, algo, info=iinfo)
        torch.cuda.synchronize()
        assert info.tolist() == iinfo.cpu().tolist(), (algo, info, iinfo)
        assert all(info[k] != 0 for k in bad)
        ok = [k for k in range(8) if k not in bad]
        assert not info[ok].any()
        xs = as_rhs(x, n, nrhs)
        assert np.isnan(xs[bad]).all()
        assert not np.isnan(xs[ok]).any()
        check_close(x, flat, b, n, nrhs, True, idx=ok)
    assert info[1] == n  # the negative last diagonal fails at the last pivot


@pytest.mark.parametrize("n", [8, 32, 50, 64, 100])
def test_cholesky_reads_lower_triangle_only(n):
    a = spd_batch(n, 6, seed=21)
    b = rhs(n, 4, 6, seed=22)
    clean, info = gpu_solve(a, b, n, 4, CH)
    assert not info.any()
    dirty = as_mats(a, n).copy()
    iu = np.triu_indices(n, 1)
    dirty[:, iu[0], iu[1]] = np.nan
    dirty = np.ascontiguousarray(dirty.transpose(0, 2, 1)).reshape(-1)
    got, info = gpu_solve(dirty, b, n, 4, CH)
    assert not info.any()
    assert np.array_equal(got, clean)


@pytest.mark.parametrize("n,nrhs,kernel", [(32, 5, api.KERNEL_AUTO), (64, 16, api.KERNEL_AUTO), (40, 2, api.KERNEL_AUTO),
                                           (12, 3, api.KERNEL_AUTO), (100, 2, api.KERNEL_AUTO), (64, 20, api.KERNEL_AUTO),
                                           (48, 4, api.KERNEL_LDS)])
def test_in_place_and_padded_strides(n, nrhs, kernel):
    batch = 7
    sa, sb = n * n + 13, n * nrhs + 5
    base = spd_batch(n, batch, seed=31)
    bb = rhs(n, nrhs, batch, seed=32)
    A = np.full(batch * sa, np.nan)
    B = np.full(batch * sb, np.nan)
    for k in range(batch):
        A[k * sa:k * sa + n * n] = base[k * n * n:(k + 1) * n * n]
        B[k * sb:k * sb + n * nrhs] = bb[k * n * nrhs:(k + 1) * n * nrhs]
    for algo in (GJ, CH):
        ta, tb = dev(A), dev(B)
        # out of place first: A and B bitwise unmodified, the padding of X untouched
        tx = torch.full_like(tb, 123.0)
        api.solve_batched(ta, tb, n, nrhs, algo, out=tx, kernel=kernel, batch=batch, strideA=sa, strideB=sb)
        torch.cuda.synchronize()
        assert np.array_equal(ta.cpu().numpy(), A, equal_nan=True) and np.array_equal(tb.cpu().numpy(), B, equal_nan=True)
        x = tx.cpu().numpy()
        for k in range(batch):
            assert (x[k * sb + n * nrhs:(k + 1) * sb] == 123.0).all()
        packed = np.concatenate([x[k * sb:k * sb + n * nrhs] for k in range(batch)])
        check_close(packed, base, bb, n, nrhs, True)
        # in place: out is B
        api.solve_batched(ta, tb, n, nrhs, algo, out=tb, kernel=kernel, batch=batch, strideA=sa, strideB=sb)
        torch.cuda.synchronize()
        y = tb.cpu().numpy()
        assert np.array_equal(np.concatenate([y[k * sb:k * sb + n * nrhs] for k in range(batch)]), packed)


@pytest.mark.parametrize("n", [20, 48, 64])
def test_per_matrix_determinism(n):
    """X_k depends on matrix k alone: a batch of dominant and general matrices, solved whole and as subsets, gives the same bits"""
    nrhs = 3
    dom = spd_batch(n, 12, seed=41).reshape(12, n * n)
    gen = general_batch(n, 12, seed=42).reshape(12, n * n)
    a = np.empty((24, n * n))
    a[0::2], a[1::2] = dom, gen
    b = rhs(n, nrhs, 24, seed=43).reshape(24, n * nrhs)
    for dt in (np.float64, np.float32):
        aa, bb = a.astype(dt), b.astype(dt)
        whole, info = gpu_solve(aa.reshape(-1), bb.reshape(-1), n, nrhs, GJ)
        assert not info.any()
        whole = whole.reshape(24, -1)
        for sel in (slice(0, None, 2), slice(1, None, 2), [3, 4, 17]):
            part, _ = gpu_solve(aa[sel].reshape(-1), bb[sel].reshape(-1), n, nrhs, GJ)
            assert np.array_equal(part.reshape(-1, n * nrhs), whole[sel])
        tile, _ = gpu_solve(aa.reshape(-1), bb.reshape(-1), n, nrhs, GJ, kernel=api.KERNEL_TILE)
        assert np.array_equal(tile.reshape(24, -1)[0::2], whole[0::2])
        check_close(whole.reshape(-1), aa.reshape(-1), bb.reshape(-1), n, nrhs, dt == np.float64)


@pytest.mark.parametrize("n", [32, 64])
def test_fused_agrees_with_composed(n):
    for dt, f64 in ((np.float64, True), (np.float32, False)):
        a = spd_batch(n, 16, seed=51, dtype=dt)
        for nrhs in (1, 16):
            b = rhs(n, nrhs, 16, seed=52, dtype=dt)
            for algo in (GJ, CH):
                assert api.solve_kernel_name(algo, dt, n, nrhs).startswith("matinv_solve_tile_")
                fused, i1 = gpu_solve(a, b, n, nrhs, algo, kernel=api.KERNEL_TILE)
                composed, i2 = gpu_solve(a, b, n, nrhs, algo, kernel=api.KERNEL_LDS)
                assert not i1.any() and not i2.any()
                check_close(fused, a, b, n, nrhs, f64)
                check_close(composed, a, b, n, nrhs, f64)
                y = as_rhs(composed, n, nrhs)
                tol = 1e-12 if f64 else 1e-5
                assert np.abs(as_rhs(fused, n, nrhs) - y).max() <= tol * np.abs(y).max()


def test_composed_path_chunking(tmp_path):
    """MATINV_BLOCKED_WS_MB=1 cuts the composed path into many k-range chunks: X is the same, bit for bit"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _solve_worker as w
    out = tmp_path / "chunk.npz"
    env = dict(os.environ, MATINV_BLOCKED_WS_MB="1")
    p = subprocess.run([sys.executable, WORKER, "chunk", str(out)], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "solve-worker ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    got = np.load(out)
    for name, n, nrhs, algo, kernel, batch in w.chunk_cases():
        a, b = w.chunk_inputs(n, nrhs, batch)
        x, info = gpu_solve(a, b, n, nrhs, algo, kernel)
        assert not info.any()
        assert np.array_equal(got[name], x), name
        check_close(x[: 5 * n * nrhs], a[: 5 * n * n], b[: 5 * n * nrhs], n, nrhs, True)


def test_reject_accounting():
    """MATINV_DEBUG_REJECTS=1: an SPD batch never leaves the fused kernel; general matrices reach the row solve and are counted"""
    env = dict(os.environ, MATINV_DEBUG_REJECTS="1")
    p = subprocess.run([sys.executable, WORKER, "rejects"], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "solve-worker ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])


def test_offsets_beyond_2_pow_32_elements():
    """1.1 M x 64^2 fp32 = 4.5e9 elements: matrix offsets past 2^32, spot-checked against numpy"""
    n, batch = 64, 1_100_000
    free, _ = torch.cuda.mem_get_info()
    need = batch * n * n * 4 + 3 * batch * n * 4
    assert free > need + (4 << 30), f"needs {need >> 30} GiB of device memory"
    g = torch.Generator(device="cuda").manual_seed(5)
    a = torch.rand(batch * n * n, dtype=torch.float32, device="cuda", generator=g)
    a.view(batch, n * n)[:, :: n + 1] += float(n)  # dominant diagonal
    b = torch.rand(batch * n, dtype=torch.float32, device="cuda", generator=g)
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    x = api.solve_batched(a, b, n, 1, GJ, info=info)
    torch.cuda.synchronize()
    assert int(info.abs().sum()) == 0
    first_high = (1 << 32) // (n * n)
    for k in (0, 12345, first_high - 1, first_high, first_high + 1, batch - 1):
        ak = a[k * n * n:(k + 1) * n * n].cpu().numpy().astype(np.float64)
        bk = b[k * n:(k + 1) * n].cpu().numpy().astype(np.float64)
        want = np.linalg.solve(as_mats(ak, n)[0], bk)
        got = x[k * n:(k + 1) * n].cpu().numpy()
        assert np.linalg.norm(got - want) / np.linalg.norm(want) < 1e-5 * np.linalg.cond(as_mats(ak, n)[0]), k
    del a, b, x


def test_solve_batched_host_matches_device():
    n, nrhs = 40, 3
    a = spd_batch(n, 11, seed=61)
    b = rhs(n, nrhs, 11, seed=62)
    x, info = api.solve_batched_host(a, b, n, nrhs, GJ)
    assert not info.any()
    check_close(x, a, b, n, nrhs, True)
    xd, _ = gpu_solve(a, b, n, nrhs, GJ)
    assert np.array_equal(x, xd)
