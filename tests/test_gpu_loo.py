"""Batched leave-one-out cross-validation of a GP (matinv_loo_batched) on the GPU against float64 numpy on the float64 image of exactly
what the kernel reads. Reference, bounds and their derivation: tests/_loo_worker.py (first order, not tuned; err / bound is printed).

The generated instantiation sweep (tests/_instantiations.py) has no `loo` route, so this file runs the LOO forms of the tile kernels at
both ends of every instantiation's size range itself, and the global form either side of its lower end and at n = 1024."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _loo_worker as W
from conftest import as_mats, pkg, spd_batch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
api = pkg("api")
lib = pkg("_lib")
U = W.U
DTYPES = (np.float64, np.float32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def gpu_loo(n, B, c, d):
    """(mean, var, logpl, info) as numpy; checks that the inputs are bitwise unchanged"""
    tb, tc, td = dev(B), dev(c), dev(d)
    batch = B.size // (n * n)
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    mean, var, logpl = api.loo_batched(n, tb, tc, td, info=info)
    torch.cuda.synchronize()
    assert np.array_equal(tb.cpu().numpy(), B, equal_nan=True) and np.array_equal(td.cpu().numpy(), d), "an input was modified"
    assert c is None or np.array_equal(tc.cpu().numpy(), c), "c was modified"
    return mean.cpu().numpy(), var.cpu().numpy(), logpl.cpu().numpy(), info.cpu().numpy()


def raw_loo(n, tb, tc, td, mean, var, logpl, batch, info=None):
    """the C entry point itself: any of mean / var / logpl may be None (NULL)"""
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    code = api.F64 if tb.dtype == torch.float64 else api.F32
    lib.check(lib.lib().matinv_loo_batched(code, n, p(tb), p(tc), p(td), p(mean), p(var), p(logpl), batch, p(info),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


# every size the tile forms begin and end at, and the global form beyond 96
TILE_SIZES = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96]
GLOBAL_SIZES = [97, 130, 200]


@pytest.mark.parametrize("n", TILE_SIZES + GLOBAL_SIZES)
def test_accuracy(n):
    batch = 13 if n <= 64 else 5
    for dt in DTYPES:
        name = api.loo_kernel_name(dt, n)
        assert name.startswith("matinv_spd_tile_f" if n <= 96 else "matinv_chol_global<") and name.endswith(", true>")
        for with_c in (True, False):
            B, c, d = W.inputs(n, batch, dt, with_c)
            mean, var, logpl, info = gpu_loo(n, B, c, d)
            assert not info.any(), (n, dt, info)
            W.check(mean, var, logpl, W.reference(B, c, d, n), n, U[np.dtype(dt)], what=f"{name} c={'yes' if with_c else 'no'}")


def test_accuracy_1024():
    n = 1024
    B, c, d = W.inputs(n, 2, np.float64)
    mean, var, logpl, info = gpu_loo(n, B, c, d)
    assert not info.any()
    W.check(mean, var, logpl, W.reference(B, c, d, n), n, U[np.dtype(np.float64)], what=api.loo_kernel_name(np.float64, n))


@pytest.mark.parametrize("n", [5, 17])
def test_is_really_leave_one_out(n):
    """for every i: delete row and column i from M and predict point i from the other n - 1 -- the meaning, not just the formula"""
    batch = 6
    B, c, d = W.inputs(n, batch, np.float64)
    mean, var, _, info = gpu_loo(n, B, c, d)
    assert not info.any()
    ref = W.reference(B, c, d, n)
    M, dd = ref["M"], ref["d"]
    mu, s2 = np.empty((batch, n)), np.empty((batch, n))
    for k in range(batch):
        for i in range(n):
            rest = [j for j in range(n) if j != i]
            Mr, m = M[k][np.ix_(rest, rest)], M[k][rest, i]
            mu[k, i] = m @ np.linalg.solve(Mr, dd[k][rest])
            s2[k, i] = M[k][i, i] - m @ np.linalg.solve(Mr, m)
    # the closed form agrees with the deletion far inside the bounds, so the bounds may be taken around either
    assert np.abs(mu - ref["mu"]).max() < 1e-12 and np.abs(s2 - ref["s2"]).max() < 1e-12
    brute = dict(ref, mu=mu, s2=s2)
    W.check(mean, var, None, brute, n, U[np.dtype(np.float64)], what="deletion")


@pytest.mark.parametrize("n", [48, 100])
def test_agrees_with_the_inverse(n):
    """1 / var and (d - mean) / var against the diagonal and the mat-vec of the library's own inverse_batched(CHOLESKY) of the
    materialised M, within twice the bounds: kappa^ = 1 / s2^ has the relative bound eps of s2, and alpha^ = (d - mu^) / s2^ has
    |d alpha| <= |d mu| / s2 + |alpha| |d s2| / s2 <= kappa * b_mean + eps * |alpha|"""
    batch = 7
    for dt in DTYPES:
        u = U[np.dtype(dt)]
        B, c, d = W.inputs(n, batch, dt)
        mean, var, _, info = gpu_loo(n, B, c, d)
        assert not info.any()
        Mflat = B.copy()
        Mflat.reshape(batch, n * n)[:, ::n + 1] += c.reshape(batch, n)  # the same rounding as the kernel's add
        iinfo = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
        X = api.inverse_batched(dev(Mflat), n, api.ALGO_CHOLESKY, info=iinfo)
        torch.cuda.synchronize()
        assert not iinfo.cpu().numpy().any()
        K = as_mats(X.cpu().numpy(), n).astype(np.float64)
        ref = W.reference(B, c, d, n)
        b_mean, b_var, _ = W.bounds(ref, n, u)
        eps = b_var / ref["s2"]
        kap_inv = np.einsum("kii->ki", K)
        alpha_inv = np.einsum("kij,kj->ki", K, ref["d"])
        m64, v64 = mean.astype(np.float64).reshape(batch, n), var.astype(np.float64).reshape(batch, n)
        r_k = np.abs(1.0 / v64 - kap_inv) / (eps * ref["kappa"])
        r_a = np.abs((ref["d"] - m64) / v64 - alpha_inv) / (ref["kappa"] * b_mean + eps * np.abs(ref["alpha"]))
        print(f"  {np.dtype(dt).name} n={n} err/bound: kappa={r_k.max():.3f} alpha={r_a.max():.3f}")
        assert (r_k <= 2).all() and (r_a <= 2).all(), (dt, n, r_k.max(), r_a.max())


@pytest.mark.parametrize("n", [17, 64, 100])
def test_not_spd_reports_info(n):
    for dt in DTYPES:
        B, _, d = W.inputs(n, 8, dt, with_c=False)
        want = W.break_three(B, None, n, (1, 3, 6))
        assert want == {1: n, 3: 2, 6: 1}
        mean, var, logpl, info = gpu_loo(n, B, None, d)
        W.check_with_rejects(mean, var, logpl, info, B, None, d, n, dt, want, what=f"not SPD {np.dtype(dt).name}")


@pytest.mark.parametrize("n", [8, 50, 96, 100])
def test_reads_lower_triangle_only(n):
    for dt in DTYPES:
        B, c, d = W.inputs(n, 6, dt)
        dirty = as_mats(B, n).copy()
        iu = np.triu_indices(n, 1)
        dirty[:, iu[0], iu[1]] = np.nan
        dirty = np.ascontiguousarray(dirty.transpose(0, 2, 1)).reshape(-1)
        assert n == 1 or np.isnan(dirty).any()
        clean = gpu_loo(n, B, c, d)
        got = gpu_loo(n, dirty, c, d)
        assert not clean[3].any() and not got[3].any()
        for a, b in zip(clean[:3], got[:3]):
            assert np.isfinite(a).all() and np.array_equal(a, b)


@pytest.mark.parametrize("n", [33, 64, 100])
def test_purity_and_optional_outputs(n):
    batch, extra = 7, 3
    for dt in DTYPES:
        B, c, d = W.inputs(n, batch + extra, dt)
        tb, tc, td = dev(B), dev(c), dev(d)
        tt = tb.dtype
        mean = torch.full(((batch + extra) * n,), 123.0, dtype=tt, device="cuda")
        var = torch.full(((batch + extra) * n,), 321.0, dtype=tt, device="cuda")
        logpl = torch.full((batch + extra,), 77.0, dtype=tt, device="cuda")
        info = torch.full((batch + extra,), -7, dtype=torch.int32, device="cuda")
        m, v, lp = api.loo_batched(n, tb, tc, td, mean=mean, var=var, logpl=logpl, batchSize=batch, info=info)
        torch.cuda.synchronize()
        assert m is mean and v is var and lp is logpl
        assert np.array_equal(tb.cpu().numpy(), B) and np.array_equal(tc.cpu().numpy(), c) and np.array_equal(td.cpu().numpy(), d)
        assert (mean[batch * n:] == 123.0).all() and (var[batch * n:] == 321.0).all() and (logpl[batch:] == 77.0).all()
        assert (info[batch:] == -7).all() and not info[:batch].any()
        full = [t.cpu().numpy() for t in (mean[:batch * n], var[:batch * n], logpl[:batch])]
        W.check(*full, W.reference(B[:batch * n * n], c[:batch * n], d[:batch * n], n), n, U[np.dtype(dt)], what="batchSize")
        # every non-empty subset of the outputs: the same bits as the full call, and nothing written where nothing was asked
        for mask in range(1, 8):
            outs = [torch.full_like(t, 5.0) if mask >> j & 1 else None for j, t in enumerate((mean, var, logpl))]
            raw_loo(n, tb, tc, td, *outs, batch)
            torch.cuda.synchronize()
            for j, (o, size) in enumerate(zip(outs, (batch * n, batch * n, batch))):
                if o is not None:
                    assert np.array_equal(o[:size].cpu().numpy(), full[j]), (n, dt, mask, j)
                    assert (o[size:] == 5.0).all()
        # the allocating form returns the same bits as well
        m2, v2, lp2 = api.loo_batched(n, tb, tc, td, batchSize=batch)
        assert m2.numel() == batch * n and v2.numel() == batch * n and lp2.numel() == batch
        assert all(np.array_equal(t.cpu().numpy(), f) for t, f in zip((m2, v2, lp2), full))


@pytest.mark.parametrize("n", [20, 64, 100])
def test_per_matrix_determinism(n):
    """the result for matrix k depends on matrix k alone: the whole batch and three subsets give the same bits"""
    for dt in DTYPES:
        B, c, d = W.inputs(n, 12, dt)
        whole = gpu_loo(n, B, c, d)
        assert not whole[3].any()
        Bm, cm, dm = B.reshape(12, n * n), c.reshape(12, n), d.reshape(12, n)
        for sel in (slice(0, None, 2), slice(1, None, 2), [3, 4, 11]):
            part = gpu_loo(n, Bm[sel].reshape(-1), cm[sel].reshape(-1), dm[sel].reshape(-1))
            assert np.array_equal(part[0], whole[0].reshape(12, n)[sel].reshape(-1))
            assert np.array_equal(part[1], whole[1].reshape(12, n)[sel].reshape(-1))
            assert np.array_equal(part[2], whole[2][sel])


def test_host_form_equals_device_form():
    n = 40
    for dt in DTYPES:
        B, c, d = W.inputs(n, 11, dt)
        for cc in (c, None):
            mean, var, logpl, info = api.loo_batched_host(n, B, cc, d)
            assert not info.any()
            W.check(mean, var, logpl, W.reference(B, cc, d, n), n, U[np.dtype(dt)], what="host")
            dm, dv, dl, _ = gpu_loo(n, B, cc, d)
            assert np.array_equal(mean, dm) and np.array_equal(var, dv) and np.array_equal(logpl, dl)


def test_grid_stride_and_chunking():
    """one process with the grid held to one round of resident workgroups and the workspace cap at 1 MiB: tests/_loo_worker.py"""
    e = dict(os.environ)
    e.update({"MATINV_TILE_GRID_MULT": "1", "MATINV_BLOCKED_WS_MB": "1"})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_loo_worker.py")], capture_output=True, text=True, env=e, timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "loo-worker ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
