"""Batched GP prediction at many query points per covariance matrix (matinv_predict_batched) on the GPU against float64 numpy on the
float64 image of exactly what the kernel reads. Reference, inputs, bounds and their derivation: tests/_predict_worker.py (first order,
not fitted; err / bound is printed; tests/test_predict_cpu.py holds a float32 numpy evaluation against the same bounds).

The generated instantiation sweep (tests/_instantiations.py) has no route for the prediction forms, so this file runs the tile forms at
both ends of every instantiation's size range itself, and the global form either side of its lower end and at n = 1024."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _predict_worker as W
from conftest import pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
api = pkg("api")
lib = pkg("_lib")
U = W.U
DTYPES = (np.float64, np.float32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(x):
    return None if x is None else torch.tensor(np.ascontiguousarray(x)).cuda()  # a copy: the shared cases are read-only arrays


def gpu_predict(n, B, c, d, As, Es, want=("mean", "var")):
    """(mean, var, info) as numpy (None for what was not asked for); checks that the inputs are bitwise unchanged"""
    tb, tc, td, ta, te = dev(B), dev(c), dev(d), dev(As), dev(Es)
    batch = B.size // (n * n)
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    mean, var = api.predict_batched(n, tb, tc, td, ta, te, info=info, want=want)
    torch.cuda.synchronize()
    for t, x in ((tb, B), (tc, c), (td, d), (ta, As), (te, Es)):
        assert x is None or np.array_equal(t.cpu().numpy(), x, equal_nan=True), "an input was modified"
    return (None if mean is None else mean.cpu().numpy()), (None if var is None else var.cpu().numpy()), info.cpu().numpy()


def accuracy(n, dt, with_c):
    name = api.predict_kernel_name(dt, n)
    assert name.startswith("matinv_spd_tile_f" if n <= 96 else "matinv_chol_global<") and name.endswith(", true, true, true>")
    B, c, d, mdl, As, Es = W.case(n, np.dtype(dt).name, with_c)
    for nquery in W.QS:
        a, e = W.first_queries(As, Es, n, nquery)
        mean, var, info = gpu_predict(n, B, c, d, a, e)
        assert not info.any(), (n, dt, info)
        W.check(mean, var, W.predict_reference(mdl, a, e, n, nquery), n, U[np.dtype(dt)], what=f"{name} c={'yes' if with_c else 'no'}")


@pytest.mark.parametrize("n", W.TILE_SIZES + W.GLOBAL_SIZES)
def test_accuracy(n):
    for dt in DTYPES:
        for with_c in (True, False):
            accuracy(n, dt, with_c)


@pytest.mark.parametrize("with_c", [True, False])
@pytest.mark.parametrize("dt", DTYPES)
def test_accuracy_1024(dt, with_c):
    accuracy(1024, dt, with_c)


def raw_predict(n, nquery, tb, tc, td, ta, te, mean, var, batch, info=None):
    """the C entry point itself: mean or var may be None (NULL)"""
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    code = api.F64 if tb.dtype == torch.float64 else api.F32
    lib.check(lib.lib().matinv_predict_batched(code, n, nquery, p(tb), p(tc), p(td), p(ta), p(te), p(mean), p(var), batch, p(info),
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


@pytest.mark.parametrize("n", [33, 64, 96, 130])
def test_optional_outputs(n):
    """only mean (also with Ds given and Es = None) and only var give the bits of the joint call; Es = None equals Es = 0; nothing is
    written beyond batchSize * Q or where nothing was asked"""
    nquery = 17
    for dt in DTYPES:
        B, c, d, mdl, As, Es = W.case(n, np.dtype(dt).name, True)
        batch = W.batch_of(n)
        a, e = W.first_queries(As, Es, n, nquery)
        mean, var, info = gpu_predict(n, B, c, d, a, e)
        assert not info.any()
        m1, v1, _ = gpu_predict(n, B, c, d, a, e, want=("mean",))
        assert v1 is None and np.array_equal(m1, mean)
        m2, v2, _ = gpu_predict(n, B, c, d, a, None, want=("mean",))
        assert v2 is None and np.array_equal(m2, mean)
        m3, v3, _ = gpu_predict(n, B, c, None, a, e, want=("var",))
        assert m3 is None and np.array_equal(v3, var)
        m4, v4, _ = gpu_predict(n, B, c, d, a, None)
        m5, v5, _ = gpu_predict(n, B, c, d, a, np.zeros_like(e))
        assert np.array_equal(m4, mean) and np.array_equal(m5, mean) and np.array_equal(v4, v5)
        # var without e is minus the variance reduction
        ref0 = W.predict_reference(mdl, a, None, n, nquery)
        assert (ref0["var"] < 0).all() and (v4 < 0).all()
        W.check(None, v4, ref0, n, U[np.dtype(dt)], what="Es = None")
        # the C entry point with tensors larger than the call: batchSize matrices only, the tails untouched
        part = batch - 2
        tb, tc, td, ta, te = dev(B), dev(c), dev(d), dev(a), dev(e)
        for with_mean, with_var in ((True, True), (True, False), (False, True)):
            om = torch.full((batch * nquery,), 5.0, dtype=tb.dtype, device="cuda") if with_mean else None
            ov = torch.full((batch * nquery,), 5.0, dtype=tb.dtype, device="cuda") if with_var else None
            oi = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
            raw_predict(n, nquery, tb, tc, td if with_mean else None, ta, te, om, ov, part, oi)
            torch.cuda.synchronize()
            for o, full in ((om, mean), (ov, var)):
                if o is not None:
                    assert np.array_equal(o[:part * nquery].cpu().numpy(), full[:part * nquery]) and (o[part * nquery:] == 5.0).all()
            assert not oi[:part].any() and (oi[part:] == -7).all()
        # given tensors are used and returned
        om = torch.empty(batch * nquery, dtype=tb.dtype, device="cuda")
        rm, rv = api.predict_batched(n, tb, tc, td, ta, te, mean=om, want=())
        torch.cuda.synchronize()
        assert rm is om and rv is None and np.array_equal(om.cpu().numpy(), mean)


@pytest.mark.parametrize("n", [33, 64, 95, 130])
def test_independence_of_queries_and_matrices(n):
    """from a Q = 33 call, queries 0, 15, 16 and 32 of each matrix are bit-equal to Q = 1 calls on those vectors alone; a matrix is
    bit-equal to a call on it alone"""
    for dt in DTYPES:
        B, c, d, mdl, As, Es = W.case(n, np.dtype(dt).name, True)
        batch = W.batch_of(n)
        mean, var, info = gpu_predict(n, B, c, d, As, Es)
        assert not info.any() and np.isfinite(mean).all() and np.isfinite(var).all()
        mean, var = mean.reshape(batch, W.QMAX), var.reshape(batch, W.QMAX)
        a3, e2 = As.reshape(batch, W.QMAX, n), Es.reshape(batch, W.QMAX)
        for j in (0, 15, 16, 32):
            m1, v1, _ = gpu_predict(n, B, c, d, np.ascontiguousarray(a3[:, j]).reshape(-1), np.ascontiguousarray(e2[:, j]))
            assert np.array_equal(m1, mean[:, j]) and np.array_equal(v1, var[:, j]), (n, dt, j)
        # queries 16 .. 32 as a call of their own: another position in the group for each of them
        m17, v17, _ = gpu_predict(n, B, c, d, np.ascontiguousarray(a3[:, 16:]).reshape(-1), np.ascontiguousarray(e2[:, 16:]).reshape(-1))
        assert np.array_equal(m17.reshape(batch, -1), mean[:, 16:]) and np.array_equal(v17.reshape(batch, -1), var[:, 16:])
        k = batch - 2
        mk, vk, _ = gpu_predict(n, B.reshape(batch, -1)[k], c.reshape(batch, -1)[k], d.reshape(batch, -1)[k], a3[k].reshape(-1), e2[k])
        assert np.array_equal(mk, mean[k]) and np.array_equal(vk, var[k])


@pytest.mark.parametrize("n", [17, 64, 100])
def test_not_spd_reports_info(n):
    nquery = 17
    for dt in DTYPES:
        B0, _, d, mdl, As, Es = W.case(n, np.dtype(dt).name, False)
        B = B0.copy()
        a, e = W.first_queries(As, Es, n, nquery)
        want = W.break_three(B, None, n, (1, 3, 4))
        assert want == {1: n, 3: 2, 4: 1}
        mean, var, info = gpu_predict(n, B, None, d, a, e)
        W.check_with_rejects(mean, var, info, B, None, d, a, e, n, nquery, dt, want, what=f"not SPD {np.dtype(dt).name}")


@pytest.mark.parametrize("n", [16, 64, 96, 130])
def test_agrees_with_the_fused_mean_and_variance(n):
    """Q = 1 is what matinv_mean_batched / matinv_variance_batched compute, each with a sweep of its own: within twice the bounds, since
    each side is within one"""
    for dt in DTYPES:
        u = U[np.dtype(dt)]
        B, c, d, mdl, As, Es = W.case(n, np.dtype(dt).name, True)
        a, e = W.first_queries(As, Es, n, 1)
        mean, var, info = gpu_predict(n, B, c, d, a, e)
        assert not info.any()
        tb, tc, td, ta, te = dev(B), dev(c), dev(d), dev(a), dev(e)
        fm = api.calcluateMean(n, ta, tb, tc, td)
        fv = api.calcluateVariance(n, ta, tb, tc, te)
        torch.cuda.synchronize()
        ref = W.predict_reference(mdl, a, e, n, 1)
        W.check(fm.cpu().numpy(), fv.cpu().numpy(), ref, n, u, what=f"fused mean / variance {np.dtype(dt).name}")
        b_mean, b_var = W.bounds(ref, n, u)
        r_m = np.abs(mean.astype(np.float64) - fm.cpu().numpy().astype(np.float64)) / b_mean[:, 0]
        r_v = np.abs(var.astype(np.float64) - fv.cpu().numpy().astype(np.float64)) / b_var[:, 0]
        print(f"  {np.dtype(dt).name} n={n} |predict - fused| / bound: mean {r_m.max():.3f} var {r_v.max():.3f}")
        assert (r_m <= 2).all() and (r_v <= 2).all()


@pytest.mark.parametrize("n", [40, 100])
def test_host_form_equals_device_form(n):
    nquery = 17
    for dt in DTYPES:
        B, c, d, mdl, As, Es = W.case(n, np.dtype(dt).name, True)
        a, e = W.first_queries(As, Es, n, nquery)
        mean, var, info = api.predict_batched_host(n, B, c, d, a, e)
        assert not info.any()
        W.check(mean, var, W.predict_reference(mdl, a, e, n, nquery), n, U[np.dtype(dt)], what="host")
        dm, dv, _ = gpu_predict(n, B, c, d, a, e)
        assert np.array_equal(mean, dm) and np.array_equal(var, dv)
        m, v, info = api.predict_batched_host(n, B, c, None, a, None, want=("var",))
        assert m is None and not info.any() and np.array_equal(v, gpu_predict(n, B, c, d, a, None)[1])


def test_grid_stride_and_chunking():
    """one process with the grid held to one round of resident workgroups and the workspace cap at 1 MiB: tests/_predict_worker.py"""
    e = dict(os.environ)
    e.update({"MATINV_TILE_GRID_MULT": "1", "MATINV_BLOCKED_WS_MB": "1"})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_predict_worker.py")], capture_output=True, text=True, env=e,
                       timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "predict-worker ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
