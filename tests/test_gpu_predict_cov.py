"""The joint predictive covariance between a GP's query points (matinv_predict_cov_batched) on the GPU against float64 numpy on the float64
image of exactly what the kernel reads. Reference, inputs, bounds and their derivation: tests/_predict_cov_worker.py (first order, not
fitted; err / bound is printed; tests/test_predict_cov_cpu.py holds a float32 numpy evaluation against the same bounds).

The generated instantiation sweep (tests/_instantiations.py) has no route for the covariance forms, so this file runs the tile forms at
both ends of every instantiation's size range itself, and the global form either side of its lower end and at n = 1024. Q = 33 makes three
groups of queries: diagonal blocks, an adjacent and a non-adjacent block below the diagonal, and two restagings of the query buffer."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _predict_cov_worker as W
import _predict_worker as P
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


def gpu_cov(n, B, c, d, As, Es, want=("mean", "cov")):
    """(mean, cov, info) as numpy (None for what was not asked for); checks that the inputs are bitwise unchanged and cov symmetric"""
    tb, tc, td, ta, te = dev(B), dev(c), dev(d), dev(As), dev(Es)
    batch = B.size // (n * n)
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    mean, cov = api.predict_cov_batched(n, tb, tc, td, ta, te, info=info, want=want)
    torch.cuda.synchronize()
    for t, x in ((tb, B), (tc, c), (td, d), (ta, As), (te, Es)):
        assert x is None or np.array_equal(t.cpu().numpy(), x, equal_nan=True), "an input was modified"
    mean, cov = (None if o is None else o.cpu().numpy() for o in (mean, cov))
    if cov is not None:
        W.assert_symmetric(cov, As.size // (batch * n))
    return mean, cov, info.cpu().numpy()


def accuracy(n, dt, with_c):
    name = api.predict_cov_kernel_name(dt, n)
    assert name.startswith("matinv_spd_tile_f" if n <= 96 else "matinv_chol_global<") and name.endswith(", true, true, true, true>")
    B, c, d, mdl, As, Es = W.case(n, np.dtype(dt).name, with_c)
    for nquery in W.QS:
        a, e = W.leading(As, Es, n, nquery)
        mean, cov, info = gpu_cov(n, B, c, d, a, e)
        assert not info.any(), (n, dt, info)
        W.check(mean, cov, W.cov_reference(mdl, a, e, n, nquery), n, U[np.dtype(dt)], what=f"{name} c={'yes' if with_c else 'no'}")


@pytest.mark.parametrize("n", W.TILE_SIZES + W.GLOBAL_SIZES)
def test_accuracy(n):
    for dt in DTYPES:
        for with_c in (True, False):
            accuracy(n, dt, with_c)


@pytest.mark.parametrize("with_c", [True, False])
@pytest.mark.parametrize("dt", DTYPES)
def test_accuracy_1024(dt, with_c):
    accuracy(1024, dt, with_c)


@pytest.mark.parametrize("n", [16, 64, 96, 130])
def test_agrees_with_predict_batched(n):
    """with the prior variances of predict_batched on the diagonal of E: mean bit-equal (the same operations), diag(cov) within twice the
    var bound of _predict_worker, since each side is within one"""
    nquery = 17
    for dt in DTYPES:
        u = U[np.dtype(dt)]
        B, c, d, mdl, As, Es = W.case(n, np.dtype(dt).name, True)
        batch = W.batch_of(n)
        a, e = W.leading(As, Es, n, nquery)
        ediag = np.ascontiguousarray(np.diagonal(e.reshape(batch, nquery, nquery), axis1=1, axis2=2)).reshape(-1)
        mean, cov, info = gpu_cov(n, B, c, d, a, e)
        assert not info.any()
        pm, pv = api.predict_batched(n, dev(B), dev(c), dev(d), dev(a), dev(ediag))
        torch.cuda.synchronize()
        pm, pv = pm.cpu().numpy(), pv.cpu().numpy()
        assert np.array_equal(mean, pm), (n, dt)
        ref = P.predict_reference(mdl, a, ediag, n, nquery)
        P.check(pm, pv, ref, n, u, what=f"predict_batched {np.dtype(dt).name}")
        _, b_var = P.bounds(ref, n, u)
        diag = np.diagonal(W.unpack(cov, nquery), axis1=1, axis2=2).astype(np.float64)
        r = np.abs(diag - pv.reshape(batch, nquery).astype(np.float64)) / b_var
        print(f"  {np.dtype(dt).name} n={n} |diag(cov) - var| / bound: {r.max():.3f}")
        assert (r <= 2).all()


def raw_cov(n, nquery, tb, tc, td, ta, te, mean, cov, batch, info=None):
    """the C entry point itself: mean or cov may be None (NULL)"""
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    code = api.F64 if tb.dtype == torch.float64 else api.F32
    lib.check(lib.lib().matinv_predict_cov_batched(code, n, nquery, p(tb), p(tc), p(td), p(ta), p(te), p(mean), p(cov), batch, p(info),
                                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


@pytest.mark.parametrize("n", [33, 64, 96, 130])
def test_optional_outputs_and_reads(n):
    """only mean and only cov give the bits of the joint call; Es = None equals Es = 0; the strict upper triangles of E and of B are not
    read; nothing is written beyond batchSize * Q^2, batchSize * Q or info[batchSize]; given tensors are returned"""
    nquery = 17
    qq = nquery * nquery
    for dt in DTYPES:
        B, c, d, mdl, As, Es = W.case(n, np.dtype(dt).name, True)
        batch = W.batch_of(n)
        a, e = W.leading(As, Es, n, nquery)
        mean, cov, info = gpu_cov(n, B, c, d, a, e)
        assert not info.any()
        m1, c1, _ = gpu_cov(n, B, c, d, a, e, want=("mean",))
        assert c1 is None and np.array_equal(m1, mean)
        m2, c2, _ = gpu_cov(n, B, c, d, a, None, want=("mean",))
        assert c2 is None and np.array_equal(m2, mean)
        m3, c3, _ = gpu_cov(n, B, c, None, a, e, want=("cov",))
        assert m3 is None and np.array_equal(c3, cov)
        m4, c4, _ = gpu_cov(n, B, c, d, a, None)
        m5, c5, _ = gpu_cov(n, B, c, d, a, np.zeros_like(e))
        assert np.array_equal(m4, mean) and np.array_equal(m5, mean) and np.array_equal(c4, c5)
        # cov without E is minus the covariance reduction
        ref0 = W.cov_reference(mdl, a, None, n, nquery)
        W.check(None, c4, ref0, n, U[np.dtype(dt)], what="Es = None")
        assert (np.diagonal(W.unpack(c4, nquery), axis1=1, axis2=2) < 0).all()
        # NaN in the strict upper triangle of E (element (i, j), i < j, at j * Q + i) and of B (element (r, col), r < col, at col * n + r)
        e_nan = e.reshape(batch, nquery, nquery).copy()
        e_nan[:, np.triu(np.ones((nquery, nquery), dtype=bool), 1).T] = np.nan  # [k, j, i] with i < j
        b_nan = B.reshape(batch, n, n).copy()
        b_nan[:, np.triu(np.ones((n, n), dtype=bool), 1).T] = np.nan
        m6, c6, i6 = gpu_cov(n, b_nan.reshape(-1), c, d, a, e_nan.reshape(-1))
        assert not i6.any() and np.array_equal(m6, mean) and np.array_equal(c6, cov)
        # the C entry point with tensors larger than the call: batchSize matrices only, the tails untouched
        part = batch - 2
        tb, tc, td, ta, te = dev(B), dev(c), dev(d), dev(a), dev(e)
        for with_mean, with_cov in ((True, True), (True, False), (False, True)):
            om = torch.full((batch * nquery,), 5.0, dtype=tb.dtype, device="cuda") if with_mean else None
            oc = torch.full((batch * qq,), 5.0, dtype=tb.dtype, device="cuda") if with_cov else None
            oi = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
            raw_cov(n, nquery, tb, tc, td if with_mean else None, ta, te if with_cov else None, om, oc, part, oi)
            torch.cuda.synchronize()
            for o, full, per in ((om, mean, nquery), (oc, cov, qq)):
                if o is not None:
                    assert np.array_equal(o[:part * per].cpu().numpy(), full[:part * per]) and (o[part * per:] == 5.0).all()
            assert not oi[:part].any() and (oi[part:] == -7).all()
        # given tensors are used and returned
        om = torch.empty(batch * nquery, dtype=tb.dtype, device="cuda")
        rm, rc = api.predict_cov_batched(n, tb, tc, td, ta, te, mean=om, want=())
        torch.cuda.synchronize()
        assert rm is om and rc is None and np.array_equal(om.cpu().numpy(), mean)
        oc = torch.empty(batch * qq, dtype=tb.dtype, device="cuda")
        rm, rc = api.predict_cov_batched(n, tb, tc, None, ta, te, cov=oc, want=())
        torch.cuda.synchronize()
        assert rm is None and rc is oc and np.array_equal(oc.cpu().numpy(), cov)


@pytest.mark.parametrize("n", [33, 64, 95, 130])
def test_locality(n):
    """from a Q = 33 call: a Q = 4 call on queries (0, 15, 16, 32) with E's submatrix reproduces that 4 x 4 submatrix bit for bit (other
    groups, other lanes, the same order of every pair); a Q = 17 call on queries 16 .. 32 reproduces the trailing 17 x 17 block; Q = 1
    calls reproduce the diagonal elements; a matrix alone reproduces its own results"""
    for dt in DTYPES:
        B, c, d, mdl, As, Es = W.case(n, np.dtype(dt).name, True)
        batch = W.batch_of(n)
        mean, cov, info = gpu_cov(n, B, c, d, As, Es)
        assert not info.any() and np.isfinite(mean).all() and np.isfinite(cov).all()
        mean, cov = mean.reshape(batch, W.QMAX), W.unpack(cov, W.QMAX)
        sel = [0, 15, 16, 32]
        a, e = W.pick(As, Es, n, sel)
        m4, c4, _ = gpu_cov(n, B, c, d, a, e)
        assert np.array_equal(m4.reshape(batch, 4), mean[:, sel]), (n, dt)
        assert np.array_equal(W.unpack(c4, 4), cov[:, sel][:, :, sel]), (n, dt)
        a, e = W.pick(As, Es, n, slice(16, 33))
        m17, c17, _ = gpu_cov(n, B, c, d, a, e)
        assert np.array_equal(m17.reshape(batch, 17), mean[:, 16:]) and np.array_equal(W.unpack(c17, 17), cov[:, 16:, 16:]), (n, dt)
        for j in sel:
            a, e = W.pick(As, Es, n, [j])
            m1, c1, _ = gpu_cov(n, B, c, d, a, e)
            assert np.array_equal(m1, mean[:, j]) and np.array_equal(c1, cov[:, j, j]), (n, dt, j)
        k = batch - 2
        mk, ck, _ = gpu_cov(n, B.reshape(batch, -1)[k], c.reshape(batch, -1)[k], d.reshape(batch, -1)[k], As.reshape(batch, -1)[k],
                            Es.reshape(batch, -1)[k])
        assert np.array_equal(mk, mean[k]) and np.array_equal(W.unpack(ck, W.QMAX)[0], cov[k])


@pytest.mark.parametrize("n", [17, 64, 100])
def test_not_spd_reports_info(n):
    nquery = 17
    for dt in DTYPES:
        B0, _, d, mdl, As, Es = W.case(n, np.dtype(dt).name, False)
        B = B0.copy()
        a, e = W.leading(As, Es, n, nquery)
        want = W.break_three(B, None, n, (1, 3, 4))
        assert want == {1: n, 3: 2, 4: 1}
        mean, cov, info = gpu_cov(n, B, None, d, a, e)
        W.check_with_rejects(mean, cov, info, B, None, d, a, e, n, nquery, dt, want, what=f"not SPD {np.dtype(dt).name}")


@pytest.mark.parametrize("n", [40, 100])
def test_host_form_equals_device_form(n):
    nquery = 17
    for dt in DTYPES:
        B, c, d, mdl, As, Es = W.case(n, np.dtype(dt).name, True)
        a, e = W.leading(As, Es, n, nquery)
        mean, cov, info = api.predict_cov_batched_host(n, B, c, d, a, e)
        assert not info.any()
        W.check(mean, cov, W.cov_reference(mdl, a, e, n, nquery), n, U[np.dtype(dt)], what="host")
        dm, dc, _ = gpu_cov(n, B, c, d, a, e)
        assert np.array_equal(mean, dm) and np.array_equal(cov, dc)
        m, v, info = api.predict_cov_batched_host(n, B, c, None, a, None, want=("cov",))
        assert m is None and not info.any() and np.array_equal(v, gpu_cov(n, B, c, d, a, None)[1])


def test_grid_stride_and_chunking():
    """one process with the grid held to one round of resident workgroups and the workspace cap at 1 MiB: tests/_predict_cov_worker.py"""
    e = dict(os.environ)
    e.update({"MATINV_TILE_GRID_MULT": "1", "MATINV_BLOCKED_WS_MB": "1"})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_predict_cov_worker.py")], capture_output=True, text=True, env=e,
                       timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "predict-cov-worker ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
