"""Gradients of the batched GP log marginal likelihood (matinv_logml_grad_batched) on the GPU against float64 numpy on the float64 image
of exactly what the kernel reads. Reference, bounds and their derivation: tests/_logml_grad_worker.py (first order, not tuned; err / bound
is printed; tests/test_logml_grad_cpu.py holds a float32 numpy evaluation against the same bounds).

The generated instantiation sweep (tests/_instantiations.py) has no route for the gradient forms, so this file runs the tile forms at
both ends of every instantiation's size range itself, and the global form either side of its lower end and at n = 1024."""
import ctypes
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import _logml_grad_worker as W
from conftest import as_mats, pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
api = pkg("api")
lib = pkg("_lib")
U = W.U
DTYPES = (np.float64, np.float32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ("grad", "gradc", "alpha")


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def gpu_grad(n, B, c, d, dMs):
    """(grad, gradc, alpha, info) as numpy; checks that the inputs are bitwise unchanged"""
    tb, tc, td, tm = dev(B), dev(c), dev(d), dev(dMs)
    batch = B.size // (n * n)
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    grad, gradc, alpha = api.logml_grad_batched(n, tb, tc, td, tm, info=info, want=ALL)
    torch.cuda.synchronize()
    assert np.array_equal(tb.cpu().numpy(), B, equal_nan=True) and np.array_equal(td.cpu().numpy(), d), "an input was modified"
    assert np.array_equal(tm.cpu().numpy(), dMs, equal_nan=True), "dMs was modified"
    assert c is None or np.array_equal(tc.cpu().numpy(), c), "c was modified"
    return grad.cpu().numpy(), gradc.cpu().numpy(), alpha.cpu().numpy(), info.cpu().numpy()


def raw_grad(n, nparam, tb, tc, td, tm, grad, gradc, alpha, batch, info=None):
    """the C entry point itself: any of grad / gradc / alpha may be None (NULL)"""
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    code = api.F64 if tb.dtype == torch.float64 else api.F32
    lib.check(lib.lib().matinv_logml_grad_batched(code, n, nparam, p(tb), p(tc), p(td), p(tm), p(grad), p(gradc), p(alpha), batch, p(info),
                                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


@pytest.mark.parametrize("n", W.TILE_SIZES + W.GLOBAL_SIZES)
def test_accuracy(n):
    batch = W.batch_of(n)
    for dt in DTYPES:
        name = api.logml_grad_kernel_name(dt, n)
        assert name.startswith("matinv_spd_tile_f" if n <= 96 else "matinv_chol_global<") and name.endswith(", true, true>")
        for nparam, with_c in itertools.product((1, 3), (True, False)):
            B, c, d = W.inputs(n, batch, dt, with_c)
            dMs = W.derivs(n, batch, nparam, dt)
            grad, gradc, alpha, info = gpu_grad(n, B, c, d, dMs)
            assert not info.any(), (n, dt, info)
            W.check(grad, gradc, alpha, W.reference(B, c, d, dMs, n, nparam), n, U[np.dtype(dt)],
                    what=f"{name} P={nparam} c={'yes' if with_c else 'no'}")


def test_accuracy_1024():
    n = 1024
    B, c, d = W.inputs(n, 2, np.float64)
    dMs = W.derivs(n, 2, 1, np.float64)
    grad, gradc, alpha, info = gpu_grad(n, B, c, d, dMs)
    assert not info.any()
    W.check(grad, gradc, alpha, W.reference(B, c, d, dMs, n, 1), n, U[np.dtype(np.float64)], what=api.logml_grad_kernel_name(np.float64, n))


def flat_sym(mats, dt):
    """(count, n, n) symmetric matrices -> flat column-major batch"""
    return np.ascontiguousarray(mats.transpose(0, 2, 1)).reshape(-1).astype(dt)


@pytest.mark.parametrize("n", [17, 100])
def test_identity_and_m_as_derivative(n):
    """the meaning, not just the formula: with dM = I the gradient is the sum of the gradients w.r.t. the diagonal terms, and with dM = M
    (a scaling of the whole covariance) it is 1/2 d^T alpha - n/2"""
    batch = 5
    for dt in DTYPES:
        u = U[np.dtype(dt)]
        B, c, d = W.inputs(n, batch, dt)
        M = W.image(B, c, n)  # exactly representable in dt: the diagonal was rounded in dt
        dM = np.stack([np.broadcast_to(np.eye(n), (batch, n, n)), M], axis=1).reshape(2 * batch, n, n)
        dMs = flat_sym(dM, dt)
        assert np.array_equal(W.sym_lower(dMs, n), dM)
        grad, gradc, alpha, info = gpu_grad(n, B, c, d, dMs)
        assert not info.any()
        ref = W.reference(B, c, d, dMs, n, 2)
        W.check(grad, gradc, alpha, ref, n, u, what=f"dM = I, M {np.dtype(dt).name}")
        b_grad, b_gradc, _ = W.bounds(ref, n, u)
        g = grad.astype(np.float64).reshape(batch, 2)
        sum_gradc = gradc.astype(np.float64).reshape(batch, n).sum(axis=1)
        r_i = np.abs(g[:, 0] - sum_gradc) / (b_grad[:, 0] + n * b_gradc)
        closed = 0.5 * np.einsum("ki,ki->k", ref["d"], ref["alpha"]) - 0.5 * n
        assert np.abs(closed - ref["grad"][:, 1]).max() < 1e-9 * n  # the identity itself, far inside the bounds
        r_m = np.abs(g[:, 1] - closed) / b_grad[:, 1]
        print(f"  {np.dtype(dt).name} n={n} err/bound: dM=I vs sum gradc {r_i.max():.3f}  dM=M vs d.alpha/2 - n/2 {r_m.max():.3f}")
        assert (r_i <= 1).all() and (r_m <= 1).all()


@pytest.mark.parametrize("n", [5, 17])
def test_unit_derivative_gives_gradc(n):
    """dM = e_i e_i^T is the derivative w.r.t. c_i: grad[k, i] == gradc[k, i]"""
    batch = 4
    for dt in DTYPES:
        u = U[np.dtype(dt)]
        B, c, d = W.inputs(n, batch, dt)
        units = np.zeros((n, n, n))
        units[np.arange(n), np.arange(n), np.arange(n)] = 1.0
        dMs = flat_sym(np.tile(units, (batch, 1, 1)), dt)
        grad, gradc, alpha, info = gpu_grad(n, B, c, d, dMs)
        assert not info.any()
        ref = W.reference(B, c, d, dMs, n, n)
        W.check(grad, gradc, alpha, ref, n, u, what=f"dM = e_i e_i^T {np.dtype(dt).name}")
        b_grad, b_gradc, _ = W.bounds(ref, n, u)
        r = np.abs(grad.astype(np.float64).reshape(batch, n) - gradc.astype(np.float64).reshape(batch, n)) / (b_grad + b_gradc[:, None])
        print(f"  {np.dtype(dt).name} n={n} err/bound: grad vs gradc {r.max():.3f}")
        assert (r <= 1).all()


def numpy_logml(M, dd):
    n = M.shape[-1]
    sol = np.linalg.solve(M, dd[..., None])[..., 0]
    return -0.5 * np.einsum("ki,ki->k", dd, sol) - 0.5 * np.linalg.slogdet(M)[1] - 0.5 * n * math.log(2 * math.pi)


@pytest.mark.parametrize("n", [5, 17])
def test_difference_quotient_of_the_library_logml(n):
    """(logml(B + h dM) - logml(B - h dM)) / 2h from the library's own logml_batched against grad. h is chosen where the same quotient,
    evaluated in numpy from the reference logml, is closest to the reference gradient (largest deviation over the batch); the GPU
    quotient may then differ from grad by four times that deviation (logml_batched's own rounding divided by 2h) plus the bound"""
    batch, nparam, dt = 6, 2, np.float64
    B, c, d = W.inputs(n, batch, dt)
    dMs = W.derivs(n, batch, nparam, dt)
    grad, _, _, info = gpu_grad(n, B, c, d, dMs)
    assert not info.any()
    ref = W.reference(B, c, d, dMs, n, nparam)
    b_grad, _, _ = W.bounds(ref, n, U[np.dtype(dt)])

    def numpy_quotient(h, p):
        return (numpy_logml(ref["M"] + h * ref["dM"][:, p], ref["d"]) - numpy_logml(ref["M"] - h * ref["dM"][:, p], ref["d"])) / (2 * h)

    dev_np = {h: max(np.abs(numpy_quotient(h, p) - ref["grad"][:, p]).max() for p in range(nparam)) for h in (1e-3, 1e-4, 1e-5, 1e-6)}
    h = min(dev_np, key=dev_np.get)
    tb_, tc, td = B.reshape(batch, n * n), dev(c), dev(d)
    dm = dMs.reshape(batch, nparam, n * n)
    g = grad.reshape(batch, nparam)
    for p in range(nparam):
        plus = api.logml_batched(n, dev(tb_ + h * dm[:, p]), tc, td)
        minus = api.logml_batched(n, dev(tb_ - h * dm[:, p]), tc, td)
        torch.cuda.synchronize()
        quot = (plus.cpu().numpy() - minus.cpu().numpy()) / (2 * h)
        diff = np.abs(quot - g[:, p])
        allowed = 4 * dev_np[h] + b_grad[:, p]
        print(f"  n={n} p={p} h={h:g}: numpy quotient off by {dev_np[h]:.3e}, GPU quotient - grad {diff.max():.3e}, allowed {allowed.min():.3e}")
        assert (diff <= allowed).all(), (n, p, h, diff.max(), allowed.min())


@pytest.mark.parametrize("n", [48, 100])
def test_agrees_with_the_inverse(n):
    """the route a caller had before: inverse_batched(CHOLESKY) of the materialised M, contracted in float64 numpy -- within twice the
    bounds (one for each of the two computed inverses)"""
    batch, nparam = 7, 2
    for dt in DTYPES:
        u = U[np.dtype(dt)]
        B, c, d = W.inputs(n, batch, dt)
        dMs = W.derivs(n, batch, nparam, dt)
        grad, gradc, alpha, info = gpu_grad(n, B, c, d, dMs)
        assert not info.any()
        Mflat = B.copy()
        Mflat.reshape(batch, n * n)[:, ::n + 1] += c.reshape(batch, n)  # the same rounding as the kernel's add
        iinfo = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
        X = api.inverse_batched(dev(Mflat), n, api.ALGO_CHOLESKY, info=iinfo)
        torch.cuda.synchronize()
        assert not iinfo.cpu().numpy().any()
        K = as_mats(X.cpu().numpy(), n).astype(np.float64)
        ref = W.reference(B, c, d, dMs, n, nparam)
        a_inv = np.einsum("kij,kj->ki", K, ref["d"])
        G = a_inv[:, :, None] * a_inv[:, None, :] - K
        via = dict(ref, alpha=a_inv, gradc=0.5 * (a_inv ** 2 - np.einsum("kii->ki", K)), grad=0.5 * np.einsum("kij,kpij->kp", G, ref["dM"]))
        rs = {k: v.max() for k, v in W.ratios(grad, gradc, alpha, via, n, u).items()}
        print(f"  {np.dtype(dt).name} n={n} err/bound against the inverse: " + " ".join(f"{k}={v:.3f}" for k, v in rs.items()))
        assert all(v <= 2 for v in rs.values()), (dt, n, rs)


@pytest.mark.parametrize("n", [17, 64, 100])
def test_not_spd_reports_info(n):
    nparam = 2
    for dt in DTYPES:
        B, _, d = W.inputs(n, 8, dt, with_c=False)
        dMs = W.derivs(n, 8, nparam, dt)
        want = W.break_three(B, None, n, (1, 3, 6))
        assert want == {1: n, 3: 2, 6: 1}
        grad, gradc, alpha, info = gpu_grad(n, B, None, d, dMs)
        W.check_with_rejects(grad, gradc, alpha, info, B, None, d, dMs, n, nparam, dt, want, what=f"not SPD {np.dtype(dt).name}")


def dirty_upper(flat, n):
    """the same batch with NaN in every strictly upper triangle"""
    m = as_mats(flat, n).copy()
    iu = np.triu_indices(n, 1)
    m[:, iu[0], iu[1]] = np.nan
    out = np.ascontiguousarray(m.transpose(0, 2, 1)).reshape(-1)
    assert n == 1 or np.isnan(out).any()
    return out


@pytest.mark.parametrize("n", [8, 50, 96, 100])
def test_reads_lower_triangle_only(n):
    for dt in DTYPES:
        B, c, d = W.inputs(n, 6, dt)
        dMs = W.derivs(n, 6, 2, dt)
        clean = gpu_grad(n, B, c, d, dMs)
        got = gpu_grad(n, dirty_upper(B, n), c, d, dirty_upper(dMs, n))
        assert not clean[3].any() and not got[3].any()
        for a, b in zip(clean[:3], got[:3]):
            assert np.isfinite(a).all() and np.array_equal(a, b)


@pytest.mark.parametrize("n", [33, 64, 100])
def test_purity_and_optional_outputs(n):
    batch, extra, nparam = 7, 3, 3
    for dt in DTYPES:
        B, c, d = W.inputs(n, batch + extra, dt)
        dMs = W.derivs(n, batch + extra, nparam, dt)
        tb, tc, td, tm = dev(B), dev(c), dev(d), dev(dMs)
        tt = tb.dtype
        grad = torch.full(((batch + extra) * nparam,), 123.0, dtype=tt, device="cuda")
        gradc = torch.full(((batch + extra) * n,), 321.0, dtype=tt, device="cuda")
        alpha = torch.full(((batch + extra) * n,), 77.0, dtype=tt, device="cuda")
        info = torch.full((batch + extra,), -7, dtype=torch.int32, device="cuda")
        # dMs of batchSize matrices only: P is taken from its size
        g, gc, a = api.logml_grad_batched(n, tb, tc, td, tm[:batch * nparam * n * n], grad=grad, gradc=gradc, alpha=alpha, batchSize=batch,
                                          info=info)
        torch.cuda.synchronize()
        assert g is grad and gc is gradc and a is alpha
        assert np.array_equal(tb.cpu().numpy(), B) and np.array_equal(tc.cpu().numpy(), c) and np.array_equal(td.cpu().numpy(), d)
        assert np.array_equal(tm.cpu().numpy(), dMs)
        assert (grad[batch * nparam:] == 123.0).all() and (gradc[batch * n:] == 321.0).all() and (alpha[batch * n:] == 77.0).all()
        assert (info[batch:] == -7).all() and not info[:batch].any()
        full = [t.cpu().numpy() for t in (grad[:batch * nparam], gradc[:batch * n], alpha[:batch * n])]
        ref = W.reference(B[:batch * n * n], c[:batch * n], d[:batch * n], dMs[:batch * nparam * n * n], n, nparam)
        W.check(*full, ref, n, U[np.dtype(dt)], what="batchSize")
        # every non-empty subset of the outputs: the same bits as the full call, and nothing written where nothing was asked
        for mask in range(1, 8):
            outs = [torch.full_like(t, 5.0) if mask >> j & 1 else None for j, t in enumerate((grad, gradc, alpha))]
            with_grad = outs[0] is not None
            raw_grad(n, nparam if with_grad else 0, tb, tc, td, tm if with_grad else None, *outs, batch)
            torch.cuda.synchronize()
            for j, (o, size) in enumerate(zip(outs, (batch * nparam, batch * n, batch * n))):
                if o is not None:
                    assert np.array_equal(o[:size].cpu().numpy(), full[j]), (n, dt, mask, j)
                    assert (o[size:] == 5.0).all()
        # the allocating form returns the same bits as well, and only what was asked for
        g2, gc2, a2 = api.logml_grad_batched(n, tb, tc, td, tm[:batch * nparam * n * n], batchSize=batch)
        assert gc2 is None and a2 is None and g2.numel() == batch * nparam and np.array_equal(g2.cpu().numpy(), full[0])
        g3, gc3, a3 = api.logml_grad_batched(n, tb, tc, td, None, batchSize=batch, want=("gradc", "alpha"))
        assert g3 is None and np.array_equal(gc3.cpu().numpy(), full[1]) and np.array_equal(a3.cpu().numpy(), full[2])


@pytest.mark.parametrize("n", [20, 64, 100])
def test_per_matrix_determinism(n):
    """the result for matrix k depends on matrix k alone: the whole batch, three subsets and one matrix alone give the same bits"""
    nparam = 2
    for dt in DTYPES:
        B, c, d = W.inputs(n, 12, dt)
        dMs = W.derivs(n, 12, nparam, dt)
        whole = gpu_grad(n, B, c, d, dMs)
        assert not whole[3].any()
        Bm, cm, dm, Mm = B.reshape(12, n * n), c.reshape(12, n), d.reshape(12, n), dMs.reshape(12, nparam * n * n)
        for sel in (slice(0, None, 2), slice(1, None, 2), [3, 4, 11], [9]):
            part = gpu_grad(n, Bm[sel].reshape(-1), cm[sel].reshape(-1), dm[sel].reshape(-1), Mm[sel].reshape(-1))
            assert np.array_equal(part[0], whole[0].reshape(12, nparam)[sel].reshape(-1))
            assert np.array_equal(part[1], whole[1].reshape(12, n)[sel].reshape(-1))
            assert np.array_equal(part[2], whole[2].reshape(12, n)[sel].reshape(-1))
        # the gradient of one derivative matrix does not depend on how many others come with it
        one = gpu_grad(n, B, c, d, np.ascontiguousarray(Mm.reshape(12, nparam, n * n)[:, 1]).reshape(-1))
        assert np.array_equal(one[0], whole[0].reshape(12, nparam)[:, 1])


def test_host_form_equals_device_form():
    n, nparam = 40, 2
    for dt in DTYPES:
        B, c, d = W.inputs(n, 11, dt)
        dMs = W.derivs(n, 11, nparam, dt)
        for cc in (c, None):
            grad, gradc, alpha, info = api.logml_grad_batched_host(n, B, cc, d, dMs)
            assert not info.any()
            W.check(grad, gradc, alpha, W.reference(B, cc, d, dMs, n, nparam), n, U[np.dtype(dt)], what="host")
            dg, dgc, da, _ = gpu_grad(n, B, cc, d, dMs)
            assert np.array_equal(grad, dg) and np.array_equal(gradc, dgc) and np.array_equal(alpha, da)
        g, gc, a, info = api.logml_grad_batched_host(n, B, c, d, None, want=("alpha",))
        assert g is None and gc is None and not info.any() and np.array_equal(a, gpu_grad(n, B, c, d, dMs)[2])


def test_grid_stride_and_chunking():
    """one process with the grid held to one round of resident workgroups and the workspace cap at 1 MiB: tests/_logml_grad_worker.py"""
    e = dict(os.environ)
    e.update({"MATINV_TILE_GRID_MULT": "1", "MATINV_BLOCKED_WS_MB": "1"})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_logml_grad_worker.py")], capture_output=True, text=True, env=e,
                       timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "logml-grad-worker ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
