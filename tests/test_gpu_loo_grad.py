"""Gradients of the batched GP leave-one-out log pseudo-likelihood (matinv_loo_grad_batched) on the GPU against float64 numpy on the
float64 image of exactly what the kernel reads. Reference, bounds and their derivation: tests/_loo_grad_worker.py (first order, not
tuned; err / bound is printed; tests/test_loo_grad_cpu.py holds a float32 numpy evaluation against the same bounds, and the reference
against finite differences).

The generated instantiation sweep (tests/_instantiations.py) has no route for the LOO-gradient forms, so this file runs the tile forms at
both ends of every instantiation's size range itself, and the global form either side of its lower end and at n = 1024."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _loo_grad_worker as W
import test_loo_grad_cpu as C
from conftest import as_mats, pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
api = pkg("api")
lib = pkg("_lib")
U = W.U
DTYPES = (np.float64, np.float32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = W.OUTPUTS


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def gpu_grad(n, B, c, d, dMs):
    """(grad, gradc, logpl, info) as numpy; checks that the inputs are bitwise unchanged"""
    tb, tc, td, tm = dev(B), dev(c), dev(d), dev(dMs)
    batch = B.size // (n * n)
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    grad, gradc, logpl = api.loo_grad_batched(n, tb, tc, td, tm, info=info, want=ALL)
    torch.cuda.synchronize()
    assert np.array_equal(tb.cpu().numpy(), B, equal_nan=True) and np.array_equal(td.cpu().numpy(), d), "an input was modified"
    assert np.array_equal(tm.cpu().numpy(), dMs, equal_nan=True), "dMs was modified"
    assert c is None or np.array_equal(tc.cpu().numpy(), c), "c was modified"
    return grad.cpu().numpy(), gradc.cpu().numpy(), logpl.cpu().numpy(), info.cpu().numpy()


def raw_grad(n, nparam, tb, tc, td, tm, grad, gradc, logpl, batch, info=None):
    """the C entry point itself: any of grad / gradc / logpl may be None (NULL)"""
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    code = api.F64 if tb.dtype == torch.float64 else api.F32
    lib.check(lib.lib().matinv_loo_grad_batched(code, n, nparam, p(tb), p(tc), p(td), p(tm), p(grad), p(gradc), p(logpl), batch, p(info),
                                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


@pytest.mark.parametrize("n", W.TILE_SIZES + W.GLOBAL_SIZES)
def test_accuracy(n):
    batch = W.batch_of(n)
    for dt in DTYPES:
        name = api.loo_grad_kernel_name(dt, n)
        assert name.startswith("matinv_spd_tile_f" if n <= 96 else "matinv_chol_global<") and name.endswith(", true, true, true, true, true>")
        for nparam in (3, 1) if n in (16, 64, 96) else (3,):
            for with_c in (True, False):
                B, c, d = W.inputs(n, batch, dt, with_c)
                dMs = W.derivs(n, batch, nparam, dt)
                grad, gradc, logpl, info = gpu_grad(n, B, c, d, dMs)
                assert not info.any(), (n, dt, info)
                W.check(grad, gradc, logpl, W.reference(B, c, d, dMs, n, nparam), n, U[np.dtype(dt)],
                        what=f"{name} P={nparam} c={'yes' if with_c else 'no'}")


def test_accuracy_1024():
    n = 1024
    B, c, d = W.inputs(n, 2, np.float64)
    dMs = W.derivs(n, 2, 1, np.float64)
    grad, gradc, logpl, info = gpu_grad(n, B, c, d, dMs)
    assert not info.any()
    W.check(grad, gradc, logpl, W.reference(B, c, d, dMs, n, 1), n, U[np.dtype(np.float64)], what=api.loo_grad_kernel_name(np.float64, n))


def flat_sym(mats, dt):
    """(count, n, n) symmetric matrices -> flat column-major batch"""
    return np.ascontiguousarray(mats.transpose(0, 2, 1)).reshape(-1).astype(dt)


@pytest.mark.parametrize("n", [17, 64, 96])
def test_identity_inputs(n):
    """dM_0 = M, dM_1 = e_i e_i^T with i in the last tile row, dM_2 = e_0 e_0^T against the two identities of the reference
    (tests/test_loo_grad_cpu.py): the contraction path crossed with the diagonal-extraction path, every tile touched by dM_0"""
    batch, i = 5, n - 1
    for dt in DTYPES:
        u = U[np.dtype(dt)]
        B, c, d = W.inputs(n, batch, dt)
        M = W.image(B, c, n)  # exactly representable in dt: the diagonal was rounded in dt
        dMs = C.identity_derivs(M, n, i).astype(dt)
        assert np.array_equal(W.sym_lower(dMs, n).reshape(batch, 3, n, n)[:, 0], M)
        grad, gradc, logpl, info = gpu_grad(n, B, c, d, dMs)
        assert not info.any()
        ref = W.reference(B, c, d, dMs, n, 3)
        W.check(grad, gradc, logpl, ref, n, u, what=f"dM = M, e_i e_i^T, e_0 e_0^T {np.dtype(dt).name}")
        b_grad, b_gradc, _ = W.bounds(ref, n, u)
        g = grad.astype(np.float64).reshape(batch, 3)
        gc = gradc.astype(np.float64).reshape(batch, n)
        closed = C.identity_targets(ref, n, i)[:, 0]
        r_m = np.abs(g[:, 0] - closed) / (b_grad[:, 0] + W.bounds(ref, n, U[np.dtype(np.float64)])[0][:, 0])
        r_i = np.abs(g[:, 1] - gc[:, i]) / (b_grad[:, 1] + b_gradc)
        r_0 = np.abs(g[:, 2] - gc[:, 0]) / (b_grad[:, 2] + b_gradc)
        print(f"  {np.dtype(dt).name} n={n} err/bound: dM=M vs closed form {r_m.max():.3f}  e_i vs gradc_i {r_i.max():.3f}  e_0 vs gradc_0 {r_0.max():.3f}")
        assert (r_m <= 1).all() and (r_i <= 1).all() and (r_0 <= 1).all()


def test_single_element_derivatives():
    """n = 96, one dM per lower tile with a single symmetric pair (i, j) set to 1: grad_p = 2 G_ij (G_ii on the diagonal). A wrong or
    missed tile of H or of the contraction costs an error of the order of the value itself"""
    n, batch = 96, 3
    pairs = []
    for ti in range(6):
        for tj in range(ti + 1):
            a, b = (5 * ti + 3 * tj + 1) % 16, (7 * tj + 2 * ti + 4) % 16
            if ti == tj and (ti % 2 == 0 or a == b):
                b = a if ti % 2 == 0 else (a + 1) % 16  # diagonal tiles: a diagonal element in one, an off-diagonal one in the next
            pairs.append((16 * ti + max(a, b), 16 * tj + min(a, b)) if ti == tj else (16 * ti + a, 16 * tj + b))
    nparam = len(pairs)
    assert nparam == 21 and len({(i // 16, j // 16) for i, j in pairs}) == 21 and all(i >= j for i, j in pairs)
    assert any(i == j for i, j in pairs) and any(i != j and i // 16 == j // 16 for i, j in pairs)
    dM = np.zeros((batch, nparam, n, n))
    for p, (i, j) in enumerate(pairs):
        dM[:, p, i, j] = dM[:, p, j, i] = 1.0
    for dt in DTYPES:
        B, c, d = W.inputs(n, batch, dt)
        dMs = flat_sym(dM.reshape(-1, n, n), dt)
        grad, gradc, logpl, info = gpu_grad(n, B, c, d, dMs)
        assert not info.any()
        ref = W.reference(B, c, d, dMs, n, nparam)
        # the reference's H is a matmul and symmetric to rounding only: G_ij + G_ji is what its sum holds, 2 G_ij what it means
        want = np.stack([ref["G"][:, i, j] if i == j else ref["G"][:, i, j] + ref["G"][:, j, i] for i, j in pairs], axis=1)
        assert np.array_equal(ref["grad"], want)
        assert np.allclose(want, np.stack([(1.0 if i == j else 2.0) * ref["G"][:, i, j] for i, j in pairs], axis=1), rtol=1e-10, atol=1e-16)
        W.check(grad, gradc, logpl, ref, n, U[np.dtype(dt)], what=f"single elements {np.dtype(dt).name}")


@pytest.mark.parametrize("n,dt", [(48, np.float64), (64, np.float32), (130, np.float64), (130, np.float32)])
def test_not_spd_reports_info(n, dt):
    nparam = 2
    B, _, d = W.inputs(n, 8, dt, with_c=False)
    dMs = W.derivs(n, 8, nparam, dt)
    want = W.break_three(B, None, n, (1, 3, 6))
    assert want == {1: n, 3: 2, 6: 1}
    grad, gradc, logpl, info = gpu_grad(n, B, None, d, dMs)
    W.check_with_rejects(grad, gradc, logpl, info, B, None, d, dMs, n, nparam, dt, want, what=f"not SPD {np.dtype(dt).name}")


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
        logpl = torch.full((batch + extra,), 77.0, dtype=tt, device="cuda")
        info = torch.full((batch + extra,), -7, dtype=torch.int32, device="cuda")
        # dMs of batchSize matrices only: P is taken from its size
        g, gc, lp = api.loo_grad_batched(n, tb, tc, td, tm[:batch * nparam * n * n], grad=grad, gradc=gradc, logpl=logpl, batchSize=batch,
                                         info=info)
        torch.cuda.synchronize()
        assert g is grad and gc is gradc and lp is logpl
        assert np.array_equal(tb.cpu().numpy(), B) and np.array_equal(tc.cpu().numpy(), c) and np.array_equal(td.cpu().numpy(), d)
        assert np.array_equal(tm.cpu().numpy(), dMs)
        assert (grad[batch * nparam:] == 123.0).all() and (gradc[batch * n:] == 321.0).all() and (logpl[batch:] == 77.0).all()
        assert (info[batch:] == -7).all() and not info[:batch].any()
        full = [t.cpu().numpy() for t in (grad[:batch * nparam], gradc[:batch * n], logpl[:batch])]
        ref = W.reference(B[:batch * n * n], c[:batch * n], d[:batch * n], dMs[:batch * nparam * n * n], n, nparam)
        W.check(*full, ref, n, U[np.dtype(dt)], what="batchSize")
        # every non-empty subset of the outputs: the same bits as the full call, and nothing written where nothing was asked
        for mask in range(1, 8):
            outs = [torch.full_like(t, 5.0) if mask >> j & 1 else None for j, t in enumerate((grad, gradc, logpl))]
            with_grad = outs[0] is not None
            raw_grad(n, nparam if with_grad else 0, tb, tc, td, tm if with_grad else None, *outs, batch)
            torch.cuda.synchronize()
            for j, (o, size) in enumerate(zip(outs, (batch * nparam, batch * n, batch))):
                if o is not None:
                    assert np.array_equal(o[:size].cpu().numpy(), full[j]), (n, dt, mask, j)
                    assert (o[size:] == 5.0).all()
        # the allocating form returns the same bits as well, and only what was asked for
        g2, gc2, lp2 = api.loo_grad_batched(n, tb, tc, td, tm[:batch * nparam * n * n], batchSize=batch)
        assert gc2 is None and lp2 is None and g2.numel() == batch * nparam and np.array_equal(g2.cpu().numpy(), full[0])
        g3, gc3, lp3 = api.loo_grad_batched(n, tb, tc, td, None, batchSize=batch, want=("gradc", "logpl"))
        assert g3 is None and np.array_equal(gc3.cpu().numpy(), full[1]) and np.array_equal(lp3.cpu().numpy(), full[2])


@pytest.mark.parametrize("n", [20, 64, 96, 100])
def test_locality_bit_for_bit(n):
    """the result for matrix k depends on matrix k alone, and grad[k, p] on dM_p alone: a permutation of the batch permutes the results;
    replacing the other dM of a matrix, permuting the p, and P = 1 with dM_p alone leave grad[k, p] unchanged"""
    nparam, batch = 3, 12
    for dt in DTYPES:
        B, c, d = W.inputs(n, batch, dt)
        dMs = W.derivs(n, batch, nparam, dt)
        whole = gpu_grad(n, B, c, d, dMs)
        assert not whole[3].any()
        Bm, cm, dm, Mm = B.reshape(batch, n * n), c.reshape(batch, n), d.reshape(batch, n), dMs.reshape(batch, nparam, n * n)
        perm = np.random.default_rng(n).permutation(batch)
        for sel in (perm, [3, 4, 11], [9]):
            part = gpu_grad(n, Bm[sel].reshape(-1), cm[sel].reshape(-1), dm[sel].reshape(-1), Mm[sel].reshape(-1))
            assert np.array_equal(part[0], whole[0].reshape(batch, nparam)[sel].reshape(-1))
            assert np.array_equal(part[1], whole[1].reshape(batch, n)[sel].reshape(-1))
            assert np.array_equal(part[2], whole[2][sel])
        g = whole[0].reshape(batch, nparam)
        other = W.derivs(n, batch, nparam, dt, seed=99).reshape(batch, nparam, n * n)
        for p in range(nparam):
            mixed = other.copy()
            mixed[:, p] = Mm[:, p]
            assert np.array_equal(gpu_grad(n, B, c, d, mixed.reshape(-1))[0].reshape(batch, nparam)[:, p], g[:, p]), (n, dt, p, "others replaced")
            one = gpu_grad(n, B, c, d, np.ascontiguousarray(Mm[:, p]).reshape(-1))
            assert np.array_equal(one[0], g[:, p]), (n, dt, p, "P = 1")
        order = [2, 0, 1]
        shuffled = gpu_grad(n, B, c, d, np.ascontiguousarray(Mm[:, order]).reshape(-1))
        assert np.array_equal(shuffled[0].reshape(batch, nparam), g[:, order]), (n, dt, "p permuted")


def test_host_form_equals_device_form():
    n, nparam = 40, 2
    for dt in DTYPES:
        B, c, d = W.inputs(n, 11, dt)
        dMs = W.derivs(n, 11, nparam, dt)
        for cc in (c, None):
            grad, gradc, logpl, info = api.loo_grad_batched_host(n, B, cc, d, dMs)
            assert not info.any()
            W.check(grad, gradc, logpl, W.reference(B, cc, d, dMs, n, nparam), n, U[np.dtype(dt)], what="host")
            dg, dgc, dlp, _ = gpu_grad(n, B, cc, d, dMs)
            assert np.array_equal(grad, dg) and np.array_equal(gradc, dgc) and np.array_equal(logpl, dlp)
        g, gc, lp, info = api.loo_grad_batched_host(n, B, c, d, None, want=("logpl",))
        assert g is None and gc is None and not info.any() and np.array_equal(lp, gpu_grad(n, B, c, d, dMs)[2])


def test_grid_stride_and_chunking():
    """one process with the grid held to one round of resident workgroups and the workspace cap at 1 MiB: tests/_loo_grad_worker.py"""
    e = dict(os.environ)
    e.update({"MATINV_TILE_GRID_MULT": "1", "MATINV_BLOCKED_WS_MB": "1"})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_loo_grad_worker.py")], capture_output=True, text=True, env=e,
                       timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "loo-grad-worker ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
