"""Reference, bounds and checks of the log-marginal-likelihood gradient tests (tests/test_gpu_logml_grad.py and
tests/test_logml_grad_cpu.py import them), and the worker of test_grid_stride_and_chunking: ONE process under MATINV_TILE_GRID_MULT=1 and
MATINV_BLOCKED_WS_MB=1 (the library reads each switch once per process), so that the tile kernels' stride loop runs twice and the global
launcher takes several chunks. Exits non-zero at the first failure and starts nothing after it; prints `logml-grad-worker ok` at the end.

Reference: float64 numpy on the float64 image of exactly what the kernel reads: the lower triangles of B and of every dM_p mirrored, and
the diagonal B_ii + c_i rounded in the working precision, as the kernel adds it. K = inv(M), alpha = K d, G = alpha alpha^T - K:
    grad_p = 1/2 sum_ij G_ij dM_p[i, j]      gradc_i = 1/2 (alpha_i^2 - K_ii)

Bounds per matrix, first order and not tuned: u = 2^-53 (fp64) or 2^-24 (fp32), eps = (n + 4) * u * cond2(M)^2 as in _loo_worker.bounds,
    |alpha^_i - alpha_i|  <= eps * ||alpha||_2
    |gradc^_i - gradc_i|  <= eps * (||alpha||_2^2 + ||K||_2)
    |grad^_p - grad_p|    <= eps * (||alpha||_2^2 + ||K||_F) * ||dM_p||_F + n^2 * u * sum_ij |G_ij dM_p[i, j]|
An inverse computed with backward error n u has ||dK|| <= n u cond ||K||, and alpha = K d inherits ||d alpha|| <= n u cond ||K|| ||d|| <=
n u cond^2 ||alpha|| because ||d|| <= ||M|| ||alpha||: that is eps ||alpha||, the +4 covering the diagonal add and the last operations at
n = 1. To first order d(alpha_i^2) = 2 alpha_i d alpha_i <= 2 eps ||alpha||^2 and d K_ii <= eps ||K||_2 / cond, so with the factor 1/2 of
gradc the bound is eps (||alpha||^2 + ||K||_2). For grad, Cauchy-Schwarz on 1/2 sum dG_ij dM_ij with ||d(alpha alpha^T)||_F <= 2 eps
||alpha||^2 and ||dK||_F <= eps ||K||_F gives the first term; the second is the rounding of the n^2 products and of their sum in any
order (n^2 u times the sum of the magnitudes, the classical bound of a recursive sum, loose for the trees the kernels use). No constant
is fitted: tests/test_logml_grad_cpu.py confirms that a float32 numpy evaluation of the same formulas stays inside the fp32 bounds at
every size the GPU tests use.
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _loo_worker as L  # noqa: E402
from conftest import as_mats  # noqa: E402

U = L.U
inputs = L.inputs
break_three = L.break_three

TILE_SIZES = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96]
GLOBAL_SIZES = [97, 130, 200]


def batch_of(n):
    return 13 if n <= 64 else 5


def sym_lower(flat, n):
    """(count, n, n) float64 from a flat column-major batch: the lower triangles, mirrored"""
    m = as_mats(flat, n).astype(np.float64)
    return np.tril(m) + np.tril(m, -1).transpose(0, 2, 1)


def image(B, c, n):
    """(batch, n, n) float64: M = B + diag c as the kernel reads it -- lower triangle of B only, the diagonal sum rounded in B's dtype"""
    M = sym_lower(B, n)
    if c is not None:
        dt = np.asarray(B).dtype
        diag = (np.asarray(B).reshape(-1, n * n)[:, ::n + 1].astype(dt) + np.asarray(c, dtype=dt).reshape(-1, n)).astype(np.float64)
        idx = np.arange(n)
        M[:, idx, idx] = diag
    return M


def derivs(n, batch, nparam, dt, seed=None):
    """batch * nparam random symmetric matrices with entries of order 1 (N(0, 1)), flat column-major"""
    rng = np.random.default_rng(7000 + 31 * n + nparam if seed is None else seed)
    a = rng.standard_normal((batch * nparam, n, n))
    return np.ascontiguousarray((a + a.transpose(0, 2, 1)) / np.sqrt(2.0)).reshape(-1).astype(dt)


def reference(B, c, d, dMs, n, nparam, idx=None):
    """the formulas above in float64; idx: the matrices to compute (the others may be not SPD)"""
    M = image(B, c, n)
    batch = M.shape[0]
    dd = np.asarray(d, dtype=np.float64).reshape(-1, n)
    dM = None if dMs is None else sym_lower(dMs, n).reshape(batch, nparam, n, n)
    if idx is not None:
        M, dd = M[idx], dd[idx]
        dM = None if dM is None else dM[idx]
    K = np.linalg.inv(M)
    alpha = np.einsum("kij,kj->ki", K, dd)
    G = alpha[:, :, None] * alpha[:, None, :] - K
    ref = {"M": M, "d": dd, "K": K, "alpha": alpha, "G": G, "dM": dM, "cond": np.linalg.cond(M),
           "gradc": 0.5 * (alpha ** 2 - np.einsum("kii->ki", K))}
    if dM is not None:
        ref["grad"] = 0.5 * np.einsum("kij,kpij->kp", G, dM)
    return ref


def bounds(ref, n, u):
    """(b_grad[k, p] or None, b_gradc[k], b_alpha[k]) of the module docstring"""
    eps = (n + 4) * u * ref["cond"] ** 2
    an = np.linalg.norm(ref["alpha"], axis=1)
    b_alpha = eps * an
    b_gradc = eps * (an ** 2 + np.linalg.norm(ref["K"], 2, axis=(1, 2)))
    b_grad = None
    if ref["dM"] is not None:
        kf = np.linalg.norm(ref["K"], "fro", axis=(1, 2))
        dmf = np.linalg.norm(ref["dM"], "fro", axis=(2, 3))
        mag = np.abs(ref["G"][:, None] * ref["dM"]).sum(axis=(2, 3))
        b_grad = (eps * (an ** 2 + kf))[:, None] * dmf + n * n * u * mag
    return b_grad, b_gradc, b_alpha


def ratios(grad, gradc, alpha, ref, n, u, idx=None):
    """err / bound of every given output (None: not requested) of the matrices idx"""
    b_grad, b_gradc, b_alpha = bounds(ref, n, u)
    sel = slice(None) if idx is None else idx
    out = {}
    if grad is not None:
        out["grad"] = np.abs(np.asarray(grad, dtype=np.float64).reshape(-1, ref["grad"].shape[1])[sel] - ref["grad"]) / b_grad
    if gradc is not None:
        out["gradc"] = np.abs(np.asarray(gradc, dtype=np.float64).reshape(-1, n)[sel] - ref["gradc"]) / b_gradc[:, None]
    if alpha is not None:
        out["alpha"] = np.abs(np.asarray(alpha, dtype=np.float64).reshape(-1, n)[sel] - ref["alpha"]) / b_alpha[:, None]
    return out


def check(grad, gradc, alpha, ref, n, u, idx=None, what="", factor=1.0):
    """every given output within factor * bound; prints err / bound first"""
    rs = ratios(grad, gradc, alpha, ref, n, u, idx)
    print(f"  {what} n={n} cond={ref['cond'].max():.2f} err/bound: " + " ".join(f"{k}={v.max():.3f}" for k, v in rs.items()))
    for k, v in rs.items():
        assert np.isfinite(v).all() and (v <= factor).all(), (what, n, k, float(np.nanmax(v)))


def float32_evaluation(B, c, d, dMs, n, nparam):
    """the reference formulas evaluated in float32 numpy on the float32 inputs: what any fp32 implementation of them may expect"""
    f = np.float32
    m = as_mats(B, n).astype(f)
    M = np.tril(m) + np.tril(m, -1).transpose(0, 2, 1)
    batch = M.shape[0]
    if c is not None:
        idx = np.arange(n)
        M[:, idx, idx] = M[:, idx, idx] + np.asarray(c, dtype=f).reshape(-1, n)
    dm = as_mats(dMs, n).astype(f)
    dM = (np.tril(dm) + np.tril(dm, -1).transpose(0, 2, 1)).reshape(batch, nparam, n, n)
    K = np.linalg.inv(M)
    assert K.dtype == f
    alpha = np.einsum("kij,kj->ki", K, np.asarray(d, dtype=f).reshape(-1, n))
    G = alpha[:, :, None] * alpha[:, None, :] - K
    grad = f(0.5) * np.einsum("kij,kpij->kp", G, dM)
    gradc = f(0.5) * (alpha * alpha - np.einsum("kii->ki", K))
    assert grad.dtype == f and gradc.dtype == f and alpha.dtype == f
    return grad, gradc, alpha


def check_with_rejects(grad, gradc, alpha, info, B, c, d, dMs, n, nparam, dt, want_info, what=""):
    """info as expected, every output NaN exactly at the not-SPD matrices, finite and within the bounds elsewhere"""
    batch = info.size
    bad = sorted(want_info)
    ok = np.array([k for k in range(batch) if k not in want_info])
    expect = np.zeros(batch, dtype=np.int64)
    for k, v in want_info.items():
        expect[k] = v
    assert np.array_equal(info, expect), (what, n, info[bad], [want_info[k] for k in bad], np.flatnonzero(info != expect)[:10])
    outs = (grad.reshape(batch, nparam), gradc.reshape(batch, n), alpha.reshape(batch, n))
    for o in outs:
        assert np.isnan(o[bad]).all(), (what, n)
        assert np.isfinite(o[ok]).all(), (what, n)
    check(grad, gradc, alpha, reference(B, c, d, dMs, n, nparam, idx=ok), n, U[np.dtype(dt)], idx=ok, what=what)


def run(api, torch, n, batch, nparam, dt, with_c, rejects_at=None):
    B, c, d = inputs(n, batch, dt, with_c)
    dMs = derivs(n, batch, nparam, dt)
    want_info = break_three(B, c, n, rejects_at) if rejects_at else {}
    dev = lambda x: None if x is None else torch.from_numpy(x).cuda()  # noqa: E731
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    grad, gradc, alpha = api.logml_grad_batched(n, dev(B), dev(c), dev(d), dev(dMs), info=info, want=("grad", "gradc", "alpha"))
    torch.cuda.synchronize()
    what = f"{api.logml_grad_kernel_name(dt, n)} batch={batch} P={nparam}"
    check_with_rejects(grad.cpu().numpy(), gradc.cpu().numpy(), alpha.cpu().numpy(), info.cpu().numpy(), B, c, d, dMs, n, nparam, dt,
                       want_info, what)


def main():
    import torch
    api = importlib.import_module("cuda-matrix-inversion_amd.api")
    assert os.environ.get("MATINV_TILE_GRID_MULT") == "1" and os.environ.get("MATINV_BLOCKED_WS_MB") == "1"
    # 4000 matrices on a grid of 256 * 12 = 3072 workgroups: the stride loop runs twice; the rejects sit in the second round.
    run(api, torch, 33, 4000, 2, np.float64, True, rejects_at=(3073, 3500, 3999))
    run(api, torch, 33, 4000, 1, np.float32, False, rejects_at=(3100, 3600, 3998))
    # 20 working copies of 135 200 bytes under a cap of 1 MiB: three chunks, two of them with a non-zero `first`
    run(api, torch, 130, 20, 2, np.float64, True)
    run(api, torch, 130, 20, 2, np.float64, False, rejects_at=(7, 13, 19))
    print("logml-grad-worker ok")


if __name__ == "__main__":
    main()
