"""Reference, bounds and checks of the leave-one-out tests (tests/test_gpu_loo.py imports them), and the worker of
test_grid_stride_and_chunking: ONE process under MATINV_TILE_GRID_MULT=1 and MATINV_BLOCKED_WS_MB=1 (the library reads each switch once
per process), so that the tile kernels' stride loop runs twice and the global launcher takes several chunks. Exits non-zero at the
first failure and starts nothing after it; prints `loo-worker ok` at the end.

Reference: float64 numpy on the float64 image of exactly what the kernel reads (lower triangle mirrored, c added). K = inv(M):
    kappa_i = K_ii, alpha = K d, mu_i = d_i - alpha_i / kappa_i, s2_i = 1 / kappa_i,
    logpl = sum_i (1/2 log kappa_i - 1/2 alpha_i^2 / kappa_i) - n/2 log(2 pi)

Bounds per matrix k, first order and not tuned: u = 2^-53 (fp64) or 2^-24 (fp32), eps = (n + 4) * u * cond2(M_k)^2,
    |s2^_i - s2_i|    <= eps * s2_i
    |mu^_i - mu_i|    <= eps * (||d_k||_2 + |d_i - mu_i|)
    |logpl^ - logpl|  <= 1/2 eps * (n + sum_i (2 |alpha_i| ||d_k||_2 + alpha_i^2 / kappa_i)) + n * u * max(1, |logpl|)
An inverse computed with backward error n*u has ||dK|| <= n*u*cond*||K||; kappa_i >= ||K|| / cond, so the relative error of kappa is
at most eps; d(alpha_i) / kappa_i <= eps * ||d||_2 because 1 / kappa_i <= ||M||; the +4 covers the diagonal add, the reciprocal and
the division, which dominate at n = 1.
"""
import importlib
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from conftest import as_mats, spd_batch  # noqa: E402

U = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}


def image(B, c, n):
    """(batch, n, n) float64: the matrices M = B + diag c as the kernel reads them (lower triangle of B only)"""
    m = as_mats(B, n).astype(np.float64)
    M = np.tril(m) + np.tril(m, -1).transpose(0, 2, 1)
    if c is not None:
        M = M + np.stack([np.diag(v) for v in np.asarray(c, dtype=np.float64).reshape(-1, n)])
    return M


def reference(B, c, d, n, idx=None):
    """the identities above in float64; idx: the matrices to compute (the others may be not SPD)"""
    M = image(B, c, n)
    dd = np.asarray(d, dtype=np.float64).reshape(-1, n)
    if idx is not None:
        M, dd = M[idx], dd[idx]
    K = np.linalg.inv(M)
    kappa = np.einsum("kii->ki", K)
    alpha = np.einsum("kij,kj->ki", K, dd)
    return {
        "M": M, "d": dd, "kappa": kappa, "alpha": alpha, "mu": dd - alpha / kappa, "s2": 1.0 / kappa,
        "logpl": (0.5 * np.log(kappa) - 0.5 * alpha * alpha / kappa).sum(axis=1) - 0.5 * n * math.log(2 * math.pi),
        "cond": np.linalg.cond(M), "dnorm": np.linalg.norm(dd, axis=1),
    }


def bounds(ref, n, u):
    """(b_mean[k, i], b_var[k, i], b_logpl[k]) of the module docstring"""
    eps = (n + 4) * u * ref["cond"] ** 2
    b_var = eps[:, None] * ref["s2"]
    b_mean = eps[:, None] * (ref["dnorm"][:, None] + np.abs(ref["d"] - ref["mu"]))
    s = (2 * np.abs(ref["alpha"]) * ref["dnorm"][:, None] + ref["alpha"] ** 2 / ref["kappa"]).sum(axis=1)
    b_logpl = 0.5 * eps * (n + s) + n * u * np.maximum(1.0, np.abs(ref["logpl"]))
    return b_mean, b_var, b_logpl


def check(mean, var, logpl, ref, n, u, idx=None, what="", factor=1.0):
    """every requested output (None: not requested) of the matrices idx within factor * bound; prints err / bound first"""
    b_mean, b_var, b_logpl = bounds(ref, n, u)
    sel = slice(None) if idx is None else idx
    ratios = {}
    if mean is not None:
        ratios["mean"] = np.abs(np.asarray(mean, dtype=np.float64).reshape(-1, n)[sel] - ref["mu"]) / b_mean
    if var is not None:
        ratios["var"] = np.abs(np.asarray(var, dtype=np.float64).reshape(-1, n)[sel] - ref["s2"]) / b_var
    if logpl is not None:
        ratios["logpl"] = np.abs(np.asarray(logpl, dtype=np.float64)[sel] - ref["logpl"]) / b_logpl
    print(f"  {what} n={n} cond={ref['cond'].max():.2f} err/bound: " + " ".join(f"{k}={v.max():.3f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert np.isfinite(v).all() and (v <= factor).all(), (what, n, k, float(np.nanmax(v)))


def inputs(n, batch, dt, with_c=True, seed=None):
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    B = spd_batch(n, batch, seed=n if seed is None else seed, dtype=dt)
    c = rng.uniform(0.1, 2.0, batch * n).astype(dt) if with_c else None
    d = rng.standard_normal(batch * n).astype(dt)
    return B, c, d


def break_three(B, c, n, at):
    """matrix at[0]: last diagonal -1 (info n); at[1]: memory column 1 zeroed (info 2); at[2]: all zero (info 1). Memory is [k, col, row].
    Their c, when there is one, becomes zero: M = B for them."""
    m = B.reshape(-1, n, n)
    if c is not None:
        c.reshape(-1, n)[list(at)] = 0.0
    m[at[0], n - 1, n - 1] = -1.0
    m[at[1], 1, :] = 0.0
    m[at[2]] = 0.0
    return {at[0]: n, at[1]: 2, at[2]: 1}


def check_with_rejects(got_mean, got_var, got_logpl, got_info, B, c, d, n, dt, want_info, what=""):
    """info as expected, all three outputs NaN exactly at the not-SPD matrices, finite and within the bounds elsewhere"""
    batch = got_info.size
    bad = sorted(want_info)
    ok = np.array([k for k in range(batch) if k not in want_info])
    expect = np.zeros(batch, dtype=np.int64)
    for k, v in want_info.items():
        expect[k] = v
    assert np.array_equal(got_info, expect), (what, n, got_info[bad], [want_info[k] for k in bad], np.flatnonzero(got_info != expect)[:10])
    m, v = got_mean.reshape(batch, n), got_var.reshape(batch, n)
    assert np.isnan(m[bad]).all() and np.isnan(v[bad]).all() and np.isnan(got_logpl[bad]).all(), (what, n)
    assert np.isfinite(m[ok]).all() and np.isfinite(v[ok]).all() and np.isfinite(got_logpl[ok]).all(), (what, n)
    check(got_mean, got_var, got_logpl, reference(B, c, d, n, idx=ok), n, U[np.dtype(dt)], idx=ok, what=what)


def run(api, torch, n, batch, dt, with_c, rejects_at=None):
    B, c, d = inputs(n, batch, dt, with_c)
    want_info = break_three(B, c, n, rejects_at) if rejects_at else {}
    dev = lambda x: None if x is None else torch.from_numpy(x).cuda()  # noqa: E731
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    mean, var, logpl = api.loo_batched(n, dev(B), dev(c), dev(d), info=info)
    torch.cuda.synchronize()
    what = f"{api.loo_kernel_name(dt, n)} batch={batch}"
    check_with_rejects(mean.cpu().numpy(), var.cpu().numpy(), logpl.cpu().numpy(), info.cpu().numpy(), B, c, d, n, dt, want_info, what)


def main():
    import torch
    api = importlib.import_module("cuda-matrix-inversion_amd.api")
    assert os.environ.get("MATINV_TILE_GRID_MULT") == "1" and os.environ.get("MATINV_BLOCKED_WS_MB") == "1"
    # 5000 matrices on a grid of 256 * 12 = 3072 workgroups: the stride loop runs twice; the rejects sit in the second round.
    run(api, torch, 48, 5000, np.float64, True, rejects_at=(3100, 4000, 4999))
    run(api, torch, 64, 5000, np.float32, False, rejects_at=(3073, 3500, 4998))
    # 40 working copies of 80 000 bytes under a cap of 1 MiB: four chunks, three of them with a non-zero `first`
    run(api, torch, 100, 40, np.float64, True)
    run(api, torch, 100, 40, np.float64, False, rejects_at=(14, 27, 39))
    print("loo-worker ok")


if __name__ == "__main__":
    main()
