"""Reference, inputs, bounds and checks of the tests of the GP log marginal likelihood from coordinates (tests/test_gpu_ard.py and
tests/test_ard_cpu.py import them), and the worker of test_grid_stride_and_chunking: ONE process under MATINV_TILE_GRID_MULT=1 and
MATINV_BLOCKED_WS_MB=1 (the library reads each switch once per process), so that the tile kernels' stride loop runs several rounds and the
global launcher takes several chunks. The worker is given a file of the outputs of the same calls made under the default switches, which
the test has checked against the reference before: it asserts equal bits, exits non-zero at the first failure and starts nothing after it;
prints `ard-worker ok` at the end.

Reference: longdouble / float64 numpy on the float64 image of exactly the inputs the kernel reads (fp32: the float32 values widened).
theta = (log sf2, log l_1 .. log l_d, log sn2), z_ik = x_ik / l_k, s_ij = sum_k (z_ik - z_jk)^2,
    M = sf2 phi(s) + sn2 I,  K = inv(M),  alpha = K y,  G = alpha alpha^T - K,
    SE: phi = exp(-s/2), psi = phi;   MATERN52: phi = (1 + a + 5 s / 3) exp(-a), psi = 5/3 (1 + a) exp(-a), a = sqrt(5 s)   (psi = -2 phi')
    logml = -1/2 (y^T alpha + log det M + n log 2 pi)        (log det: Cholesky diagonal in longdouble, _whiten_worker.logdet_longdouble)
    grad = 1/2 sum_ij G_ij dM_p[i, j],  dM_0 = sf2 phi,  dM_{1+k} = sf2 psi (z_ik - z_jk)^2,  dM_{d+1} = sn2 I
The reference also returns M, K, G, s, phi, psi and the dM_p for the bounds.

Inputs (chosen so that the reference alone stays well conditioned): points uniform in [0, n^(1/d)]^d (unit density), l_k in [0.5, 1],
sf2 in [0.5, 2], sn2 in [0.3, 0.6] sf2, y standard normal. cond2(M) stayed below 45 over every size, d and kind tried;
tests/test_ard_cpu.py asserts cond2(M) <= COND_CAP = 64 for every matrix the GPU tests use. A draw that breaks the cap takes another seed.

Bounds, first order and derived, not fitted. u = 2^-53 (fp64) or 2^-24 (fp32). Each bound has two parts.
(1) The bound the project already uses for the same output ON A GIVEN M, with the exact dM_p: eps = (n + 4) u cond2(M)^2,
    alpha   eps ||alpha||_2                                                                   (_logml_grad_worker)
    logml   _multi_target_worker.bounds with D = 1 (quad, logdet and the roundings of the last three operations)
    grad_p  eps (||alpha||^2 + ||K||_F) ||dM_p||_F + (n^2 + 2) u sum_ij |G_ij dM_p[i, j]|     (_logml_grad_worker; + 2: the weight and
            the product that forms the element of dM_p on the fly)
(2) The propagated GENERATION error of M and of every dM_p. Counted roundings, E = 4 u the documented error (below 2 ulp) of the device
    exponential (csrc/ard_element.hpp), sqrt correctly rounded up to 2 u:
      sf2, sn2, l_k        relative error E                    (one exponential of an exact input)
      z_ik                 E (common to column k: it scales every difference alike) and u of its own (the division)
      D_k = z_ik - z_jk    |dD_k| <= u (|z_ik| + |z_jk|) + (E + u) |D_k|                      (the two divisions, l_k, the subtraction)
      s                    ds <= sum_k 2 |D_k| |dD_k| + d u s                                 (d fused multiply-adds)
                              <= u [ 2 sum_k |D_k| (|z_ik| + |z_jk|) + (2 (4 + 1) + d) s ];  on the diagonal D_k = 0 and s = 0 exactly
      phi                  SE: |dphi| <= phi (ds / 2 + E)        (-s/2 is exact; |phi'| = phi / 2)
                           M52: |dphi| <= psi / 2 ds + phi u (10 + 4 a)
                                (|phi'| = psi / 2; a = sqrt5 sqrt s carries 2 u + 2 u on top of ds, the exponential answers an argument
                                error a * 4 u with a relative error of that size; 1 + a, 5/3, 5/3 s, the sum, the product: 6 u; E)
      psi                  SE: as phi.  M52: |dpsi| <= 25/6 exp(-a) ds + psi u (10 + 4 a)    (psi' = -25/6 exp(-a))
      M_ij                 |dM_ij| <= sf2 |dphi| + (E + u) sf2 phi + tiny,  i != j;  |dM_ii| <= (E + 2 u) M_ii
                           tiny = sf2 times the smallest normal number: the underflow of the exponential
      dM_0                 as M off the diagonal; (E + u) sf2 on it.   dM_{d+1} = sn2 I: E sn2.
      dM_{1+k}             sf2 |dpsi| D_k^2 + sf2 psi (2 |D_k| |dD_k| + u D_k^2) + (E + 2 u) |dM_{1+k}|
    For the usual s this is u (a + b s) |M_ij| with a, b of order 10 + d, the dependence on s coming from |s phi' / phi|.
    Propagation, componentwise (|.| of a matrix is taken element by element):
      |d alpha|   <= |K| |dM| |alpha|
      |d logml|   <= 1/2 (|alpha|^T |dM| |alpha| + sum_ij |K_ij| |dM_ij|)                     (d quad = -alpha^T dM alpha, d logdet = tr(K dM))
      |d grad_p|  <= 1/2 sum_ij (|dG_ij| |dM_p[i, j]| + |G_ij| |d dM_p[i, j]|),   |dG| <= |d alpha| |alpha|^T + |alpha| |d alpha|^T + |K| |dM| |K|
      grad_{d+1} = 1/2 sn2 tr G needs only the diagonal of dG.
The global kernel (n > 96) doubles the logarithm of the folded roots: 2 n u more on logdet (_multi_target_worker).
Nothing here is fitted to what the kernels return; tests/test_ard_cpu.py confirms that a float32 numpy evaluation of the formulas stays
inside the fp32 bounds at every (n, d, kind) the GPU tests use, and that the bounds reject five kinds of wrong result.
"""
import functools
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _multi_target_worker as MT  # noqa: E402
import _whiten_worker as W  # noqa: E402

U = MT.U
LOG2PI = MT.LOG2PI
batch_of = MT.batch_of  # 13 up to n = 64, 5 beyond, 2 at n = 1024
SE, MATERN52 = 0, 1
KINDS = (SE, MATERN52)
COND_CAP = 64.0
TILE_SIZES = [1, 2, 15, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 95, 96]  # both ends of every tile form, full and ragged
GLOBAL_SIZES = [97, 130]
DIMS = (1, 2, 3, 16)
DIM_1024 = 3  # n = 1024 runs once per dtype
OUTPUTS = ("logml", "grad", "alpha")
E_EXP = 4.0  # the error of the device exponential in units of u: below 2 ulp
TINY = {np.dtype(np.float64): np.finfo(np.float64).tiny, np.dtype(np.float32): float(np.finfo(np.float32).tiny)}


def inputs(n, d, batch, dt, seed=None, shared=False):
    """(X (batch or 1, n, d), y (batch or 1, n), theta (batch, d + 2)) in dtype dt by the recipe of the module docstring"""
    rng = np.random.default_rng(12000 + 97 * n + 7 * d if seed is None else seed)
    nb = 1 if shared else batch
    X = rng.uniform(0.0, n ** (1.0 / d), (nb, n, d))
    y = rng.standard_normal((nb, n))
    ell = rng.uniform(0.5, 1.0, (batch, d))
    sf2 = rng.uniform(0.5, 2.0, batch)
    sn2 = rng.uniform(0.3, 0.6, batch) * sf2
    theta = np.concatenate([np.log(sf2)[:, None], np.log(ell), np.log(sn2)[:, None]], axis=1)
    return X.astype(dt), y.astype(dt), theta.astype(dt)


def element(s, kind, f=np.float64):
    """(phi, psi, |psi'|) of the module docstring in the dtype of s"""
    if kind == SE:
        phi = np.exp(f(-0.5) * s)
        return phi, phi, f(0.5) * phi
    a = np.sqrt(f(5.0) * s)
    e = np.exp(-a)
    return (f(1.0) + a + f(5.0) / f(3.0) * s) * e, f(5.0) / f(3.0) * (f(1.0) + a) * e, f(25.0) / f(6.0) * e


def formulas(X, y, theta, n, d, kind, f):
    """the formulas of the module docstring in the dtype f on inputs of that dtype; X, y broadcast over the batch of theta"""
    th = np.asarray(theta, dtype=f).reshape(-1, d + 2)
    batch = th.shape[0]
    Xb = np.broadcast_to(np.asarray(X, dtype=f).reshape(-1, n, d), (batch, n, d))
    yb = np.broadcast_to(np.asarray(y, dtype=f).reshape(-1, n), (batch, n))
    sf2, ell, sn2 = np.exp(th[:, 0]), np.exp(th[:, 1:d + 1]), np.exp(th[:, d + 1])
    z = Xb / ell[:, None, :]
    D = z[:, :, None, :] - z[:, None, :, :]  # (batch, n, n, d)
    s = np.zeros((batch, n, n), dtype=f)
    for k in range(d):
        s = s + D[..., k] * D[..., k]
    phi, psi, dpsi = element(s, kind, f)
    eye = np.eye(n, dtype=f)
    M = sf2[:, None, None] * phi + sn2[:, None, None] * eye
    return dict(y=yb, sf2=sf2, ell=ell, sn2=sn2, z=z, D=D, s=s, phi=phi, psi=psi, dpsi=dpsi, M=M)


def derivative_matrices(r, n, d):
    """(batch, d + 2, n, n): dM_0, dM_1 .. dM_d, dM_{d+1}"""
    f = r["M"].dtype.type
    sf = r["sf2"][:, None, None]
    dM = [sf * r["phi"]] + [sf * r["psi"] * r["D"][..., k] ** 2 for k in range(d)] + \
         [r["sn2"][:, None, None] * np.eye(n, dtype=f)]
    return np.stack(dM, axis=1)


def reference(X, y, theta, n, d, kind, idx=None):
    """the outputs and every term of the bounds, float64 (logml longdouble); idx: the matrices to compute (the others may be not SPD)"""
    th = np.asarray(theta, dtype=np.float64).reshape(-1, d + 2)
    Xa = np.asarray(X, dtype=np.float64).reshape(-1, n, d)
    ya = np.asarray(y, dtype=np.float64).reshape(-1, n)
    if idx is not None:
        th = th[idx]
        Xa = Xa if Xa.shape[0] == 1 else Xa[idx]
        ya = ya if ya.shape[0] == 1 else ya[idx]
    r = formulas(Xa, ya, th, n, d, kind, np.float64)
    M = r["M"]
    sv = np.linalg.svd(M, compute_uv=False)
    K = np.linalg.inv(M)
    alpha = np.einsum("kij,kj->ki", K, r["y"])
    G = alpha[:, :, None] * alpha[:, None, :] - K
    dM = derivative_matrices(r, n, d)
    logdet = W.logdet_longdouble(M, np.linalg.cholesky(M))
    quad = np.einsum("ki,ki->k", r["y"], alpha)
    r.update(K=K, alpha=alpha, G=G, dM=dM, cond=sv[:, 0] / sv[:, -1], knorm=1.0 / sv[:, -1], logdet=logdet, quad=quad,
             quadmag=np.einsum("ki,kij,kj->k", np.abs(r["y"]), np.abs(K), np.abs(r["y"])),
             logml=-(quad + logdet + n * np.log(2 * np.longdouble(np.pi))) / 2, grad=0.5 * np.einsum("kij,kpij->kp", G, dM))
    return r


def generation_error(r, n, d, kind, u, dt):
    """(|dM| (batch, n, n), |d dM_p| (batch, d + 2, n, n)) of part (2) of the module docstring"""
    z, D, s = r["z"], r["D"], r["s"]
    E = E_EXP * u
    zsum = np.abs(z)[:, :, None, :] + np.abs(z)[:, None, :, :]
    dD = u * zsum + (E + u) * np.abs(D)
    ds = (2 * np.abs(D) * dD).sum(axis=3) + d * u * s
    sf = r["sf2"][:, None, None]
    if kind == SE:
        dphi = r["phi"] * (0.5 * ds + E)
        dpsi = dphi
    else:
        a = np.sqrt(5.0 * s)
        dphi = 0.5 * r["psi"] * ds + r["phi"] * u * (10 + 4 * a)
        dpsi = r["dpsi"] * ds + r["psi"] * u * (10 + 4 * a)
    off = sf * dphi + (E + u) * sf * r["phi"] + sf * TINY[np.dtype(dt)]
    eye = np.eye(n)[None]
    dMerr = off * (1 - eye) + (E + 2 * u) * r["M"] * eye
    d0 = off * (1 - eye) + (E + u) * sf * eye
    dk = [sf * dpsi * D[..., k] ** 2 + sf * r["psi"] * (2 * np.abs(D[..., k]) * dD[..., k] + u * D[..., k] ** 2) +
          (E + 2 * u) * np.abs(r["dM"][:, 1 + k]) for k in range(d)]
    dn = E * r["sn2"][:, None, None] * eye
    return dMerr, np.stack([d0] + dk + [np.broadcast_to(dn, d0.shape)], axis=1)


def bounds(r, n, d, kind, u, dt):
    """dict of the bounds of the module docstring: logml[k], grad[k, p], alpha[k, i]"""
    eps = (n + 4) * u * r["cond"] ** 2
    K, G, dM, alpha = r["K"], r["G"], r["dM"], r["alpha"]
    aK, aa = np.abs(K), np.abs(alpha)
    an = np.linalg.norm(alpha, axis=1)
    kf = np.linalg.norm(K, "fro", axis=(1, 2))
    ld = r["logdet"].astype(np.float64)
    # (1) on a given M
    b_logdet = n * n * u * r["cond"] + n * u * np.maximum(1.0, np.abs(ld)) + (2 * n * u if n > 96 else 0.0)
    b_quad = eps * r["knorm"] * np.linalg.norm(r["y"], axis=1) ** 2 + 2 * n * u * r["quadmag"] + u * np.abs(r["quad"])
    sq = r["quad"] + ld
    b_logml = (b_quad + b_logdet) / 2 + u * (np.abs(sq) + 2 * n * LOG2PI + np.abs(sq + n * LOG2PI)) / 2
    b_alpha = np.broadcast_to((eps * an)[:, None], alpha.shape).copy()
    dmf = np.linalg.norm(dM, "fro", axis=(2, 3))
    b_grad = (eps * (an ** 2 + kf))[:, None] * dmf + (n * n + 2) * u * np.abs(G[:, None] * dM).sum(axis=(2, 3))
    # (2) the generation error, propagated
    dMerr, ddM = generation_error(r, n, d, kind, u, dt)
    dMa = np.einsum("kij,kj->ki", dMerr, aa)
    dalpha = np.einsum("kij,kj->ki", aK, dMa)
    b_alpha += dalpha
    b_logml += 0.5 * (np.einsum("ki,ki->k", aa, dMa) + (aK * dMerr).sum(axis=(1, 2)))
    dG = dalpha[:, :, None] * aa[:, None, :] + aa[:, :, None] * dalpha[:, None, :] + aK @ dMerr @ aK
    b_grad += 0.5 * ((dG[:, None] * np.abs(dM)).sum(axis=(2, 3)) + (np.abs(G)[:, None] * ddM).sum(axis=(2, 3)))
    return dict(logml=b_logml, grad=b_grad, alpha=b_alpha)


def shapes(n, d):
    return dict(logml=(-1,), grad=(-1, d + 2), alpha=(-1, n))


def ratios(out, r, n, d, kind, u, dt, idx=None):
    """err / bound of every output in the dict `out` (packed, as the kernels pack them) for the matrices idx"""
    b = bounds(r, n, d, kind, u, dt)
    shp = shapes(n, d)
    rs = {}
    for name in OUTPUTS:
        if out.get(name) is None:
            continue
        got = np.asarray(out[name]).reshape(shp[name])
        got = got if idx is None else got[idx]
        assert np.isfinite(got).all(), name
        err = np.abs(got.astype(np.longdouble) - r[name]).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            rs[name] = np.where(err == 0, 0.0, err / b[name])
    return rs


def check(out, r, n, d, kind, dt, idx=None, what="", factor=1.0):
    """every given output within factor * bound; prints err / bound first. Returns {name: worst err / bound}"""
    rs = ratios(out, r, n, d, kind, U[np.dtype(dt)], dt, idx)
    worst = {k: float(v.max()) for k, v in rs.items()}
    print(f"  {what} n={n} d={d} kind={kind} {np.dtype(dt).name} cond={r['cond'].max():.2f} err/bound: " +
          " ".join(f"{k}={v:.4f}" for k, v in worst.items()))
    for k, v in rs.items():
        assert np.isfinite(v).all() and (v <= factor).all(), (what, n, d, kind, k, float(np.nanmax(v)))
    return worst


@functools.lru_cache(maxsize=6)
def case(n, d, dtname, kind):
    """the shared case: (X, y, theta, reference) with per-matrix points. Nobody writes into it; the last few are kept (a reference holds
    every dM_p)"""
    dt = np.dtype(dtname).type
    X, y, theta = inputs(n, d, batch_of(n), dt)
    for x in (X, y, theta):
        x.setflags(write=False)
    return X, y, theta, reference(X, y, theta, n, d, kind)


def gpu_cases():
    """every (n, d) the accuracy tests of tests/test_gpu_ard.py run, for both dtypes and both kinds"""
    return [(n, d) for n in TILE_SIZES + GLOBAL_SIZES for d in DIMS] + [(1024, DIM_1024)]


def float32_evaluation(X, y, theta, n, d, kind):
    """the formulas evaluated in float32 numpy on the float32 inputs: what any fp32 implementation of them may expect"""
    f = np.float32
    r = formulas(X, y, theta, n, d, kind, f)
    K = np.linalg.inv(r["M"])
    alpha = np.einsum("kij,kj->ki", K, r["y"])
    G = alpha[:, :, None] * alpha[:, None, :] - K
    logdet = np.linalg.slogdet(r["M"])[1].astype(f)
    logml = f(-0.5) * (np.einsum("ki,ki->k", r["y"], alpha) + logdet + f(n) * f(LOG2PI))
    grad = f(0.5) * np.einsum("kij,kpij->kp", G, derivative_matrices(r, n, d))
    out = dict(logml=logml, grad=grad.reshape(-1), alpha=alpha.reshape(-1))
    assert all(v.dtype == f for v in out.values())
    return out


# ---- GPU helpers (torch and the package are imported by the caller) ---------------------------------------------------------------------
def run(api, torch, n, X, y, theta, kind, want=OUTPUTS, d=None):
    """api.ard_logml_batched on numpy inputs: (dict of the numpy outputs in `want`, info). Asserts that no input changed"""
    d = X.shape[-1] if d is None else d
    batch = theta.size // (d + 2)
    host = [np.ascontiguousarray(x) for x in (X, y, theta)]
    dev = [torch.tensor(x).cuda() for x in host]
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    res = api.ard_logml_batched(n, *dev, kind=kind, ndim=d, batchSize=batch, info=info, want=want)
    torch.cuda.synchronize()
    for h, dv in zip(host, dev):
        assert np.array_equal(dv.cpu().numpy(), h, equal_nan=True), "an input was modified"
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in zip(OUTPUTS, res)}
    assert all((out[k] is not None) == (k in want) for k in OUTPUTS)
    return {k: v for k, v in out.items() if v is not None}, info.cpu().numpy()


same_bits = MT.same_bits


def nan_points(X, n, where):
    """a copy of X (batch, n, d) with a NaN coordinate in point j of matrix k for every (k -> j) of `where`; {k: j + 1}: the info expected"""
    out = np.array(X)
    for k, j in where.items():
        out[k, j, -1] = np.nan
    return out, {k: j + 1 for k, j in where.items()}


def check_with_rejects(out, info, X, y, theta, n, d, kind, dt, want_info, what="", sample=None):
    """info as expected, every output NaN exactly at the rejected matrices, finite everywhere else and within the bounds there (sample:
    at that many of them, evenly spread and with both neighbours of every reject, where the reference of thousands would not fit)"""
    batch = info.size
    bad = sorted(want_info)
    ok = np.array([k for k in range(batch) if k not in want_info])
    expect = np.zeros(batch, dtype=np.int64)
    for k, v in want_info.items():
        expect[k] = v
    assert np.array_equal(info, expect), (what, n, info[bad], [want_info[k] for k in bad], np.flatnonzero(info != expect)[:10])
    for k, v in out.items():
        o = v.reshape(batch, -1)
        assert np.isnan(o[bad]).all() and np.isfinite(o[ok]).all(), (what, n, k)
    if sample is not None and ok.size > sample:
        near = [k + e for k in bad for e in (-1, 1) if 0 <= k + e < batch and k + e not in want_info]
        ok = np.unique(np.concatenate([ok[::max(1, ok.size // sample)], np.array(near, dtype=ok.dtype), ok[-1:]]))
    return check(out, reference(X, y, theta, n, d, kind, idx=ok), n, d, kind, dt, idx=ok, what=what)


# the calls of test_grid_stride_and_chunking: (n, d, batch, dtype, kind, shared X, rejects {matrix: point}). 4000 matrices on a grid of
# 256 * 12 = 3072 workgroups run the stride loop twice; the rejects sit beyond the first round. 20 working copies of
# (130 * 130 + 130 * 2) * 8 = 137 280 bytes under a cap of 1 MiB: seven to a chunk, three chunks, two of them with a non-zero `first`.
STRIDE_CASES = ((33, 2, 4000, np.float64, SE, False, {3073: 0, 3500: 17, 3999: 32}),
                (33, 3, 4000, np.float32, MATERN52, True, {}),
                (17, 1, 4000, np.float32, SE, False, {3100: 16, 3600: 5, 3998: 0}),
                (130, 2, 20, np.float64, MATERN52, False, {7: 0, 13: 64, 19: 129}))


def stride_inputs(n, d, batch, dt, kind, shared, rejects):
    X, y, theta = inputs(n, d, batch, dt, seed=15000 + n + d, shared=shared)
    want_info = {}
    if rejects:
        X, want_info = nan_points(X, n, rejects)
    return X, y, theta, want_info


def stride_key(i, k):
    return f"case{i}_{k}"


def main():
    import torch
    api = importlib.import_module("cuda-matrix-inversion_amd.api")
    assert os.environ.get("MATINV_TILE_GRID_MULT") == "1" and os.environ.get("MATINV_BLOCKED_WS_MB") == "1"
    saved = np.load(sys.argv[1])
    for i, (n, d, batch, dt, kind, shared, rejects) in enumerate(STRIDE_CASES):
        X, y, theta, _ = stride_inputs(n, d, batch, dt, kind, shared, rejects)
        out, info = run(api, torch, n, X, y, theta, kind, d=d)
        assert np.array_equal(info, saved[stride_key(i, "info")]), (i, "info")
        same_bits(out, {k: saved[stride_key(i, k)] for k in out}, (i, "default call"))
        print(f"  {api.ard_logml_kernel_name(dt, kind, n)} batch={batch} d={d}: the bits of the default call")
    print("ard-worker ok")


if __name__ == "__main__":
    main()
