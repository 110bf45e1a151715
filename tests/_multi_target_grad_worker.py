"""Reference, inputs, bounds and checks of the multi-output gradient tests (tests/test_gpu_multi_target_grad.py and
tests/test_multi_target_grad_cpu.py import them), and the worker of test_grid_stride_and_chunking: ONE process under
MATINV_TILE_GRID_MULT=1 and MATINV_BLOCKED_WS_MB=1 (the library reads each switch once per process), so that the tile kernels' stride loop
runs several rounds on the same per-workgroup workspace and the global launcher takes several chunks. The worker is given a file of the
outputs of the same calls made under the default switches, which the test has checked against the reference before: it asserts equal
bits, exits non-zero at the first failure and starts nothing after it; prints `multi-target-grad-worker ok` at the end.

Reference: float64 numpy on the float64 image of exactly what the kernel reads (_logml_grad_worker.image and sym_lower: the lower
triangles of B and of every dM_p mirrored, the diagonal B_ii + c_i rounded in the working precision). With K = inv(M), alpha_t = K y_t for
the D targets of a matrix and G = sum_t alpha_t alpha_t^T - D K:
    grad_p = 1/2 sum_ij G_ij dM_p[i, j]      gradc_i = 1/2 G_ii      logml_t, alpha_t: _multi_target_worker.reference (logdet as there)
grad and gradc are the derivatives of sum_t logml_t: d logml_t = 1/2 (alpha_t^T dM alpha_t - tr(K dM)), summed over t
(tests/test_multi_target_grad_cpu.py checks it against central finite differences).

Inputs: B, c, Ys of _multi_target_worker.case; dM of _logml_grad_worker.derivs.

Bounds, first order and not fitted: u = 2^-53 (fp64) or 2^-24 (fp32), eps = (n + 4) * u * cond2(M)^2, S = sum_t ||alpha_t||_2^2.
    alpha, logml   those of _multi_target_worker.bounds
    gradc   |gradc^_i - gradc_i| <= eps * (S + D ||K||_2) + (D + 2) * u * 1/2 (sum_t alpha_ti^2 + D K_ii)
    grad    |grad^_p - grad_p|   <= eps * (S + D ||K||_F) * ||dM_p||_F + (n^2 + D) * u * sum_ij (sum_t |alpha_ti alpha_tj| + D |K_ij|) |dM_p[i, j]|
The first terms are those of _logml_grad_worker summed over the targets: d(alpha_t alpha_t^T) <= 2 eps ||alpha_t||^2 in the Frobenius
norm, which the factor 1/2 of the outputs halves, and d(D K) <= D eps ||K||; Cauchy-Schwarz against dM_p for grad. The second terms are
the rounding of what is summed: G_ij is a sum of D products and one scaled element, D + 2 roundings on the magnitudes
sum_t |alpha_ti alpha_tj| + D |K_ij| (K_ii > 0 and alpha_ti^2 >= 0 on the diagonal, and the factor 1/2 is exact); grad adds the n^2
products with dM_p and their sum in any order (the classical bound of a recursive sum, loose for the trees the kernels use). Nothing
here is fitted to what the kernels return; tests/test_multi_target_grad_cpu.py confirms that a float32 numpy evaluation of the same
formulas stays inside the fp32 bounds at every size and (D, P) the GPU tests use.
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
import _logml_grad_worker as G  # noqa: E402
import _multi_target_worker as MT  # noqa: E402

U = MT.U
break_three = MT.break_three
first = MT.first
derivs, sym_lower, image = G.derivs, G.sym_lower, G.image
TILE_SIZES, GLOBAL_SIZES, batch_of = MT.TILE_SIZES, MT.GLOBAL_SIZES, MT.batch_of
DP = ((1, 1), (16, 2), (17, 1), (33, 3))  # a partial group, an exact group, a group plus one, two groups plus one
DP_1024 = (3, 1)                          # n = 1024 runs once per dtype
DMAX, PMAX = MT.DMAX, 3
OUTPUTS = ("grad", "gradc", "logml", "alpha")


def first_derivs(dMs, n, total, sel):
    """the derivative matrices `sel` (a count, a slice or a list) of the `total` matrices of every covariance matrix, packed"""
    sel = slice(0, sel) if isinstance(sel, int) else sel
    return np.ascontiguousarray(np.asarray(dMs).reshape(-1, total, n * n)[:, sel]).reshape(-1)


def reference(mt, dMs, n, P, idx=None):
    """mt: the _multi_target_worker reference of the D targets (MT.reference / MT.take); adds G, grad, gradc and the terms of the bounds.
    dMs None: without grad. idx: the matrices mt holds, when dMs holds more"""
    ref = dict(mt)
    a, K = mt["alpha"], mt["K"]
    D = a.shape[1]
    Gm = np.einsum("kti,ktj->kij", a, a) - D * K
    ref.update(G=Gm, gradc=0.5 * np.einsum("kii->ki", Gm), S=(a ** 2).sum(axis=(1, 2)),
               gmag=np.einsum("kti,ktj->kij", np.abs(a), np.abs(a)) + D * np.abs(K))
    if dMs is not None and P:
        dM = sym_lower(dMs, n).reshape(-1, P, n, n)
        if idx is not None:
            dM = dM[idx]
        ref.update(dM=dM, grad=0.5 * np.einsum("kij,kpij->kp", Gm, dM))
    return ref


def sum_logml(M, y):
    """sum_t logml_t of ONE matrix in float64: what grad and gradc differentiate"""
    n = M.shape[0]
    quad = np.einsum("ti,ti->", y, np.linalg.solve(M, y.T).T)
    return -0.5 * (quad + y.shape[0] * (np.linalg.slogdet(M)[1] + n * np.log(2 * np.pi)))


@functools.lru_cache(maxsize=None)
def case(n, dtname, with_c):
    """the shared case of size n: (B, c, Ys, dMs, reference) with DMAX targets and PMAX derivative matrices per matrix; B, c, Ys and the
    multi-target reference are those of _multi_target_worker.case. Computed once; nobody writes into it"""
    B, c, Ys, _, full = MT.case(n, dtname, with_c)
    dMs = derivs(n, batch_of(n), PMAX, np.dtype(dtname).type)
    dMs.setflags(write=False)
    return B, c, Ys, dMs, full


def take(full, dMs, n, D, P):
    """the reference of the first D targets and the first P derivative matrices of the shared case"""
    return reference(MT.take(full, D, 0), first_derivs(dMs, n, PMAX, P) if P else None, n, P)


def bounds(ref, n, u):
    """dict of the bounds of the module docstring: grad[k, p], gradc[k, i], logml[k, t], alpha[k, t, 1]"""
    out = {k: v for k, v in MT.bounds(ref, n, u).items() if k in ("logml", "alpha")}
    eps = (n + 4) * u * ref["cond"] ** 2
    D = ref["alpha"].shape[1]
    out["gradc"] = (eps * (ref["S"] + D * ref["knorm"]))[:, None] + (D + 2) * u * 0.5 * np.einsum("kii->ki", ref["gmag"])
    if "dM" in ref:
        kf = np.linalg.norm(ref["K"], "fro", axis=(1, 2))
        dmf = np.linalg.norm(ref["dM"], "fro", axis=(2, 3))
        mag = (ref["gmag"][:, None] * np.abs(ref["dM"])).sum(axis=(2, 3))
        out["grad"] = (eps * (ref["S"] + D * kf))[:, None] * dmf + (n * n + D) * u * mag
    return out


def shapes(ref, n):
    D = ref["alpha"].shape[1]
    P = ref["dM"].shape[1] if "dM" in ref else 0
    return dict(grad=(-1, P), gradc=(-1, n), logml=(-1, D), alpha=(-1, D, n))


def ratios(out, ref, n, u, idx=None):
    """err / bound of every output in the dict `out` (packed, as the kernels pack them) for the matrices idx"""
    b = bounds(ref, n, u)
    shp = shapes(ref, n)
    pick = (lambda a: a) if idx is None else (lambda a: a[idx])
    rs = {}
    for name in OUTPUTS:
        if out.get(name) is None:
            continue
        got = pick(np.asarray(out[name]).reshape(shp[name]))
        err = np.abs(got.astype(np.longdouble) - ref[name]).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            rs[name] = np.where(err == 0, 0.0, err / b[name])
        assert np.isfinite(got).all(), name
    return rs


def check(out, ref, n, u, idx=None, what="", factor=1.0):
    """every given output within factor * bound; prints err / bound first. Returns {name: worst err / bound}"""
    rs = ratios(out, ref, n, u, idx)
    shp = shapes(ref, n)
    worst = {k: float(v.max()) for k, v in rs.items()}
    print(f"  {what} n={n} D={shp['logml'][1]} P={shp['grad'][1]} cond={ref['cond'].max():.2f} err/bound: " +
          " ".join(f"{k}={v:.4f}" for k, v in worst.items()))
    for k, v in rs.items():
        assert np.isfinite(v).all() and (v <= factor).all(), (what, n, k, float(np.nanmax(v)))
    return worst


def float32_evaluation(B, c, Ys, dMs, n, D, P):
    """the reference formulas evaluated in float32 numpy on the float32 inputs: what any fp32 implementation of them may expect"""
    f = np.float32
    mt = MT.float32_evaluation(B, c, Ys, None, n, D, 0)
    M = np.tril(MT.as_mats(B, n).astype(f))
    M = M + np.tril(M, -1).transpose(0, 2, 1)
    if c is not None:
        idx = np.arange(n)
        M[:, idx, idx] = M[:, idx, idx] + np.asarray(c, dtype=f).reshape(-1, n)
    K = np.linalg.inv(M)
    a = mt["alpha"].reshape(-1, D, n)
    Gm = np.einsum("kti,ktj->kij", a, a) - f(D) * K
    out = dict(gradc=(f(0.5) * np.einsum("kii->ki", Gm)).reshape(-1), logml=mt["logml"], alpha=mt["alpha"])
    if P:
        dm = np.tril(MT.as_mats(dMs, n).astype(f))
        dM = (dm + np.tril(dm, -1).transpose(0, 2, 1)).reshape(-1, P, n, n)
        out["grad"] = (f(0.5) * np.einsum("kij,kpij->kp", Gm, dM)).reshape(-1)
    assert all(v.dtype == f for v in out.values())
    return out


# ---- GPU helpers (torch and the package are imported by the caller) ---------------------------------------------------------------------
def run(api, torch, n, B, c, Ys, dMs, want=OUTPUTS, D=None, P=None):
    """api.multi_target_grad_batched on packed numpy inputs: (dict of the numpy outputs in `want`, info). Asserts that no input changed"""
    batch = B.size // (n * n)
    host = [None if x is None else np.ascontiguousarray(x) for x in (B, c, Ys, dMs)]
    dev = [None if x is None else torch.tensor(x).cuda() for x in host]
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    res = api.multi_target_grad_batched(n, *dev, batchSize=batch, info=info, want=want, ntarget=D, nparam=P)
    torch.cuda.synchronize()
    for h, d in zip(host, dev):
        assert h is None or np.array_equal(d.cpu().numpy(), h, equal_nan=True), "an input was modified"
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in zip(OUTPUTS, res)}
    assert all((out[k] is not None) == (k in want) for k in OUTPUTS)
    return {k: v for k, v in out.items() if v is not None}, info.cpu().numpy()


same_bits = MT.same_bits


def check_with_rejects(out, info, B, c, Ys, dMs, n, D, P, dt, want_info, what=""):
    """info as expected, every output NaN exactly at the not-SPD matrices, finite and within the bounds elsewhere"""
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
    ref = reference(MT.reference(MT.model(B, c, n, idx=ok), Ys, None, n, D, 0, idx=ok), dMs, n, P, idx=ok)
    return check(out, ref, n, U[np.dtype(dt)], idx=ok, what=what)


# the calls of test_grid_stride_and_chunking: (n, batch, D, P, dtype, with c, rejects). 4000 matrices on a grid of 256 * 12 = 3072
# workgroups run the stride loop twice (under the 1 MiB cap the workspace of D n elements per workgroup holds the grid to fewer
# workgroups still, so every slice is reused many times); the rejects sit beyond the first round. 20 working copies of
# 130 * (130 + 33) * 8 = 169 520 bytes under a cap of 1 MiB: six to a chunk, four chunks, three of them with a non-zero `first`.
STRIDE_CASES = ((33, 4000, 33, 2, np.float64, True, (3073, 3500, 3999)),
                (33, 4000, 33, 1, np.float32, False, (3100, 3600, 3998)),
                (130, 20, 33, 2, np.float64, True, (7, 13, 19)))


def stride_inputs(n, batch, D, P, dt, with_c, rejects_at):
    B, c, _ = MT.L.inputs(n, batch, dt, with_c)
    Ys = MT.targets(n, batch, D, dt, seed=7700 + n)
    dMs = derivs(n, batch, P, dt)
    want_info = break_three(B, c, n, rejects_at)
    return B, c, Ys, dMs, want_info


def stride_key(i, k):
    return f"case{i}_{k}"


def main():
    import torch
    api = importlib.import_module("cuda-matrix-inversion_amd.api")
    assert os.environ.get("MATINV_TILE_GRID_MULT") == "1" and os.environ.get("MATINV_BLOCKED_WS_MB") == "1"
    saved = np.load(sys.argv[1])
    for i, (n, batch, D, P, dt, with_c, rejects_at) in enumerate(STRIDE_CASES):
        B, c, Ys, dMs, want_info = stride_inputs(n, batch, D, P, dt, with_c, rejects_at)
        # without alpha the groups come back from the per-workgroup workspace, with it from dAlpha
        out, info = run(api, torch, n, B, c, Ys, dMs, want=("grad", "gradc", "logml"))
        assert np.array_equal(info, saved[stride_key(i, "info")]), (i, "info")
        same_bits(out, {k: saved[stride_key(i, k)] for k in out}, (i, "workspace"))
        out, _ = run(api, torch, n, B, c, Ys, dMs)
        same_bits(out, {k: saved[stride_key(i, k)] for k in out}, (i, "alpha"))
        print(f"  {api.multi_target_grad_kernel_name(dt, n)} batch={batch} D={D} P={P}: the bits of the default call")
    print("multi-target-grad-worker ok")


if __name__ == "__main__":
    main()
