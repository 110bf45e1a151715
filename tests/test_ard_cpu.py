"""CPU-side checks of the GP log marginal likelihood from coordinates (matinv_ard_logml_batched*): exports and prototypes, argument
refusals, dispatch names against the compiled stubs (the forms carry the names of the SPD inversion kernels with thirteen more template
arguments), the meaning of the reference (its gradient against central finite differences of its logml), and the checks that the bounds of
tests/_ard_worker.py hold for a float32 numpy evaluation of the formulas and fail wrong results. No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import _ard_worker as A
import test_instantiations_cpu as audit
from conftest import pkg

NAMES = ["matinv_ard_logml_batched", "matinv_ard_logml_kernel_name", "matinv_ard_logml_batched_host"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = ", true" * 13 + ">"
DTYPES = (np.float64, np.float32)


def test_ard_symbols_exported_with_their_prototypes():
    lib = pkg("_lib")
    L = lib.lib()
    header = open(os.path.join(ROOT, "include", "matinv.h")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in lib.NATIVE_NAMES
        assert re.search(rf"\b{name}\(", header), name
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    assert L.matinv_ard_logml_batched.argtypes == [ci] * 4 + [vp, sz, vp, sz] + [vp] * 4 + [sz, vp, vp]
    assert L.matinv_ard_logml_batched_host.argtypes == [ci] * 4 + [vp, sz, vp, sz] + [vp] * 4 + [sz, vp]
    assert L.matinv_ard_logml_batched.restype is ci and L.matinv_ard_logml_batched_host.restype is ci
    assert L.matinv_ard_logml_kernel_name.argtypes == [ci, ci, ci] and L.matinv_ard_logml_kernel_name.restype is ctypes.c_char_p
    m = re.search(r"int matinv_ard_logml_batched\(([^;]*)\);", header)
    assert m and [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == \
        ["dtype", "kind", "n", "ndim", "dXs", "xstride", "dYs", "ystride", "dThetas", "dLogML", "dGrad", "dAlpha", "batch", "dInfo", "stream"]
    m = re.search(r"int matinv_ard_logml_batched_host\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == 14
    assert re.search(r"MATINV_COV_SE = 0", header) and re.search(r"MATINV_COV_MATERN52 = 1", header)
    api = pkg("api")
    for name in ("ard_logml_batched", "ard_logml_batched_host", "ard_logml_kernel_name"):
        assert callable(getattr(api, name))
    assert (api.COV_SE, api.COV_MATERN52) == (0, 1) == (A.SE, A.MATERN52)
    assert L.matinv_abi_version() == 2


def test_ard_kernel_names_are_compiled_stubs():
    """both directions: every name is exactly a stub, every stub of the new forms is named, and no earlier form is claimed"""
    api = pkg("api")
    seen = set()
    for dt in DTYPES:
        for kind in A.KINDS:
            for n in range(1, 1025):
                name = api.ard_logml_kernel_name(dt, kind, n)
                assert name.endswith(TAIL) and name.startswith("matinv_spd_tile_f" if n <= 96 else "matinv_chol_global<"), (n, name)
                seen.add(name)
    assert seen <= audit.STUBS, sorted(seen - audit.STUBS)  # exactly a stub, not a prefix of one

    def nargs(s):
        return len(s[s.index("<") + 1:-1].split(", "))

    forms = {s for s in audit.STUBS if (s.startswith("matinv_chol_global<") and nargs(s) == 14) or
             (s.startswith("matinv_spd_tile_f") and nargs(s) == 15)}
    assert len(forms) == 26 and forms == seen, sorted(forms ^ seen)
    # nothing compiled carries more arguments than the new forms, and the names of the family before them are not theirs
    assert not [s for s in audit.STUBS if s.startswith(("matinv_chol_global<", "matinv_spd_tile_f")) and
                nargs(s) > (14 if s.startswith("matinv_chol") else 15)]
    for dt in DTYPES:
        for n in (2, 96, 97, 1024):
            assert api.trend_loo_kernel_name(dt, n) not in seen and api.trend_loo_kernel_name(dt, n) in audit.STUBS
        for n in (-1, 0, 1025, 4096):
            assert api.ard_logml_kernel_name(dt, A.SE, n) == ""
        assert api.ard_logml_kernel_name(dt, 2, 32) == "" == api.ard_logml_kernel_name(dt, -1, 32)
    L = pkg("_lib").lib()
    assert L.matinv_ard_logml_kernel_name(2, 0, 32) == b"" == L.matinv_ard_logml_kernel_name(-1, 0, 32)


def test_ard_argument_refusals_without_device():
    lib = pkg("_lib")
    L = lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    AUTO = object()

    def args(dtype=0, kind=0, n=4, d=2, x=p, xs=AUTO, y=p, ys=AUTO, th=p, lm=p, gr=p, al=p, batch=2):
        return (dtype, kind, n, d, x, n * d if xs is AUTO else xs, y, n if ys is AUTO else ys, th, lm, gr, al, batch, None)

    def dev(**kw):
        return L.matinv_ard_logml_batched(*args(**kw), None)

    def host(**kw):
        return L.matinv_ard_logml_batched_host(*args(**kw))

    def refused(rc, code, text):
        assert rc == code, (rc, code, text, L.matinv_last_error())
        assert text in L.matinv_last_error(), (text, L.matinv_last_error())

    none = dict(lm=None, gr=None, al=None)
    nothing = dict(x=None, y=None, th=None, **none)
    for f in (dev, host):
        refused(f(n=0), lib.ERR_ARG, b"n must be")
        refused(f(dtype=2), lib.ERR_ARG, b"unknown dtype")
        for kind in (-1, 2):
            refused(f(kind=kind), lib.ERR_ARG, b"unknown covariance function")
            refused(f(kind=kind, batch=0, **nothing), lib.ERR_ARG, b"unknown covariance function")
        for d in (0, -3):
            refused(f(d=d), lib.ERR_ARG, b"ndim must be >= 1")
            refused(f(d=d, batch=0, **nothing), lib.ERR_ARG, b"ndim must be >= 1")
        refused(f(d=17), lib.ERR_UNSUPPORTED, b"ndim=17")
        refused(f(d=17, x=None), lib.ERR_ARG, b"null device pointer")  # the count limit comes after the pointer checks
        refused(f(xs=7), lib.ERR_ARG, b"xstride must be")
        refused(f(xs=4), lib.ERR_ARG, b"xstride must be")
        refused(f(ys=5), lib.ERR_ARG, b"ystride must be")
        refused(f(ys=8), lib.ERR_ARG, b"ystride must be")
        refused(f(**none), lib.ERR_ARG, b"no output requested")
        for one in ("x", "y", "th"):
            refused(f(**{one: None}), lib.ERR_ARG, b"null device pointer")
        refused(f(batch=0x80000000), lib.ERR_ARG, b"batch")
        refused(f(n=1025, batch=1), lib.ERR_UNSUPPORTED, b"n=1025")
        assert f(n=1025, batch=1, x=None) == lib.ERR_ARG
        assert f(batch=0, **nothing) == lib.OK
        assert f(batch=0, xs=3, ys=1, **nothing) == lib.OK  # a no-op after the dtype, n, kind and ndim checks
        assert f(batch=0, dtype=5, **nothing) == lib.ERR_ARG
        assert f(batch=0, n=0, **nothing) == lib.ERR_ARG


def test_api_argument_validation():
    api = pkg("api")
    n, d = 4, 2
    X, y, th = np.zeros((2, n, d)), np.zeros((2, n)), np.zeros((2, d + 2))
    with pytest.raises(ValueError, match="want must name"):
        api.ard_logml_batched_host(n, X, y, th, want=("logml", "quad"))
    with pytest.raises(ValueError, match="want must name"):
        api.ard_logml_batched_host(n, X, y, th, want=())
    with pytest.raises(ValueError, match="ndim is needed"):
        api.ard_logml_batched_host(n, X.reshape(-1), y, th)
    with pytest.raises(ValueError, match="theta needs"):
        api._ard_plan(n, X, y, th, d, 3, lambda a: a.size)
    with pytest.raises(ValueError, match="X needs"):
        api.ard_logml_batched_host(n, X[:1, :3], y, th, ndim=d)
    with pytest.raises(TypeError, match="one dtype"):
        api.ard_logml_batched_host(n, X, y.astype(np.float32), th)
    # a shared point set or target vector is recognised by its size
    assert api._ard_plan(n, X[0], y, th, None, None, lambda a: a.size) == (d, 2, 0, n)
    assert api._ard_plan(n, X, y[0], th, None, None, lambda a: a.size) == (d, 2, n * d, 0)
    assert api._ard_plan(n, X[0], y[0], th[:1], None, None, lambda a: a.size) == (d, 1, n * d, n)


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("d", [1, 3])
def test_reference_gradient_matches_central_differences(kind, d):
    n, h = 9, 1e-5
    X, y, th = A.inputs(n, d, 3, np.float64, seed=5 + d)
    ref = A.reference(X, y, th, n, d, kind)
    fd = np.empty_like(ref["grad"])
    for p in range(d + 2):
        e = np.zeros(d + 2)
        e[p] = h
        fd[:, p] = ((A.reference(X, y, th + e, n, d, kind)["logml"] - A.reference(X, y, th - e, n, d, kind)["logml"]) / (2 * h)).astype(np.float64)
    scale = np.abs(ref["grad"]).max()
    assert np.abs(fd - ref["grad"]).max() <= 1e-7 * max(1.0, scale), (np.abs(fd - ref["grad"]).max(), scale)
    # psi = -2 phi' on a grid of s
    s = np.linspace(0.01, 30.0, 400)
    phi_p, _, _ = A.element(s + 1e-6, kind)
    phi_m, psi, dpsi = A.element(s - 1e-6, kind)
    assert np.allclose(-2 * (phi_p - phi_m) / 2e-6, A.element(s, kind)[1], rtol=1e-6, atol=1e-12)
    psi_p = A.element(s + 1e-6, kind)[1]
    assert np.allclose(np.abs(psi_p - psi) / 2e-6, A.element(s, kind)[2], rtol=1e-5, atol=1e-12)


@pytest.mark.parametrize("kind", A.KINDS)
def test_gpu_cases_are_well_conditioned_and_float32_numpy_stays_inside_the_bounds(kind):
    """cond2(M) <= COND_CAP for every matrix the GPU tests use (both dtypes draw the same points; the float32 image is checked), and the
    float32 numpy evaluation of the formulas lies inside the fp32 bounds at each of them"""
    worst, worst_cond = {}, 0.0
    for n, d in A.gpu_cases():
        X, y, th = A.inputs(n, d, A.batch_of(n), np.float32)
        ref = A.reference(X, y, th, n, d, kind)
        assert ref["cond"].max() <= A.COND_CAP, (n, d, kind, float(ref["cond"].max()))
        ref64 = ref if n > 130 else A.reference(*A.inputs(n, d, A.batch_of(n), np.float64), n, d, kind)
        assert ref64["cond"].max() <= A.COND_CAP, (n, d, kind, float(ref64["cond"].max()))
        worst_cond = max(worst_cond, float(ref["cond"].max()), float(ref64["cond"].max()))
        rs = A.ratios(A.float32_evaluation(X, y, th, n, d, kind), ref, n, d, kind, A.U[np.dtype(np.float32)], np.float32)
        for k, v in rs.items():
            assert (v <= 1.0).all(), (n, d, kind, k, float(v.max()))
            worst[k] = max(worst.get(k, 0.0), float(v.max()))
    print(f"kind={kind}: worst cond {worst_cond:.1f}; float32 numpy worst err/bound " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    for i, (n, d, batch, dt, knd, shared, rejects) in enumerate(A.STRIDE_CASES):
        X, y, th, _ = A.stride_inputs(n, d, 64, dt, knd, shared, {})
        assert A.reference(X, y, th, n, d, knd)["cond"].max() <= A.COND_CAP


def wrong_results(ref, n, d, kind):
    """five plausible mistakes, each as the dict of outputs it would give (float64, exact otherwise)"""
    K, G, dM, alpha = ref["K"], ref["G"], ref["dM"], ref["alpha"]
    good = dict(logml=ref["logml"].astype(np.float64), grad=ref["grad"].copy(), alpha=alpha.copy())
    out = {}
    if kind == A.MATERN52:  # psi replaced by phi
        w = dict(good, grad=good["grad"].copy())
        for k in range(d):
            w["grad"][:, 1 + k] = 0.5 * np.einsum("kij,kij->k", G, ref["sf2"][:, None, None] * ref["phi"] * ref["D"][..., k] ** 2)
        out["psi replaced by phi"] = w
    # the contribution of one off-diagonal pair dropped from one grad[1 + k]: the pair with the largest term
    w = dict(good, grad=good["grad"].copy())
    term = G * dM[:, 1]
    term[:, np.arange(n), np.arange(n)] = 0
    flat = np.abs(term).reshape(term.shape[0], -1).argmax(axis=1)
    w["grad"][:, 1] -= term.reshape(term.shape[0], -1)[np.arange(term.shape[0]), flat]  # (i, j) and (j, i): 2 * 1/2
    out["one pair dropped"] = w
    # the weight 1/2 of the diagonal tiles forgotten: every element of the 16 x 16 diagonal blocks counted twice
    blk = (np.arange(n)[:, None] // 16) == (np.arange(n)[None, :] // 16)
    w = dict(good, grad=good["grad"] + 0.5 * np.einsum("kij,kpij->kp", G * blk, dM))
    out["diagonal-tile weight forgotten"] = w
    if d >= 2:  # two dimensions' gradients swapped
        w = dict(good, grad=good["grad"].copy())
        w["grad"][:, [1, 2]] = w["grad"][:, [2, 1]]
        out["two dimensions swapped"] = w
    # sn2 left out of M
    M0 = ref["M"] - ref["sn2"][:, None, None] * np.eye(n)
    M0 = M0 + 1e-6 * np.eye(n)  # the noise-free matrix may be numerically singular: the mistake, not a breakdown, is what is tested
    K0 = np.linalg.inv(M0)
    a0 = np.einsum("kij,kj->ki", K0, ref["y"])
    G0 = a0[:, :, None] * a0[:, None, :] - K0
    out["sn2 left out of M"] = dict(logml=-(np.einsum("ki,ki->k", ref["y"], a0) + np.linalg.slogdet(M0)[1] + n * A.LOG2PI) / 2,
                                    grad=0.5 * np.einsum("kij,kpij->kp", G0, dM), alpha=a0)
    return out


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", A.KINDS)
def test_bounds_reject_wrong_results(dt, kind):
    n, d = 33, 3
    X, y, th, ref = A.case(n, d, np.dtype(dt).name, kind)
    u = A.U[np.dtype(dt)]
    good = dict(logml=ref["logml"].astype(np.float64), grad=ref["grad"], alpha=ref["alpha"])
    assert all((v <= 1.0).all() for v in A.ratios(good, ref, n, d, kind, u, dt).values())
    wrong = wrong_results(ref, n, d, kind)
    assert len(wrong) == (5 if kind == A.MATERN52 else 4)
    for what, w in wrong.items():
        rs = A.ratios(w, ref, n, d, kind, u, dt)
        worst = max(float(v.max()) for v in rs.values())
        print(f"  {what}: err/bound {worst:.3g}")
        # the batch is caught, and so is every matrix of it -- but for the swap, which no bound can see in a matrix whose two
        # gradients happen to agree to within it: there three quarters of the matrices are asked for
        per_matrix = np.maximum.reduce([v.reshape(v.shape[0], -1).max(axis=1) for v in rs.values()])
        caught = per_matrix > 1.0
        assert caught.mean() >= 0.75 if what == "two dimensions swapped" else caught.all(), (what, per_matrix)
