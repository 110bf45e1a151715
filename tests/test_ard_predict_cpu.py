"""CPU-side checks of GP prediction from coordinates (matinv_ard_predict_batched*): exports and prototypes, every argument refusal in the
order of the checks, dispatch names against the compiled stubs (the forms carry the names of the log-determinant kernels with one more
template argument), the reference against a direct evaluation, the conditioning of every matrix the GPU tests use, and the checks that the
bounds of tests/_ard_predict_worker.py hold for a float32 numpy evaluation of the formulas and fail wrong results. No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import _ard_predict_worker as AP
import _ard_worker as A
import test_instantiations_cpu as audit
from conftest import pkg

NAMES = ["matinv_ard_predict_batched", "matinv_ard_predict_kernel_name", "matinv_ard_predict_batched_host"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (np.float64, np.float32)


def test_ard_predict_symbols_exported_with_their_prototypes():
    lib = pkg("_lib")
    L = lib.lib()
    header = open(os.path.join(ROOT, "include", "matinv.h")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in lib.NATIVE_NAMES
        assert re.search(rf"\b{name}\(", header), name
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    common = [ci] * 5 + [vp, sz, vp, sz, vp, vp, sz, vp, vp, sz, vp]
    assert L.matinv_ard_predict_batched.argtypes == common + [vp]
    assert L.matinv_ard_predict_batched_host.argtypes == common
    assert L.matinv_ard_predict_batched.restype is ci and L.matinv_ard_predict_batched_host.restype is ci
    assert L.matinv_ard_predict_kernel_name.argtypes == [ci, ci, ci] and L.matinv_ard_predict_kernel_name.restype is ctypes.c_char_p
    m = re.search(r"int matinv_ard_predict_batched\(([^;]*)\);", header)
    assert m and [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == \
        ["dtype", "kind", "n", "ndim", "nquery", "dXs", "xstride", "dYs", "ystride", "dThetas", "dXqs", "xqstride", "dMean", "dVar", "batch",
         "dInfo", "stream"]
    m = re.search(r"int matinv_ard_predict_batched_host\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == 16
    assert "var + exp(theta[ndim + 1])" in header  # the variance of a noisy observation is the caller's sum
    api = pkg("api")
    for name in ("ard_predict_batched", "ard_predict_batched_host", "ard_predict_kernel_name"):
        assert callable(getattr(api, name))
    assert L.matinv_abi_version() == 2


def test_ard_predict_kernel_names_are_compiled_stubs():
    """both directions: every name is exactly a stub, every stub of the new forms is named, and no earlier family's name is among them"""
    api = pkg("api")
    seen = set()
    for dt in DTYPES:
        t, c = ("f64", "double") if dt is np.float64 else ("f32", "float")
        for kind in A.KINDS:
            for n in range(1, 1025):
                name = api.ard_predict_kernel_name(dt, kind, n)
                nt, full = (n + 15) // 16, "true" if n % 16 == 0 else "false"
                want = f"matinv_logdet_tile_{t}<{nt}, {full}, true, true>" if n <= 96 else f"matinv_logdet_global<{c}, true, true>"
                assert name == want, (n, name)
                seen.add(name)
    assert seen <= audit.STUBS, sorted(seen - audit.STUBS)  # exactly a stub, not a prefix of one

    def nargs(s):
        return len(s[s.index("<") + 1:-1].split(", "))

    forms = {s for s in audit.STUBS if (s.startswith("matinv_logdet_global<") and nargs(s) == 3) or
             (s.startswith("matinv_logdet_tile_f") and nargs(s) == 4)}
    assert len(forms) == 26 and forms == seen, sorted(forms ^ seen)
    assert not [s for s in audit.STUBS if s.startswith(("matinv_logdet_global<", "matinv_logdet_tile_f")) and
                nargs(s) > (3 if s.startswith("matinv_logdet_global") else 4)]
    GJ, CH = api.ALGO_GAUSS_JORDAN, api.ALGO_CHOLESKY
    for dt in DTYPES:
        for n in (1, 2, 96, 97, 1024):
            earlier = [api.ard_logml_kernel_name(dt, A.SE, n), api.logml_kernel_name(dt, n), api.predict_kernel_name(dt, n),
                       api.logdet_kernel_name(CH, dt, n), api.logdet_kernel_name(GJ, dt, n), api.logdet_kernel_name(CH, dt, n, api.KERNEL_GLOBAL)]
            for e in earlier:
                assert e and e not in seen and any(audit.matches(e, s) for s in audit.STUBS), (n, e)
        for n in (-1, 0, 1025, 4096):
            assert api.ard_predict_kernel_name(dt, A.SE, n) == ""
        assert api.ard_predict_kernel_name(dt, 2, 32) == "" == api.ard_predict_kernel_name(dt, -1, 32)
    L = pkg("_lib").lib()
    assert L.matinv_ard_predict_kernel_name(2, 0, 32) == b"" == L.matinv_ard_predict_kernel_name(-1, 0, 32)


def test_ard_predict_argument_refusals_without_device():
    lib = pkg("_lib")
    L = lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    AUTO = object()

    def args(dtype=0, kind=0, n=4, d=2, q=3, x=p, xs=AUTO, y=p, ys=AUTO, th=p, xq=p, xqs=AUTO, mean=p, var=p, batch=2):
        return (dtype, kind, n, d, q, x, n * d if xs is AUTO else xs, y, n if ys is AUTO else ys, th, xq, q * d if xqs is AUTO else xqs,
                mean, var, batch, None)

    def dev(**kw):
        return L.matinv_ard_predict_batched(*args(**kw), None)

    def host(**kw):
        return L.matinv_ard_predict_batched_host(*args(**kw))

    def refused(rc, code, text):
        assert rc == code, (rc, code, text, L.matinv_last_error())
        assert text in L.matinv_last_error(), (text, L.matinv_last_error())

    none = dict(mean=None, var=None)
    nothing = dict(x=None, y=None, th=None, xq=None, **none)
    for f in (dev, host):
        # 1 check_head, 2 kind, 3 ndim >= 1: also for an empty batch; each comes before everything after it
        refused(f(n=0, dtype=2, kind=5, d=0), lib.ERR_ARG, b"n must be")
        refused(f(dtype=2, kind=5, d=0), lib.ERR_ARG, b"unknown dtype")
        for kind in (-1, 2):
            refused(f(kind=kind, d=0, q=0), lib.ERR_ARG, b"unknown covariance function")
            refused(f(kind=kind, batch=0, **nothing), lib.ERR_ARG, b"unknown covariance function")
        for d in (0, -3):
            refused(f(d=d, q=0, xs=1), lib.ERR_ARG, b"ndim must be >= 1")
            refused(f(d=d, batch=0, **nothing), lib.ERR_ARG, b"ndim must be >= 1")
        # 4 the empty batch is a no-op after them
        assert f(batch=0, **nothing) == lib.OK
        assert f(batch=0, q=0, xs=3, ys=1, xqs=5, d=17, **nothing) == lib.OK
        assert f(batch=0, dtype=5, **nothing) == lib.ERR_ARG
        assert f(batch=0, n=0, **nothing) == lib.ERR_ARG
        # 5 nquery, before the strides
        for q in (0, -2):
            refused(f(q=q, xs=7, x=None), lib.ERR_ARG, b"nquery must be >= 1")
        # 6 the three strides, in their order, before the pointers
        refused(f(xs=7, ys=5, xqs=5, x=None), lib.ERR_ARG, b"xstride must be")
        refused(f(xs=4), lib.ERR_ARG, b"xstride must be")
        refused(f(ys=5, xqs=5, x=None), lib.ERR_ARG, b"ystride must be")
        refused(f(ys=8), lib.ERR_ARG, b"ystride must be")
        refused(f(xqs=5, x=None), lib.ERR_ARG, b"xqstride must be")
        refused(f(xqs=2), lib.ERR_ARG, b"xqstride must be")
        refused(f(xqs=12), lib.ERR_ARG, b"xqstride must be")
        assert f(xs=0, ys=0, xqs=0, batch=0x80000000) == lib.ERR_ARG  # stride 0 is no refusal: the next one is the batch
        assert b"batch" in L.matinv_last_error()
        # 7 pointers, before the outputs
        for one in ("x", "th", "xq"):
            refused(f(**{one: None}, **none), lib.ERR_ARG, b"null device pointer")
        # 8 outputs
        refused(f(**none), lib.ERR_ARG, b"no output requested")
        refused(f(y=None), lib.ERR_ARG, b"mean requested without the observations")
        refused(f(y=None, var=None, d=17), lib.ERR_ARG, b"mean requested without the observations")
        # 9 check_tail: the batch, then n; y may be null without mean
        refused(f(batch=0x80000000, n=1025, d=17), lib.ERR_ARG, b"batch")
        refused(f(n=1025, batch=1, d=17), lib.ERR_UNSUPPORTED, b"n=1025")
        refused(f(n=1025, batch=1, y=None, mean=None), lib.ERR_UNSUPPORTED, b"n=1025")
        assert f(n=1025, batch=1, x=None) == lib.ERR_ARG
        # 10 the ndim limit, after the pointer checks
        refused(f(d=17), lib.ERR_UNSUPPORTED, b"ndim=17")
        refused(f(d=17, y=None, mean=None), lib.ERR_UNSUPPORTED, b"ndim=17")
        refused(f(d=17, x=None), lib.ERR_ARG, b"null device pointer")
        refused(f(d=17, **none), lib.ERR_ARG, b"no output requested")


def test_api_argument_validation():
    api = pkg("api")
    n, d, Q = 4, 2, 3
    X, y, th, Xq = np.zeros((2, n, d)), np.zeros((2, n)), np.zeros((2, d + 2)), np.zeros((2, Q, d))
    with pytest.raises(ValueError, match="want must name"):
        api.ard_predict_batched_host(n, X, y, th, Xq, want=("mean", "cov"))
    with pytest.raises(ValueError, match="want must name"):
        api.ard_predict_batched_host(n, X, y, th, Xq, want=())
    with pytest.raises(ValueError, match="mean needs y"):
        api.ard_predict_batched_host(n, X, None, th, Xq)
    with pytest.raises(ValueError, match="Xq must be"):
        api.ard_predict_batched_host(n, X, y, th, Xq.reshape(-1))
    with pytest.raises(ValueError, match="Xq must be"):
        api.ard_predict_batched_host(n, X, y, th, np.zeros((2, Q, d + 1)))
    with pytest.raises(ValueError, match="Xq needs"):
        api.ard_predict_batched_host(n, np.zeros((3, n, d)), np.zeros((3, n)), np.zeros((3, d + 2)), Xq)
    with pytest.raises(TypeError, match="one dtype"):
        api.ard_predict_batched_host(n, X, y, th, Xq.astype(np.float32))
    size = lambda a: a.size  # noqa: E731
    # the present callers get the present tuple; with Xq it goes on with (nquery, xqstride); a shared query set is recognised by its size
    assert api._ard_plan(n, X, y, th, None, None, size) == (d, 2, n * d, n)
    assert api._ard_plan(n, X, y, th, None, None, size, Xq) == (d, 2, n * d, n, Q, Q * d)
    assert api._ard_plan(n, X[0], y[0], th, None, None, size, Xq[0]) == (d, 2, 0, 0, Q, 0)
    assert api._ard_plan(n, X, None, th, None, None, size, Xq[:1]) == (d, 2, n * d, n, Q, 0)
    assert api._ard_plan(n, X[0], y[0], th[:1], None, None, size, Xq[0]) == (d, 1, n * d, n, Q, Q * d)


@pytest.mark.parametrize("kind", A.KINDS)
def test_reference_equals_a_direct_evaluation(kind):
    """mean and var of the augmented-set construction against K-based formulas written out here, to 1e-12"""
    n, d, Q, batch = 9, 3, 5, 3
    X, y, th = A.inputs(n, d, batch, np.float64, seed=3)
    Xq = AP.queries(n, d, batch, Q, np.float64, seed=4)
    Xq[:, 0] = X[:, 2]  # a query on a training point: no noise in its a_j
    ref = AP.reference(X, y, th, Xq, n, d, Q, kind, AP.U[np.dtype(np.float64)], np.float64)
    for k in range(batch):
        sf2, ell, sn2 = np.exp(th[k, 0]), np.exp(th[k, 1:d + 1]), np.exp(th[k, d + 1])
        z, zq = X[k] / ell, Xq[k] / ell
        phi = lambda s: A.element(s, kind)[0]  # noqa: E731
        M = sf2 * phi(((z[:, None] - z[None]) ** 2).sum(axis=2)) + sn2 * np.eye(n)
        a = sf2 * phi(((z[:, None] - zq[None]) ** 2).sum(axis=2))  # (n, Q)
        K = np.linalg.inv(M)
        assert np.abs(a.T @ K @ y[k] - ref["mean"][k]).max() <= 1e-12
        assert np.abs(sf2 - np.einsum("iq,ij,jq->q", a, K, a) - ref["var"][k]).max() <= 1e-12
        assert a[2, 0] == sf2 * phi(np.float64(0.0)) == ref["a"][k, 0, 2]
    ev = AP.evaluation(X, y, th, Xq, n, d, Q, kind, np.float64)
    assert np.abs(ev["mean"].reshape(batch, Q) - ref["mean"]).max() <= 1e-12 and np.abs(ev["var"].reshape(batch, Q) - ref["var"]).max() <= 1e-12
    # y is optional without the mean, and the first queries of a reference are the reference of the first queries
    r2 = AP.reference(X, None, th, Xq[:, :2], n, d, 2, kind, AP.U[np.dtype(np.float64)], np.float64)
    assert "mean" not in r2 and np.array_equal(r2["var"], AP.first_queries(ref, 2)["var"])
    assert np.array_equal(r2["dA"], AP.first_queries(ref, 2)["dA"])


@pytest.mark.parametrize("kind", A.KINDS)
def test_gpu_cases_are_well_conditioned_and_float32_numpy_stays_inside_the_bounds(kind):
    """cond2(M) <= COND_CAP for every matrix the GPU tests use (both dtypes draw the same points), and the float32 numpy evaluation of
    the formulas lies inside the fp32 bounds at each (n, d, Q) of them"""
    u32 = AP.U[np.dtype(np.float32)]
    worst, worst_cond = {}, 0.0
    for n, d in AP.gpu_cases():
        batch = AP.batch_of(n)
        X, y, th = A.inputs(n, d, batch, np.float32)
        Xq = AP.queries(n, d, batch, AP.QMAX, np.float32)
        ref = AP.reference(X, y, th, Xq, n, d, AP.QMAX, kind, u32, np.float32)
        assert ref["cond"].max() <= A.COND_CAP, (n, d, kind, float(ref["cond"].max()))
        if n <= 130:
            X64, _, th64 = A.inputs(n, d, batch, np.float64)
            M64 = A.formulas(X64, np.zeros((batch, n)), th64, n, d, kind, np.float64)["M"]
            assert np.linalg.cond(M64).max() <= A.COND_CAP, (n, d, kind)
        worst_cond = max(worst_cond, float(ref["cond"].max()))
        ev = AP.evaluation(X, y, th, Xq, n, d, AP.QMAX, kind, np.float32)
        for Q in AP.QS:  # the first Q queries: what the GPU tests run
            sub = {k: v.reshape(batch, AP.QMAX)[:, :Q].reshape(-1) for k, v in ev.items()}
            for k, v in AP.ratios(sub, AP.first_queries(ref, Q), n, u32).items():
                assert (v <= 1.0).all(), (n, d, Q, kind, k, float(v.max()))
                worst[k] = max(worst.get(k, 0.0), float(v.max()))
    print(f"kind={kind}: worst cond {worst_cond:.1f}; float32 numpy worst err/bound " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    for i, (n, d, Q, batch, dt, knd, shared, rejects) in enumerate(AP.STRIDE_CASES):
        X, y, th, Xq, _ = AP.stride_inputs(n, d, Q, 64, dt, knd, shared, {})
        assert AP.reference(X, y, th, Xq, n, d, Q, knd, AP.U[np.dtype(dt)], dt)["cond"].max() <= A.COND_CAP


WRONG = ("noise at a coincident point", "query not divided by l", "two dimensions swapped", "prior variance with noise",
         "phi of the other kind", "one training point dropped")


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", A.KINDS)
def test_bounds_reject_wrong_results(dt, kind):
    n, d, Q = 33, 3, 17
    batch = AP.batch_of(n)
    u = AP.U[np.dtype(dt)]
    X, y, th = A.inputs(n, d, batch, dt)
    Xq = AP.queries(n, d, batch, Q, dt)
    Xq[:, 0] = X[:, 5]  # one query on a training point
    ref = AP.reference(X, y, th, Xq, n, d, Q, kind, u, dt)
    good = AP.evaluation(X, y, th, Xq, n, d, Q, kind, np.float64)
    assert all((v <= 1.0).all() for v in AP.ratios(good, ref, n, u).values())
    for what in WRONG:
        rs = AP.ratios(AP.evaluation(X, y, th, Xq, n, d, Q, kind, np.float64, wrong=what), ref, n, u)
        per_matrix = np.maximum.reduce([v.max(axis=1) for v in rs.values()])
        print(f"  {what}: err/bound {per_matrix.max():.3g} .. {per_matrix.min():.3g}")
        # every matrix is caught -- but for the swap, which no bound can see in a matrix whose queries happen to have two coordinates
        # that agree to within it: there three quarters of the matrices are asked for, as tests/test_ard_cpu.py does
        caught = per_matrix > 1.0
        assert caught.mean() >= 0.75 if what == "two dimensions swapped" else caught.all(), (what, per_matrix)
