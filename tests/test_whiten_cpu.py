"""CPU-side checks of the batched whitening, Mahalanobis distances and Gaussian log-density (matinv_whiten_batched*): exports, argument
errors, dispatch names, the audit of the compiled whiten kernel forms that the generated instantiation sweep cannot make (the forms carry
the names of the SPD inversion kernels with seven more template arguments), the meaning of the reference, and the check that the bounds of
tests/_whiten_worker.py hold for a float32 numpy evaluation of the reference formulas. No GPU needed."""
import ctypes
import re

import numpy as np
import pytest

import _whiten_worker as W
import test_instantiations_cpu as audit
from conftest import pkg

NAMES = ["matinv_whiten_batched", "matinv_whiten_kernel_name", "matinv_whiten_batched_host"]


def test_whiten_symbols_exported():
    lib = pkg("_lib")
    L = lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in lib.NATIVE_NAMES
    api = pkg("api")
    for name in ("whiten_batched", "whiten_batched_host", "whiten_kernel_name"):
        assert callable(getattr(api, name))


def test_whiten_argument_errors_without_device():
    """the checks of matinv_colour_batched, same codes, same order"""
    lib = pkg("_lib")
    L = lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def dev(dtype=0, q=4, npoint=2, c=p, stride=16, m=p, x=p, w=p, mh=p, ld=p, lp=p, batch=2):
        return L.matinv_whiten_batched(dtype, q, npoint, c, stride, m, x, w, mh, ld, lp, batch, None, None)

    def host(dtype=0, q=4, npoint=2, c=p, stride=16, m=p, x=p, w=p, mh=p, ld=p, lp=p, batch=2):
        return L.matinv_whiten_batched_host(dtype, q, npoint, c, stride, m, x, w, mh, ld, lp, batch, None)

    none = dict(w=None, mh=None, ld=None, lp=None)
    nothing = dict(c=None, m=None, x=None, **none)
    for f in (dev, host):
        assert f(q=0) == lib.ERR_ARG
        assert b"q must be" in L.matinv_last_error()
        assert f(dtype=2) == lib.ERR_ARG
        assert f(c=None) == lib.ERR_ARG
        assert f(**none) == lib.ERR_ARG
        assert b"output" in L.matinv_last_error()
        # X and S are needed with W, maha or logpdf, and only with them
        for one in ("w", "mh", "lp"):
            only = dict(none, **{one: p})
            assert f(x=None, **only) == lib.ERR_ARG
            assert b"dX" in L.matinv_last_error()
            assert f(npoint=0, **only) == lib.ERR_ARG
            assert b"npoint" in L.matinv_last_error()
        assert f(stride=15) == lib.ERR_ARG
        assert b"strideC" in L.matinv_last_error()
        # the order of colour_check_args: q before dtype, the missing output before the stride
        assert f(q=0, dtype=2) == lib.ERR_ARG and b"q must be" in L.matinv_last_error()
        assert f(stride=15, **none) == lib.ERR_ARG and b"output" in L.matinv_last_error()
        # batch == 0 is a no-op even with NULL pointers; q and dtype are still checked
        assert f(batch=0, **nothing) == lib.OK
        assert f(batch=0, dtype=5, **nothing) == lib.ERR_ARG
        assert f(batch=0, q=0, **nothing) == lib.ERR_ARG
        # q = 1025 and S = 1025 are refused after the pointer checks
        big = 1025 * 1025
        assert f(batch=1, q=1025, stride=big) == lib.ERR_UNSUPPORTED
        assert f(batch=1, q=1025, stride=big, x=None, npoint=0, **dict(none, ld=p)) == lib.ERR_UNSUPPORTED
        assert f(batch=1, q=1025, stride=big, **none) == lib.ERR_ARG
        assert f(batch=1, q=1025, stride=big, c=None) == lib.ERR_ARG
        assert f(batch=1, npoint=1025) == lib.ERR_UNSUPPORTED
        assert b"npoint" in L.matinv_last_error()
        assert f(batch=0x80000000) == lib.ERR_ARG
        assert b"batch" in L.matinv_last_error()


def test_api_argument_validation():
    """api.whiten_batched refuses what it can see before the library is called"""
    torch = pytest.importorskip("torch")
    api = pkg("api")
    q = 4
    C = torch.eye(q, dtype=torch.float64).reshape(-1).repeat(2)
    X = torch.zeros(2 * 3 * q, dtype=torch.float64)
    with pytest.raises(ValueError):  # CPU tensors
        api.whiten_batched(q, C, None, X)
    if torch.cuda.is_available():
        C, X = C.cuda(), X.cuda()
        with pytest.raises(ValueError, match="want holds"):
            api.whiten_batched(q, C, None, X, want=("W", "L"))
        with pytest.raises(ValueError, match="no output"):
            api.whiten_batched(q, C, None, X, want=())
        with pytest.raises(ValueError, match="need the points"):
            api.whiten_batched(q, C, None, None, want=("maha",))
        with pytest.raises(ValueError, match="Xs needs"):
            api.whiten_batched(q, C, None, X[:q], want=("W",))
        with pytest.raises(TypeError):
            api.whiten_batched(q, C, None, X.float())
        with pytest.raises(ValueError, match="Ms needs"):
            api.whiten_batched(q, C, X[:q], X)
        with pytest.raises(ValueError, match="Ms needs"):
            api.whiten_batched(q, C, None, X, maha=X[:5], want=())
        with pytest.raises(ValueError, match="info"):
            api.whiten_batched(q, C, None, X, info=torch.zeros(2, dtype=torch.int64, device="cuda"))
    # the host form validates before it needs a device
    Cn, Xn = np.tile(np.eye(q).reshape(-1), 2), np.zeros(2 * 3 * q)
    with pytest.raises(ValueError, match="want must name"):
        api.whiten_batched_host(q, Cn, None, Xn, want=())
    with pytest.raises(ValueError, match="want must name"):
        api.whiten_batched_host(q, Cn, None, Xn, want=("Y",))
    with pytest.raises(ValueError, match="need the points"):
        api.whiten_batched_host(q, Cn, None, None, want=("logpdf",))
    with pytest.raises(ValueError, match="Xs needs"):
        api.whiten_batched_host(q, Cn, None, Xn[:q], want=("W",))
    with pytest.raises(TypeError):
        api.whiten_batched_host(q, Cn, None, Xn.astype(np.float32))
    with pytest.raises(ValueError, match="Ms smaller"):
        api.whiten_batched_host(q, Cn, Xn[:q], Xn)


@pytest.mark.parametrize("f64", [True, False])
def test_whiten_dispatch_names(f64):
    api = pkg("api")
    dt, t, c = (api.F64, "f64", "double") if f64 else (api.F32, "f32", "float")
    seven = "true, true, true, true, true, true, true"
    assert api.whiten_kernel_name(dt, 1) == f"matinv_spd_tile_{t}<1, false, {seven}>"
    assert api.whiten_kernel_name(dt, 16) == f"matinv_spd_tile_{t}<1, true, {seven}>"
    assert api.whiten_kernel_name(dt, 17) == f"matinv_spd_tile_{t}<2, false, {seven}>"
    assert api.whiten_kernel_name(dt, 96) == f"matinv_spd_tile_{t}<6, true, {seven}>"
    assert api.whiten_kernel_name(dt, 97) == f"matinv_chol_global<{c}, {seven}>"
    assert api.whiten_kernel_name(dt, 1024) == f"matinv_chol_global<{c}, {seven}>"
    assert api.whiten_kernel_name(dt, 0) == "" == api.whiten_kernel_name(dt, 1025)
    assert api.whiten_kernel_name(9, 32) == "" == api.whiten_kernel_name(-1, 200)
    assert api.whiten_kernel_name(np.float64 if f64 else np.float32, 33) == api.whiten_kernel_name(dt, 33)


def test_host_form_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    api = pkg("api")
    lib = pkg("_lib")
    C = np.eye(20).reshape(-1)
    x = np.ones(3 * 20)
    calls = (lambda: api.whiten_batched_host(20, C, np.ones(20), x),
             lambda: api.whiten_batched_host(20, C, None, None, want=("logdet",)))
    for call in calls:
        with pytest.raises(lib.MatinvError) as err:
            call()
        assert err.value.code in (lib.ERR_NO_DEVICE, lib.ERR_HIP)
        assert lib.lib().matinv_last_error()


WHITEN_FORMS = (r"matinv_spd_tile_f(64|32)<\d+, (true|false), true, true, true, true, true, true, true>",
                r"matinv_chol_global<(double|float), true, true, true, true, true, true, true>")


@pytest.mark.skipif(audit.NM is None, reason="no nm on this machine")
def test_every_whiten_name_is_a_compiled_kernel_and_every_whiten_form_is_named():
    """what test_instantiations_cpu checks for the routes of the generated sweep, for the whiten forms: exact names, both directions"""
    api = pkg("api")
    named = {api.whiten_kernel_name(dt, q) for dt in (api.F64, api.F32) for q in range(1, 1025)}
    assert "" not in named and len(named) == 2 * (12 + 1)
    assert all(any(re.fullmatch(p, s) for p in WHITEN_FORMS) for s in named)
    missing = sorted(named - audit.STUBS)
    assert not missing, f"named by matinv_whiten_kernel_name but not compiled: {missing}"
    compiled = {s for s in audit.STUBS if any(re.fullmatch(p, s) for p in WHITEN_FORMS)}
    assert compiled, "no whiten form is compiled"
    assert not sorted(compiled - named), f"compiled whiten forms no q reaches: {sorted(compiled - named)}"
    # the six earlier audits do not take a whiten form for one of theirs, nor the reverse
    import test_colour_cpu
    import test_logml_grad_cpu
    import test_loo_cpu
    import test_loo_grad_cpu
    import test_predict_cov_cpu
    import test_predict_cpu
    others = test_loo_cpu.LOO_FORMS + test_logml_grad_cpu.GRAD_FORMS + test_predict_cpu.PREDICT_FORMS + \
        test_predict_cov_cpu.PREDICT_COV_FORMS + test_loo_grad_cpu.LOO_GRAD_FORMS + test_colour_cpu.COLOUR_FORMS
    assert not any(re.fullmatch(p, s) for p in others for s in named)
    theirs = {s for s in audit.STUBS if any(re.fullmatch(p, s) for p in others)}
    assert theirs and not any(re.fullmatch(p, s) for p in WHITEN_FORMS for s in theirs)


@pytest.mark.parametrize("q", [1, 16, 17, 97])
def test_reference_solves_the_system_and_is_the_gaussian_log_density(q):
    C, m, X = W.case(q, "float64", 5)
    ref = W.whiten_reference(C, m, X, q)
    L, Wh = ref["L"], ref["W"].astype(np.float64)
    rhs = ref["z"] - ref["m"][:, None, :]
    # Lh Wh = x - m
    assert np.abs(np.einsum("kij,ksj->ksi", L, Wh) - rhs).max() < 1e-13 * max(1.0, np.abs(rhs).max())
    # maha = (x - m)^T C^-1 (x - m), logdet = slogdet, logpdf = the density of N(m, C), by a direct evaluation
    sol = np.linalg.solve(ref["C"], rhs.transpose(0, 2, 1)).transpose(0, 2, 1)
    maha = (rhs * sol).sum(axis=2)
    sign, logdet = np.linalg.slogdet(ref["C"])
    assert (sign == 1).all()
    assert np.abs(ref["maha"].astype(np.float64) - maha).max() < 1e-12 * max(1.0, maha.max())
    assert np.abs(ref["logdet"].astype(np.float64) - logdet).max() < 1e-12 * max(1.0, np.abs(logdet).max())
    direct = -0.5 * (maha + logdet[:, None] + q * np.log(2 * np.pi))
    assert np.abs(ref["logpdf"].astype(np.float64) - direct).max() < 1e-12 * max(1.0, np.abs(direct).max())
    assert np.abs(ref["Linv"] @ L - np.eye(q)).max() < 1e-13
    # the shared reference and its slices are this reference
    full = W.case_reference(q, "float64", 5)
    part = W.take(full, slice(0, 16))
    assert np.array_equal(full["W"], ref["W"]) and np.array_equal(part["W"], ref["W"][:, :16]) and part["L"] is full["L"]


@pytest.mark.parametrize("q", W.QSIZES + [1024])
def test_float32_numpy_stays_inside_the_fp32_bounds(q):
    """the bounds are derived, not fitted: a float32 numpy evaluation of the reference formulas must pass (3) - (5) and the logpdf bound
    at every size and point count the GPU tests use, before they are held against the kernels"""
    batch = 2 if q == 1024 else 20
    C, m, X = W.case(q, "float32", batch)
    full = W.whiten_reference(C, m, X, q)
    u = W.U[np.dtype(np.float32)]
    for S in ((1,) if q == 1024 else W.SS):
        x = W.samples(X, q, slice(0, S))
        W.check(W.float32_evaluation(C, m, x, q), W.take(full, slice(0, S)), q, u, what="float32 numpy")


def test_bounds_vanish_with_the_error_sources():
    """x = m: the reference is exactly zero and so is bound (4); a wrong W by one part in a thousand fails bound (3)"""
    q = 17
    C, m, X = W.case(q, "float64", 5)
    xm = np.ascontiguousarray(np.broadcast_to(m.reshape(5, 1, q), (5, 3, q))).reshape(-1)
    ref = W.whiten_reference(C, m, xm, q)
    u = W.U[np.dtype(np.float64)]
    assert not ref["W"].any() and not ref["maha"].any()
    assert not W.maha_bound(ref, q, u, W.w_bound(ref, q, u)).any()
    ref = W.whiten_reference(C, m, X, q)
    wrong = dict(W=(ref["W"].astype(np.float64) * 1.001).reshape(-1))
    with pytest.raises(AssertionError):
        W.check(wrong, ref, q, u, what="wrong on purpose")
