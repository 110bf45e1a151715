"""CPU-side checks of the gradients of the batched GP leave-one-out log pseudo-likelihood (matinv_loo_grad_batched*): exports, argument
errors, dispatch names, the audit of the compiled LOO-gradient kernel forms that the generated instantiation sweep cannot make (the forms
carry the names of the SPD inversion kernels with five more template arguments), the reference of tests/_loo_grad_worker.py against
finite differences of the LOO reference, its two exact identities, and the check that the bounds hold for a float32 numpy evaluation of
the reference formulas. No GPU needed."""
import ctypes
import re

import numpy as np
import pytest

import _loo_grad_worker as W
import _loo_worker as L
import test_instantiations_cpu as audit
from conftest import pkg

NAMES = ["matinv_loo_grad_batched", "matinv_loo_grad_kernel_name", "matinv_loo_grad_batched_host"]


def test_loo_grad_symbols_exported():
    lib = pkg("_lib")
    Lb = lib.lib()
    for name in NAMES:
        assert hasattr(Lb, name), name
        assert name in lib.NATIVE_NAMES
    assert Lb.matinv_abi_version() == 2
    api = pkg("api")
    for name in ("loo_grad_batched", "loo_grad_batched_host", "loo_grad_kernel_name"):
        assert callable(getattr(api, name))


def test_loo_grad_argument_errors_without_device():
    lib = pkg("_lib")
    Lb = lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def dev(dtype=0, n=4, nparam=1, b=p, c=p, d=p, dm=p, grad=p, gradc=p, logpl=p, batch=2):
        return Lb.matinv_loo_grad_batched(dtype, n, nparam, b, c, d, dm, grad, gradc, logpl, batch, None, None)

    def host(dtype=0, n=4, nparam=1, b=p, c=p, d=p, dm=p, grad=p, gradc=p, logpl=p, batch=2):
        return Lb.matinv_loo_grad_batched_host(dtype, n, nparam, b, c, d, dm, grad, gradc, logpl, batch, None)

    nothing = dict(b=None, c=None, d=None, dm=None, grad=None, gradc=None, logpl=None)
    for f in (dev, host):
        assert f(n=0) == lib.ERR_ARG
        assert b"n must be" in Lb.matinv_last_error()
        assert f(n=-2) == lib.ERR_ARG
        assert f(dtype=2) == lib.ERR_ARG
        assert f(b=None) == lib.ERR_ARG
        assert f(d=None) == lib.ERR_ARG
        assert f(grad=None, gradc=None, logpl=None) == lib.ERR_ARG
        assert b"output" in Lb.matinv_last_error()
        # grad needs at least one derivative matrix, and the matrices themselves
        assert f(nparam=0) == lib.ERR_ARG
        assert b"nparam" in Lb.matinv_last_error()
        assert f(dm=None) == lib.ERR_ARG
        assert b"dDMs" in Lb.matinv_last_error()
        assert f(nparam=-1) == lib.ERR_ARG
        assert f(nparam=-1, grad=None) == lib.ERR_ARG
        # batch == 0 is a no-op even with NULL pointers; n and dtype are still checked
        assert f(batch=0, **nothing) == lib.OK
        assert f(batch=0, nparam=0, **nothing) == lib.OK
        assert f(batch=0, dtype=5, **nothing) == lib.ERR_ARG
        assert f(batch=0, n=0, **nothing) == lib.ERR_ARG
        # n = 1025 is refused after the pointer checks: any single output passes them, so do a NULL c and, without grad, nparam = 0 and
        # a NULL dDMs
        assert f(n=1025, batch=1) == lib.ERR_UNSUPPORTED
        assert f(n=1025, batch=1, gradc=None, logpl=None) == lib.ERR_UNSUPPORTED
        assert f(n=1025, batch=1, grad=None, logpl=None) == lib.ERR_UNSUPPORTED
        assert f(n=1025, batch=1, grad=None, gradc=None) == lib.ERR_UNSUPPORTED
        assert f(n=1025, batch=1, grad=None, nparam=0, dm=None) == lib.ERR_UNSUPPORTED
        assert f(n=1025, batch=1, c=None) == lib.ERR_UNSUPPORTED
        assert f(n=1025, batch=1, grad=None, gradc=None, logpl=None) == lib.ERR_ARG
        assert f(n=1025, batch=1, d=None) == lib.ERR_ARG
        assert f(n=1025, batch=1, nparam=0) == lib.ERR_ARG
        assert f(n=1025, batch=1, dm=None) == lib.ERR_ARG
    assert dev(batch=0x80000000) == lib.ERR_ARG
    assert b"batch" in Lb.matinv_last_error()


@pytest.mark.parametrize("f64", [True, False])
def test_loo_grad_dispatch_names(f64):
    api = pkg("api")
    dt, t, c = (api.F64, "f64", "double") if f64 else (api.F32, "f32", "float")
    tail = "true, true, true, true, true>"
    assert api.loo_grad_kernel_name(dt, 1) == f"matinv_spd_tile_{t}<1, false, {tail}"
    assert api.loo_grad_kernel_name(dt, 16) == f"matinv_spd_tile_{t}<1, true, {tail}"
    assert api.loo_grad_kernel_name(dt, 17) == f"matinv_spd_tile_{t}<2, false, {tail}"
    assert api.loo_grad_kernel_name(dt, 95) == f"matinv_spd_tile_{t}<6, false, {tail}"
    assert api.loo_grad_kernel_name(dt, 96) == f"matinv_spd_tile_{t}<6, true, {tail}"
    assert api.loo_grad_kernel_name(dt, 97) == f"matinv_chol_global<{c}, {tail}"
    assert api.loo_grad_kernel_name(dt, 1024) == f"matinv_chol_global<{c}, {tail}"
    assert api.loo_grad_kernel_name(dt, 0) == "" == api.loo_grad_kernel_name(dt, 1025)
    assert api.loo_grad_kernel_name(9, 32) == "" == api.loo_grad_kernel_name(-1, 200)


def test_loo_grad_host_form_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    api = pkg("api")
    lib = pkg("_lib")
    a = np.eye(20).reshape(-1)
    d = np.ones(20)
    calls = (lambda: api.loo_grad_batched_host(20, a, d, d, a), lambda: api.loo_grad_batched_host(20, a, None, d, None, want=("logpl",)))
    for call in calls:
        with pytest.raises(lib.MatinvError) as e:
            call()
        assert e.value.code in (lib.ERR_NO_DEVICE, lib.ERR_HIP)
        assert lib.lib().matinv_last_error()


LOO_GRAD_FORMS = (r"matinv_spd_tile_f(64|32)<\d+, (true|false), true, true, true, true, true>",
                  r"matinv_chol_global<(double|float), true, true, true, true, true>")


@pytest.mark.skipif(audit.NM is None, reason="no nm on this machine")
def test_every_loo_gradient_name_is_a_compiled_kernel_and_every_loo_gradient_form_is_named():
    """what test_instantiations_cpu checks for the routes of the generated sweep, for the LOO-gradient forms: exact names, both directions"""
    api = pkg("api")
    named = {api.loo_grad_kernel_name(dt, n) for dt in (api.F64, api.F32) for n in range(1, 1025)}
    assert "" not in named and len(named) == 2 * (12 + 1)
    missing = sorted(named - audit.STUBS)
    assert not missing, f"named by matinv_loo_grad_kernel_name but not compiled: {missing}"
    compiled = {s for s in audit.STUBS if any(re.fullmatch(p, s) for p in LOO_GRAD_FORMS)}
    assert compiled, "no LOO-gradient form is compiled"
    assert not sorted(compiled - named), f"compiled LOO-gradient forms no n reaches: {sorted(compiled - named)}"
    # the audits of the earlier forms do not take a LOO-gradient form for one of theirs, and this one takes none of theirs
    import test_logml_grad_cpu
    import test_loo_cpu
    import test_predict_cov_cpu
    import test_predict_cpu
    earlier = test_loo_cpu.LOO_FORMS + test_logml_grad_cpu.GRAD_FORMS + test_predict_cpu.PREDICT_FORMS + test_predict_cov_cpu.PREDICT_COV_FORMS
    assert not any(re.fullmatch(p, s) for p in earlier for s in named)
    others = {f(dt, n) for dt in (api.F64, api.F32) for n in range(1, 1025)
              for f in (api.loo_kernel_name, api.logml_grad_kernel_name, api.predict_kernel_name, api.predict_cov_kernel_name)}
    assert not any(re.fullmatch(p, s) for p in LOO_GRAD_FORMS for s in others)


FD_H = 1e-4


@pytest.mark.parametrize("n", [5, 17, 64])
def test_reference_is_the_gradient_of_the_reference_logpl(n):
    """the float64 reference against central differences of _loo_worker.reference(...)["logpl"]: along every dM_p and along three c_i.

    Tolerance, for the step h = FD_H: a central difference of f(h) = logpl(M + h D) is off by h^2 / 6 |f'''| plus (|df(h)| + |df(-h)|) /
    (2 h), df the rounding error of one evaluation of f.
      * rounding: df <= the float64 bound of _loo_worker.bounds for logpl, so this term is that bound / h.
      * truncation: K(h) = (M + h D)^-1 = K (I + h D K)^-1 is a Neumann series in x = h rho0, rho0 = ||K||_2 ||D||_2; kappa_i >= ||K||_2 /
        cond, so relative to its value every factor of f (kappa_i, alpha_i) is majorised by 1 / (1 - h rho), rho = rho0 cond. Then
        1/2 log kappa_i is majorised by 1/2 log(1 / (1 - x)), third derivative 1/2 * 2 rho^3, and 1/2 alpha_i^2 / kappa_i (three such
        factors) by 1/2 (alpha_i^2 / kappa_i) (1 - x)^-3, third derivative 1/2 * 60 rho^3:  |f'''| <= rho^3 (n + 30 sum_i alpha_i^2 / kappa_i).
    """
    h, nparam, batch = FD_H, 2, 3
    B, c, d = W.inputs(n, batch, np.float64)
    dMs = W.derivs(n, batch, nparam, np.float64)
    ref = W.reference(B, c, d, dMs, n, nparam)
    knorm = np.linalg.norm(ref["K"], 2, axis=(1, 2))
    quad = (ref["alpha"] ** 2 / ref["kappa"]).sum(axis=1)
    rounding = L.bounds(ref, n, W.U[np.dtype(np.float64)])[2] / h

    def tol(k, dnorm2):
        rho = knorm[k] * dnorm2 * ref["cond"][k]
        return h * h / 6 * rho ** 3 * (n + 30 * quad[k]) + rounding[k]

    flat = dMs.reshape(batch, nparam, n * n)
    worst = 0.0
    for p_ in range(nparam):
        step = (h * flat[:, p_]).reshape(-1)
        dq = (L.reference(B + step, c, d, n)["logpl"] - L.reference(B - step, c, d, n)["logpl"]) / (2 * h)
        for k in range(batch):
            t = tol(k, np.linalg.norm(ref["dM"][k, p_], 2))
            worst = max(worst, abs(dq[k] - ref["grad"][k, p_]) / t)
            assert abs(dq[k] - ref["grad"][k, p_]) <= t, (n, k, p_, dq[k], ref["grad"][k, p_], t)
    for i in (0, n // 2, n - 1):
        e = np.zeros((batch, n))
        e[:, i] = h
        e = e.reshape(-1)
        dq = (L.reference(B, c + e, d, n)["logpl"] - L.reference(B, c - e, d, n)["logpl"]) / (2 * h)
        for k in range(batch):
            t = tol(k, 1.0)
            worst = max(worst, abs(dq[k] - ref["gradc"][k, i]) / t)
            assert abs(dq[k] - ref["gradc"][k, i]) <= t, (n, k, i, dq[k], ref["gradc"][k, i], t)
    print(f"  n={n} h={h}: worst |difference| / tolerance {worst:.3f}")
    # and the value itself is the LOO reference's
    assert np.allclose(ref["logpl"], L.reference(B, c, d, n)["logpl"], rtol=1e-13, atol=0)


def identity_derivs(M, n, i):
    """flat dMs with P = 3 per matrix: dM_0 = M, dM_1 = e_i e_i^T, dM_2 = e_0 e_0^T"""
    batch = M.shape[0]
    dM = np.zeros((batch, 3, n, n))
    dM[:, 0] = M
    dM[:, 1, i, i] = 1.0
    dM[:, 2, 0, 0] = 1.0
    return dM.reshape(-1)


def identity_targets(ref, n, i):
    """what the two identities say grad[:, 0 .. 2] is, from the other quantities of the reference"""
    t0 = -0.5 * n + 0.5 * (ref["alpha"] ** 2 / ref["kappa"]).sum(axis=1)
    return np.stack([t0, ref["gradc"][:, i], ref["gradc"][:, 0]], axis=1)


@pytest.mark.parametrize("n", [1, 17, 64, 96])
def test_the_two_exact_identities_of_the_reference(n):
    """dM_p = e_i e_i^T gives grad_p = gradc_i (the sum holds one non-zero term: the same bits); dM_p = M gives grad_p = -n/2 + 1/2 sum_i
    alpha_i^2 / kappa_i (logpl is homogeneous: scaling M by t scales kappa and alpha by 1/t), here to the float64 bound of grad"""
    B, c, d = W.inputs(n, 4, np.float64)
    i = n - 1
    dMs = identity_derivs(W.image(B, c, n), n, i)
    ref = W.reference(B, c, d, dMs, n, 3)
    want = identity_targets(ref, n, i)
    assert np.array_equal(ref["grad"][:, 1:], want[:, 1:])
    b_grad = W.bounds(ref, n, W.U[np.dtype(np.float64)])[0]
    assert (np.abs(ref["grad"][:, 0] - want[:, 0]) <= b_grad[:, 0]).all()


@pytest.mark.parametrize("n", W.TILE_SIZES + W.GLOBAL_SIZES)
def test_float32_numpy_stays_inside_the_fp32_bounds(n):
    """the bounds are derived, not fitted: a float32 numpy evaluation of the reference formulas (LAPACK inverse, matmul, einsum) must pass
    them at every size, shape and input the GPU accuracy test uses, before they are held against the kernels"""
    dt = np.float32
    for nparam in (1, 3):
        for with_c in (True, False):
            B, c, d = W.inputs(n, W.batch_of(n), dt, with_c)
            dMs = W.derivs(n, W.batch_of(n), nparam, dt)
            got = W.float32_evaluation(B, c, d, dMs, n, nparam)
            W.check(*got, W.reference(B, c, d, dMs, n, nparam), n, W.U[np.dtype(dt)], what=f"float32 numpy P={nparam} c={with_c}")
