"""CPU-side checks of the gradients of the batched GP log marginal likelihood (matinv_logml_grad_batched*): exports, argument errors,
dispatch names, the audit of the compiled gradient kernel forms that the generated instantiation sweep cannot make (the forms carry the
names of the SPD inversion kernels with two more template arguments), and the check that the bounds of tests/_logml_grad_worker.py hold
for a float32 numpy evaluation of the reference formulas. No GPU needed."""
import ctypes
import re

import numpy as np
import pytest

import _logml_grad_worker as W
import test_instantiations_cpu as audit
from conftest import pkg

NAMES = ["matinv_logml_grad_batched", "matinv_logml_grad_kernel_name", "matinv_logml_grad_batched_host"]


def test_logml_grad_symbols_exported():
    lib = pkg("_lib")
    L = lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in lib.NATIVE_NAMES
    assert L.matinv_abi_version() == 2
    api = pkg("api")
    for name in ("logml_grad_batched", "logml_grad_batched_host", "logml_grad_kernel_name"):
        assert callable(getattr(api, name))


def test_logml_grad_argument_errors_without_device():
    lib = pkg("_lib")
    L = lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def dev(dtype=0, n=4, nparam=1, b=p, c=p, d=p, dm=p, grad=p, gradc=p, alpha=p, batch=2):
        return L.matinv_logml_grad_batched(dtype, n, nparam, b, c, d, dm, grad, gradc, alpha, batch, None, None)

    def host(dtype=0, n=4, nparam=1, b=p, c=p, d=p, dm=p, grad=p, gradc=p, alpha=p, batch=2):
        return L.matinv_logml_grad_batched_host(dtype, n, nparam, b, c, d, dm, grad, gradc, alpha, batch, None)

    nothing = dict(b=None, c=None, d=None, dm=None, grad=None, gradc=None, alpha=None)
    for f in (dev, host):
        assert f(n=0) == lib.ERR_ARG
        assert b"n must be" in L.matinv_last_error()
        assert f(n=-2) == lib.ERR_ARG
        assert f(dtype=2) == lib.ERR_ARG
        assert f(b=None) == lib.ERR_ARG
        assert f(d=None) == lib.ERR_ARG
        assert f(grad=None, gradc=None, alpha=None) == lib.ERR_ARG
        assert b"output" in L.matinv_last_error()
        # grad needs at least one derivative matrix, and the matrices themselves
        assert f(nparam=0) == lib.ERR_ARG
        assert b"nparam" in L.matinv_last_error()
        assert f(dm=None) == lib.ERR_ARG
        assert b"dDMs" in L.matinv_last_error()
        assert f(nparam=-1) == lib.ERR_ARG
        assert f(nparam=-1, grad=None) == lib.ERR_ARG
        # batch == 0 is a no-op even with NULL pointers; n and dtype are still checked
        assert f(batch=0, **nothing) == lib.OK
        assert f(batch=0, nparam=0, **nothing) == lib.OK
        assert f(batch=0, dtype=5, **nothing) == lib.ERR_ARG
        assert f(batch=0, n=0, **nothing) == lib.ERR_ARG
        # n = 2000 is refused after the pointer checks: any single output passes them, so do a NULL c and, without grad, nparam = 0 and
        # a NULL dDMs
        assert f(n=2000, batch=1) == lib.ERR_UNSUPPORTED
        assert f(n=2000, batch=1, gradc=None, alpha=None) == lib.ERR_UNSUPPORTED
        assert f(n=2000, batch=1, grad=None, alpha=None) == lib.ERR_UNSUPPORTED
        assert f(n=2000, batch=1, grad=None, gradc=None) == lib.ERR_UNSUPPORTED
        assert f(n=2000, batch=1, grad=None, nparam=0, dm=None) == lib.ERR_UNSUPPORTED
        assert f(n=2000, batch=1, c=None) == lib.ERR_UNSUPPORTED
        assert f(n=2000, batch=1, grad=None, gradc=None, alpha=None) == lib.ERR_ARG
        assert f(n=2000, batch=1, d=None) == lib.ERR_ARG
        assert f(n=2000, batch=1, nparam=0) == lib.ERR_ARG
        assert f(n=2000, batch=1, dm=None) == lib.ERR_ARG
    assert dev(batch=0x80000000) == lib.ERR_ARG
    assert b"batch" in L.matinv_last_error()


@pytest.mark.parametrize("f64", [True, False])
def test_logml_grad_dispatch_names(f64):
    api = pkg("api")
    dt, t, c = (api.F64, "f64", "double") if f64 else (api.F32, "f32", "float")
    assert api.logml_grad_kernel_name(dt, 1) == f"matinv_spd_tile_{t}<1, false, true, true>"
    assert api.logml_grad_kernel_name(dt, 15) == f"matinv_spd_tile_{t}<1, false, true, true>"
    assert api.logml_grad_kernel_name(dt, 16) == f"matinv_spd_tile_{t}<1, true, true, true>"
    assert api.logml_grad_kernel_name(dt, 17) == f"matinv_spd_tile_{t}<2, false, true, true>"
    assert api.logml_grad_kernel_name(dt, 96) == f"matinv_spd_tile_{t}<6, true, true, true>"
    assert api.logml_grad_kernel_name(dt, 97) == f"matinv_chol_global<{c}, true, true>"
    assert api.logml_grad_kernel_name(dt, 1024) == f"matinv_chol_global<{c}, true, true>"
    assert api.logml_grad_kernel_name(dt, 0) == "" == api.logml_grad_kernel_name(dt, 1025)
    assert api.logml_grad_kernel_name(9, 32) == "" == api.logml_grad_kernel_name(-1, 200)


def test_logml_grad_host_form_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    api = pkg("api")
    lib = pkg("_lib")
    a = np.eye(20).reshape(-1)
    d = np.ones(20)
    calls = (lambda: api.logml_grad_batched_host(20, a, d, d, a), lambda: api.logml_grad_batched_host(20, a, None, d, None, want=("alpha",)))
    for call in calls:
        with pytest.raises(lib.MatinvError) as e:
            call()
        assert e.value.code in (lib.ERR_NO_DEVICE, lib.ERR_HIP)
        assert lib.lib().matinv_last_error()


GRAD_FORMS = (r"matinv_spd_tile_f(64|32)<\d+, (true|false), true, true>", r"matinv_chol_global<(double|float), true, true>")


@pytest.mark.skipif(audit.NM is None, reason="no nm on this machine")
def test_every_gradient_name_is_a_compiled_kernel_and_every_gradient_form_is_named():
    """what test_instantiations_cpu checks for the routes of the generated sweep, for the gradient forms: exact names, both directions"""
    api = pkg("api")
    named = {api.logml_grad_kernel_name(dt, n) for dt in (api.F64, api.F32) for n in range(1, 1025)}
    assert "" not in named and len(named) == 2 * (12 + 1)
    missing = sorted(named - audit.STUBS)
    assert not missing, f"named by matinv_logml_grad_kernel_name but not compiled: {missing}"
    compiled = {s for s in audit.STUBS if any(re.fullmatch(p, s) for p in GRAD_FORMS)}
    assert compiled, "no gradient form is compiled"
    assert not sorted(compiled - named), f"compiled gradient forms no n reaches: {sorted(compiled - named)}"
    # and the LOO audit's patterns do not take a gradient form for a LOO form
    import test_loo_cpu
    assert not any(re.fullmatch(p, s) for p in test_loo_cpu.LOO_FORMS for s in named)


@pytest.mark.parametrize("n", W.TILE_SIZES + W.GLOBAL_SIZES)
def test_float32_numpy_stays_inside_the_fp32_bounds(n):
    """the bounds are derived, not fitted: a float32 numpy evaluation of the reference formulas (LAPACK inverse, einsum) must pass them
    at every size, shape and input the GPU accuracy test uses, before they are held against the kernels"""
    dt = np.float32
    for nparam in (1, 3):
        for with_c in (True, False):
            B, c, d = W.inputs(n, W.batch_of(n), dt, with_c)
            dMs = W.derivs(n, W.batch_of(n), nparam, dt)
            got = W.float32_evaluation(B, c, d, dMs, n, nparam)
            W.check(*got, W.reference(B, c, d, dMs, n, nparam), n, W.U[np.dtype(dt)], what=f"float32 numpy P={nparam} c={with_c}")


def test_reference_is_the_gradient_of_the_reference_logml():
    """the float64 reference against central differences of the log marginal likelihood in numpy: d/d theta_p and d/d c_i"""
    n, nparam = 6, 2
    B, c, d = W.inputs(n, 3, np.float64)
    dMs = W.derivs(n, 3, nparam, np.float64)
    ref = W.reference(B, c, d, dMs, n, nparam)

    def logml(M, dd):
        return -0.5 * dd @ np.linalg.solve(M, dd) - 0.5 * np.linalg.slogdet(M)[1]

    h = 1e-5
    for k in range(3):
        for p_ in range(nparam):
            dq = (logml(ref["M"][k] + h * ref["dM"][k, p_], ref["d"][k]) - logml(ref["M"][k] - h * ref["dM"][k, p_], ref["d"][k])) / (2 * h)
            assert abs(dq - ref["grad"][k, p_]) < 1e-8 * max(1.0, abs(dq))
        for i in range(n):
            e = np.zeros((n, n))
            e[i, i] = h
            dq = (logml(ref["M"][k] + e, ref["d"][k]) - logml(ref["M"][k] - e, ref["d"][k])) / (2 * h)
            assert abs(dq - ref["gradc"][k, i]) < 1e-8 * max(1.0, abs(dq))
