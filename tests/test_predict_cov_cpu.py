"""CPU-side checks of the joint predictive covariance between a GP's query points (matinv_predict_cov_batched*): exports, argument errors,
dispatch names, the audit of the compiled covariance kernel forms that the generated instantiation sweep cannot make (the forms carry the
names of the SPD inversion kernels with four more template arguments), the check that the bounds of tests/_predict_cov_worker.py hold for a
float32 numpy evaluation of the reference formulas, and the meaning of the reference itself. No GPU needed."""
import ctypes
import re

import numpy as np
import pytest

import _predict_cov_worker as W
import test_instantiations_cpu as audit
from conftest import pkg

NAMES = ["matinv_predict_cov_batched", "matinv_predict_cov_kernel_name", "matinv_predict_cov_batched_host"]


def test_predict_cov_symbols_exported():
    lib = pkg("_lib")
    L = lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in lib.NATIVE_NAMES
    assert L.matinv_abi_version() == 2
    api = pkg("api")
    for name in ("predict_cov_batched", "predict_cov_batched_host", "predict_cov_kernel_name"):
        assert callable(getattr(api, name))


def test_predict_cov_argument_errors_without_device():
    lib = pkg("_lib")
    L = lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def dev(dtype=0, n=4, nquery=2, b=p, c=p, d=p, a=p, e=p, mean=p, cov=p, batch=2):
        return L.matinv_predict_cov_batched(dtype, n, nquery, b, c, d, a, e, mean, cov, batch, None, None)

    def host(dtype=0, n=4, nquery=2, b=p, c=p, d=p, a=p, e=p, mean=p, cov=p, batch=2):
        return L.matinv_predict_cov_batched_host(dtype, n, nquery, b, c, d, a, e, mean, cov, batch, None)

    nothing = dict(b=None, c=None, d=None, a=None, e=None, mean=None, cov=None)
    for f in (dev, host):
        assert f(n=0) == lib.ERR_ARG
        assert b"n must be" in L.matinv_last_error()
        assert f(n=-2) == lib.ERR_ARG
        assert f(dtype=2) == lib.ERR_ARG
        assert f(b=None) == lib.ERR_ARG
        assert f(a=None) == lib.ERR_ARG
        assert f(mean=None, cov=None) == lib.ERR_ARG
        assert b"output" in L.matinv_last_error()
        assert f(nquery=0) == lib.ERR_ARG
        assert b"nquery" in L.matinv_last_error()
        assert f(nquery=-3) == lib.ERR_ARG
        # d is needed with mean, and only with it
        assert f(d=None) == lib.ERR_ARG
        assert b"dDs" in L.matinv_last_error()
        # batch == 0 is a no-op even with NULL pointers and nquery = 0; n and dtype are still checked
        assert f(batch=0, **nothing) == lib.OK
        assert f(batch=0, nquery=0, **nothing) == lib.OK
        assert f(batch=0, nquery=5000, **nothing) == lib.OK
        assert f(batch=0, dtype=5, **nothing) == lib.ERR_ARG
        assert f(batch=0, n=0, **nothing) == lib.ERR_ARG
        # n = 2000 and nquery = 1025 are refused after the pointer checks: either output alone passes them, so do a NULL c, a NULL e
        # and, without mean, a NULL d
        for big in (dict(n=2000), dict(nquery=1025)):
            assert f(batch=1, **big) == lib.ERR_UNSUPPORTED
            assert f(batch=1, mean=None, **big) == lib.ERR_UNSUPPORTED
            assert f(batch=1, cov=None, **big) == lib.ERR_UNSUPPORTED
            assert f(batch=1, mean=None, d=None, **big) == lib.ERR_UNSUPPORTED
            assert f(batch=1, c=None, e=None, **big) == lib.ERR_UNSUPPORTED
            assert f(batch=1, mean=None, cov=None, **big) == lib.ERR_ARG
            assert f(batch=1, a=None, **big) == lib.ERR_ARG
            assert f(batch=1, d=None, **big) == lib.ERR_ARG
            assert f(batch=0x80000000, **big) == lib.ERR_ARG
        assert f(n=2000, batch=1, nquery=0) == lib.ERR_ARG
        assert f(nquery=1025, batch=1) == lib.ERR_UNSUPPORTED
        assert b"nquery" in L.matinv_last_error()
        assert f(batch=0x80000000) == lib.ERR_ARG
        assert b"batch" in L.matinv_last_error()


@pytest.mark.parametrize("f64", [True, False])
def test_predict_cov_dispatch_names(f64):
    api = pkg("api")
    dt, t, c = (api.F64, "f64", "double") if f64 else (api.F32, "f32", "float")
    assert api.predict_cov_kernel_name(dt, 1) == f"matinv_spd_tile_{t}<1, false, true, true, true, true>"
    assert api.predict_cov_kernel_name(dt, 15) == f"matinv_spd_tile_{t}<1, false, true, true, true, true>"
    assert api.predict_cov_kernel_name(dt, 16) == f"matinv_spd_tile_{t}<1, true, true, true, true, true>"
    assert api.predict_cov_kernel_name(dt, 17) == f"matinv_spd_tile_{t}<2, false, true, true, true, true>"
    assert api.predict_cov_kernel_name(dt, 96) == f"matinv_spd_tile_{t}<6, true, true, true, true, true>"
    assert api.predict_cov_kernel_name(dt, 97) == f"matinv_chol_global<{c}, true, true, true, true>"
    assert api.predict_cov_kernel_name(dt, 1024) == f"matinv_chol_global<{c}, true, true, true, true>"
    assert api.predict_cov_kernel_name(dt, 0) == "" == api.predict_cov_kernel_name(dt, 1025)
    assert api.predict_cov_kernel_name(9, 32) == "" == api.predict_cov_kernel_name(-1, 200)


def test_predict_cov_host_form_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    api = pkg("api")
    lib = pkg("_lib")
    b = np.eye(20).reshape(-1)
    d = np.ones(20)
    a = np.ones(3 * 20)
    calls = (lambda: api.predict_cov_batched_host(20, b, d, d, a, np.eye(3).reshape(-1)),
             lambda: api.predict_cov_batched_host(20, b, None, None, a, None, want=("cov",)))
    for call in calls:
        with pytest.raises(lib.MatinvError) as e:
            call()
        assert e.value.code in (lib.ERR_NO_DEVICE, lib.ERR_HIP)
        assert lib.lib().matinv_last_error()


PREDICT_COV_FORMS = (r"matinv_spd_tile_f(64|32)<\d+, (true|false), true, true, true, true>",
                     r"matinv_chol_global<(double|float), true, true, true, true>")


@pytest.mark.skipif(audit.NM is None, reason="no nm on this machine")
def test_every_covariance_name_is_a_compiled_kernel_and_every_covariance_form_is_named():
    """what test_instantiations_cpu checks for the routes of the generated sweep, for the covariance forms: exact names, both directions"""
    api = pkg("api")
    named = {api.predict_cov_kernel_name(dt, n) for dt in (api.F64, api.F32) for n in range(1, 1025)}
    assert "" not in named and len(named) == 2 * (12 + 1)
    assert all(any(re.fullmatch(p, s) for p in PREDICT_COV_FORMS) for s in named)
    missing = sorted(named - audit.STUBS)
    assert not missing, f"named by matinv_predict_cov_kernel_name but not compiled: {missing}"
    compiled = {s for s in audit.STUBS if any(re.fullmatch(p, s) for p in PREDICT_COV_FORMS)}
    assert compiled, "no covariance form is compiled"
    assert not sorted(compiled - named), f"compiled covariance forms no n reaches: {sorted(compiled - named)}"
    # the audits of the LOO, the gradient and the prediction forms do not take a covariance form for one of theirs, nor the reverse
    import test_logml_grad_cpu
    import test_loo_cpu
    import test_predict_cpu
    others = test_loo_cpu.LOO_FORMS + test_logml_grad_cpu.GRAD_FORMS + test_predict_cpu.PREDICT_FORMS
    assert not any(re.fullmatch(p, s) for p in others for s in named)
    theirs = {s for s in audit.STUBS if any(re.fullmatch(p, s) for p in others)}
    assert theirs and not any(re.fullmatch(p, s) for p in PREDICT_COV_FORMS for s in theirs)


@pytest.mark.parametrize("n", W.TILE_SIZES + W.GLOBAL_SIZES + [1024])
def test_float32_numpy_stays_inside_the_fp32_bounds(n):
    """the bounds are derived, not fitted: a float32 numpy evaluation of the reference formulas (LAPACK inverse, einsum) must pass them
    at every size, Q and input the GPU accuracy test uses, before they are held against the kernels; and the inputs are what the worker
    says: the posterior covariance is a covariance"""
    dt = np.float32
    for with_c in (True, False):
        B, c, d, mdl, As, Es = W.case(n, "float32", with_c)
        for nquery in W.QS:
            a, e = W.leading(As, Es, n, nquery)
            ref = W.cov_reference(mdl, a, e, n, nquery)
            assert np.linalg.eigvalsh(ref["cov"]).min() > 0.09
            got = W.float32_evaluation(B, c, d, a, e, n, nquery)
            W.check(*got, ref, n, W.U[np.dtype(dt)], what=f"float32 numpy c={with_c}")


@pytest.mark.parametrize("n", [17, 130])
def test_float64_case_is_a_covariance(n):
    B, c, d, mdl, As, Es = W.case(n, "float64", True)
    ref = W.cov_reference(mdl, As, Es, n, W.QMAX)
    assert np.linalg.eigvalsh(ref["cov"]).min() > 0.09
    a, e = W.pick(As, Es, n, [0, 15, 16, 32])
    sub = W.cov_reference(mdl, a, e, n, 4)
    assert np.array_equal(sub["E"], ref["E"][:, [0, 15, 16, 32]][:, :, [0, 15, 16, 32]])


def test_reference_is_the_conditional_of_the_joint_gaussian():
    """the meaning, in numpy only: for the joint (n + Q)-dimensional Gaussian of (observations, latent values at the Q queries) with
    covariance J = [[M, A^T], [A, E]] (A the Q x n matrix of the a_i), the reference mean and cov are the conditional mean and covariance
    of the queries given the observations d -- the Schur complement of M, read off the inverse of the joint covariance:
    cov = inv(P_qq), mean = -cov P_qo d with P = inv(J)"""
    n, nquery = 6, 3
    B, c, d, mdl, As, Es = W.case(n, "float64", True)
    a, e = W.leading(As, Es, n, nquery)
    ref = W.cov_reference(mdl, a, e, n, nquery)
    dd = d.reshape(-1, n)
    for k in range(ref["M"].shape[0]):
        A = ref["a"][k]
        J = np.block([[ref["M"][k], A.T], [A, ref["E"][k]]])
        assert np.linalg.eigvalsh(J).min() > 0  # E was chosen above A K A^T: the joint covariance is a covariance
        P = np.linalg.inv(J)
        cov = np.linalg.inv(P[n:, n:])
        mean = -cov @ (P[n:, :n] @ dd[k])
        assert np.abs(cov - ref["cov"][k]).max() < 1e-10 * max(1.0, np.abs(cov).max())
        assert np.abs(mean - ref["mean"][k]).max() < 1e-10 * max(1.0, np.abs(mean).max())
