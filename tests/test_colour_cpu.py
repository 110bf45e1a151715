"""CPU-side checks of the batched Cholesky factor / coloured samples (matinv_colour_batched*) and of the joint posterior samples
(matinv_sample_batched*): exports, argument errors, dispatch names, the audit of the compiled colour kernel forms that the generated
instantiation sweep cannot make (the forms carry the names of the SPD inversion kernels with six more template arguments), the meaning of the
references, the check that the bounds of tests/_colour_worker.py hold for a float32 numpy evaluation of the reference formulas, and the
not-positive-definite fixtures. No GPU needed."""
import ctypes
import re

import numpy as np
import pytest

import _colour_worker as W
import test_instantiations_cpu as audit
from conftest import pkg

NAMES = ["matinv_colour_batched", "matinv_colour_kernel_name", "matinv_colour_batched_host", "matinv_sample_batched",
         "matinv_sample_batched_host"]


def test_colour_symbols_exported():
    lib = pkg("_lib")
    L = lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in lib.NATIVE_NAMES
    api = pkg("api")
    for name in ("colour_batched", "colour_batched_host", "colour_kernel_name", "sample_batched", "sample_batched_host"):
        assert callable(getattr(api, name))


def test_colour_argument_errors_without_device():
    lib = pkg("_lib")
    L = lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def dev(dtype=0, q=4, nsample=2, c=p, stride=16, m=p, z=p, y=p, l=p, batch=2):
        return L.matinv_colour_batched(dtype, q, nsample, c, stride, m, z, y, l, batch, None, None)

    def host(dtype=0, q=4, nsample=2, c=p, stride=16, m=p, z=p, y=p, l=p, batch=2):
        return L.matinv_colour_batched_host(dtype, q, nsample, c, stride, m, z, y, l, batch, None)

    nothing = dict(c=None, m=None, z=None, y=None, l=None)
    for f in (dev, host):
        assert f(q=0) == lib.ERR_ARG
        assert b"q must be" in L.matinv_last_error()
        assert f(dtype=2) == lib.ERR_ARG
        assert f(c=None) == lib.ERR_ARG
        assert f(y=None, l=None) == lib.ERR_ARG
        assert b"output" in L.matinv_last_error()
        # Z and S are needed with Y, and only with it
        assert f(z=None) == lib.ERR_ARG
        assert b"dZ" in L.matinv_last_error()
        assert f(nsample=0) == lib.ERR_ARG
        assert b"nsample" in L.matinv_last_error()
        assert f(stride=15) == lib.ERR_ARG
        assert b"strideC" in L.matinv_last_error()
        # batch == 0 is a no-op even with NULL pointers; q and dtype are still checked
        assert f(batch=0, **nothing) == lib.OK
        assert f(batch=0, dtype=5, **nothing) == lib.ERR_ARG
        assert f(batch=0, q=0, **nothing) == lib.ERR_ARG
        # q = 1025 and S = 1025 are refused after the pointer checks
        big = 1025 * 1025
        assert f(batch=1, q=1025, stride=big) == lib.ERR_UNSUPPORTED
        assert f(batch=1, q=1025, stride=big, y=None, z=None, nsample=0) == lib.ERR_UNSUPPORTED
        assert f(batch=1, q=1025, stride=big, y=None, l=None) == lib.ERR_ARG
        assert f(batch=1, q=1025, stride=big, c=None) == lib.ERR_ARG
        assert f(batch=1, nsample=1025) == lib.ERR_UNSUPPORTED
        assert b"nsample" in L.matinv_last_error()
        assert f(batch=0x80000000) == lib.ERR_ARG
        assert b"batch" in L.matinv_last_error()


def test_sample_argument_errors_without_device():
    lib = pkg("_lib")
    L = lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def dev(dtype=0, n=4, nquery=2, nsample=2, b=p, c=p, d=p, a=p, e=p, z=p, y=p, mean=p, cov=p, batch=2):
        return L.matinv_sample_batched(dtype, n, nquery, nsample, b, c, d, a, e, z, y, mean, cov, batch, None, None)

    def host(dtype=0, n=4, nquery=2, nsample=2, b=p, c=p, d=p, a=p, e=p, z=p, y=p, mean=p, cov=p, batch=2):
        return L.matinv_sample_batched_host(dtype, n, nquery, nsample, b, c, d, a, e, z, y, mean, cov, batch, None)

    for f in (dev, host):
        assert f(n=0) == lib.ERR_ARG
        assert f(dtype=3) == lib.ERR_ARG
        assert f(nquery=0) == lib.ERR_ARG
        assert f(nsample=0) == lib.ERR_ARG
        for missing in ("b", "a", "z", "y"):
            assert f(**{missing: None}) == lib.ERR_ARG, missing
        # d = NULL is the zero-mean posterior, but then there is no mean to return
        assert f(d=None) == lib.ERR_ARG
        assert b"dDs" in L.matinv_last_error()
        assert f(batch=0, b=None, a=None, z=None, y=None) == lib.OK
        for big in (dict(n=1025), dict(nquery=1025), dict(nsample=1025)):
            assert f(batch=1, **big) == lib.ERR_UNSUPPORTED
            assert f(batch=1, mean=None, cov=None, d=None, c=None, e=None, **big) == lib.ERR_UNSUPPORTED
            assert f(batch=1, y=None, **big) == lib.ERR_ARG


@pytest.mark.parametrize("f64", [True, False])
def test_colour_dispatch_names(f64):
    api = pkg("api")
    dt, t, c = (api.F64, "f64", "double") if f64 else (api.F32, "f32", "float")
    six = "true, true, true, true, true, true"
    assert api.colour_kernel_name(dt, 1) == f"matinv_spd_tile_{t}<1, false, {six}>"
    assert api.colour_kernel_name(dt, 16) == f"matinv_spd_tile_{t}<1, true, {six}>"
    assert api.colour_kernel_name(dt, 17) == f"matinv_spd_tile_{t}<2, false, {six}>"
    assert api.colour_kernel_name(dt, 96) == f"matinv_spd_tile_{t}<6, true, {six}>"
    assert api.colour_kernel_name(dt, 97) == f"matinv_chol_global<{c}, {six}>"
    assert api.colour_kernel_name(dt, 1024) == f"matinv_chol_global<{c}, {six}>"
    assert api.colour_kernel_name(dt, 0) == "" == api.colour_kernel_name(dt, 1025)
    assert api.colour_kernel_name(9, 32) == "" == api.colour_kernel_name(-1, 200)


def test_host_forms_without_gpu_fail_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    api = pkg("api")
    lib = pkg("_lib")
    C = np.eye(20).reshape(-1)
    z = np.ones(3 * 20)
    B, a, e, zq = np.eye(20).reshape(-1), np.ones(3 * 20), np.eye(3).reshape(-1), np.ones(2 * 3)
    calls = (lambda: api.colour_batched_host(20, C, np.ones(20), z),
             lambda: api.colour_batched_host(20, C, None, None, want=("L",)),
             lambda: api.sample_batched_host(20, B, None, np.ones(20), a, e, zq, want=("Y", "mean", "cov")),
             lambda: api.sample_batched_host(20, B, None, None, a, e, zq))
    for call in calls:
        with pytest.raises(lib.MatinvError) as err:
            call()
        assert err.value.code in (lib.ERR_NO_DEVICE, lib.ERR_HIP)
        assert lib.lib().matinv_last_error()


COLOUR_FORMS = (r"matinv_spd_tile_f(64|32)<\d+, (true|false), true, true, true, true, true, true>",
                r"matinv_chol_global<(double|float), true, true, true, true, true, true>")


@pytest.mark.skipif(audit.NM is None, reason="no nm on this machine")
def test_every_colour_name_is_a_compiled_kernel_and_every_colour_form_is_named():
    """what test_instantiations_cpu checks for the routes of the generated sweep, for the colour forms: exact names, both directions"""
    api = pkg("api")
    named = {api.colour_kernel_name(dt, q) for dt in (api.F64, api.F32) for q in range(1, 1025)}
    assert "" not in named and len(named) == 2 * (12 + 1)
    assert all(any(re.fullmatch(p, s) for p in COLOUR_FORMS) for s in named)
    missing = sorted(named - audit.STUBS)
    assert not missing, f"named by matinv_colour_kernel_name but not compiled: {missing}"
    compiled = {s for s in audit.STUBS if any(re.fullmatch(p, s) for p in COLOUR_FORMS)}
    assert compiled, "no colour form is compiled"
    assert not sorted(compiled - named), f"compiled colour forms no q reaches: {sorted(compiled - named)}"
    # the five earlier audits do not take a colour form for one of theirs, nor the reverse
    import test_logml_grad_cpu
    import test_loo_cpu
    import test_loo_grad_cpu
    import test_predict_cov_cpu
    import test_predict_cpu
    others = test_loo_cpu.LOO_FORMS + test_logml_grad_cpu.GRAD_FORMS + test_predict_cpu.PREDICT_FORMS + \
        test_predict_cov_cpu.PREDICT_COV_FORMS + test_loo_grad_cpu.LOO_GRAD_FORMS
    assert not any(re.fullmatch(p, s) for p in others for s in named)
    theirs = {s for s in audit.STUBS if any(re.fullmatch(p, s) for p in others)}
    assert theirs and not any(re.fullmatch(p, s) for p in COLOUR_FORMS for s in theirs)


@pytest.mark.parametrize("q", [1, 16, 17, 97])
def test_reference_is_the_factor_and_colours_the_identity(q):
    C, m, _ = W.case(q, "float64", 5)
    Z = np.tile(np.eye(q).reshape(-1), 5)
    ref = W.reference(C, m, Z, q)
    L = ref["L"]
    assert np.array_equal(np.triu(L, 1), np.zeros_like(L)) and (np.diagonal(L, axis1=1, axis2=2) > 0).all()
    assert np.abs(L @ L.transpose(0, 2, 1) - ref["C"]).max() < 1e-13 * np.abs(ref["C"]).max()
    # Z = I: sample s is column s of L on top of m, i.e. Y[k, s, i] - m[k, i] = L[k, i, s]
    assert np.abs(ref["Y"] - ref["m"][:, None, :] - L.transpose(0, 2, 1)).max() < 1e-14
    assert 1 <= ref["kappa"].max() < 12


def test_sample_reference_is_the_conditional_of_the_joint_gaussian():
    """the construction of test_predict_cov_cpu, for the case the sample tests use: the reference cov and mean are the conditional covariance
    and mean of the queries given the observations, read off the inverse of the joint covariance J = [[M, A^T], [A, E]], and the samples
    Yh = mean + Lh z have exactly that covariance: Lh Lh^T = cov"""
    n, nquery = 16, 17
    B, c, d, As, Es, Z = W.sample_case(n, nquery, "float64")
    cref, ref = W.sample_reference(B, c, d, As, Es, Z, n, nquery)
    dd = d.reshape(-1, n)
    for k in range(W.SAMPLE_BATCH):
        A = cref["a"][k]
        J = np.block([[cref["M"][k], A.T], [A, cref["E"][k]]])
        assert np.linalg.eigvalsh(J).min() > 0
        Pj = np.linalg.inv(J)
        cov = np.linalg.inv(Pj[n:, n:])
        mean = -cov @ (Pj[n:, :n] @ dd[k])
        assert np.abs(cov - cref["cov"][k]).max() < 1e-10 * max(1.0, np.abs(cov).max())
        assert np.abs(mean - cref["mean"][k]).max() < 1e-10 * max(1.0, np.abs(mean).max())
        assert np.abs(ref["L"][k] @ ref["L"][k].T - cov).max() < 1e-10 * max(1.0, np.abs(cov).max())
        assert np.abs(ref["Y"][k] - mean - ref["z"][k] @ ref["L"][k].T).max() < 1e-12


@pytest.mark.parametrize("q", W.QSIZES + [1024])
def test_float32_numpy_stays_inside_the_fp32_bounds(q):
    """the bounds are derived, not fitted: a float32 numpy evaluation of the reference formulas (LAPACK factor, einsum) must pass them at
    every size the GPU tests use, before they are held against the kernels"""
    batch = 2 if q == 1024 else 20
    C, m, Z = W.case(q, "float32", batch)
    ref = W.reference(C, m, Z, q)
    L, Y = W.float32_evaluation(C, m, Z, q)
    u = W.U[np.dtype(np.float32)]
    W.check_factor(L, ref, q, u, what="float32 numpy")
    W.check_y(Y, ref, q, u, what="float32 numpy")


@pytest.mark.parametrize("q", [33, 97])
def test_not_positive_definite_fixtures_fail_at_the_stated_column(q):
    for dtname in ("float64", "float32"):
        C, _, _ = W.case(q, dtname, 4)
        assert [W.first_bad_pivot(c) for c in W.mats(C, q)] == [0] * 4
        for j in (1, 16, 17, q):
            broken = W.break_at(C, q, 2, j)
            assert broken.dtype == C.dtype
            assert [W.first_bad_pivot(c) for c in W.mats(broken, q)] == [0, 0, j, 0], (q, j)
            same = np.array_equal(broken.reshape(4, -1)[[0, 1, 3]], C.reshape(4, -1)[[0, 1, 3]])
            assert same and (broken != C).sum() == 1
