"""CPU-side checks of the multi-output GP solves (matinv_multi_target_batched*): exports, argument errors, dispatch names, the audit of the
compiled multi-target kernel forms that the generated instantiation sweep cannot make (the forms carry the names of the SPD inversion
kernels with eight more template arguments), the meaning of the reference, and the check that the bounds of tests/_multi_target_worker.py
hold for a float32 numpy evaluation of the reference formulas. No GPU needed."""
import ctypes
import re

import numpy as np
import pytest

import _multi_target_worker as MT
import test_instantiations_cpu as audit
from conftest import pkg

NAMES = ["matinv_multi_target_batched", "matinv_multi_target_kernel_name", "matinv_multi_target_batched_host"]


def test_multi_target_symbols_exported():
    lib = pkg("_lib")
    L = lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in lib.NATIVE_NAMES
    api = pkg("api")
    for name in ("multi_target_batched", "multi_target_batched_host", "multi_target_kernel_name"):
        assert callable(getattr(api, name))
    assert L.matinv_abi_version() == 2


def test_multi_target_argument_errors_without_device():
    """every rule of the contract in include/matinv.h, in the order of matinv_predict_batched"""
    lib = pkg("_lib")
    L = lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def dev(dtype=0, n=4, D=2, Q=2, b=p, c=p, y=p, a=p, al=p, qd=p, ld=p, lm=p, mn=p, batch=2):
        return L.matinv_multi_target_batched(dtype, n, D, Q, b, c, y, a, al, qd, ld, lm, mn, batch, None, None)

    def host(dtype=0, n=4, D=2, Q=2, b=p, c=p, y=p, a=p, al=p, qd=p, ld=p, lm=p, mn=p, batch=2):
        return L.matinv_multi_target_batched_host(dtype, n, D, Q, b, c, y, a, al, qd, ld, lm, mn, batch, None)

    none = dict(al=None, qd=None, ld=None, lm=None, mn=None)
    nothing = dict(b=None, c=None, y=None, a=None, **none)
    for f in (dev, host):
        assert f(n=0) == lib.ERR_ARG
        assert b"n must be" in L.matinv_last_error()
        assert f(dtype=2) == lib.ERR_ARG
        assert f(b=None) == lib.ERR_ARG
        assert f(**none) == lib.ERR_ARG
        assert b"output" in L.matinv_last_error()
        # Y and D are needed for every output but logdet, and only for them
        for one in ("al", "qd", "lm", "mn"):
            only = dict(none, **{one: p})
            assert f(y=None, **only) == lib.ERR_ARG
            assert b"dYs" in L.matinv_last_error()
            assert f(D=0, **only) == lib.ERR_ARG
            assert b"ntarget" in L.matinv_last_error()
        # A and Q are needed with mean, and only with it
        assert f(a=None) == lib.ERR_ARG
        assert b"dAs" in L.matinv_last_error()
        assert f(Q=0) == lib.ERR_ARG
        assert b"nquery" in L.matinv_last_error()
        # the order of the other GP entry points: n before dtype, the counts before the pointers, the outputs before the limits
        assert f(n=0, dtype=2) == lib.ERR_ARG and b"n must be" in L.matinv_last_error()
        assert f(Q=0, a=None) == lib.ERR_ARG and b"nquery" in L.matinv_last_error()
        assert f(n=1025, **none) == lib.ERR_ARG and b"output" in L.matinv_last_error()
        # batch == 0 is a no-op even with NULL pointers; n and dtype are still checked
        assert f(batch=0, **nothing) == lib.OK
        assert f(batch=0, dtype=5, **nothing) == lib.ERR_ARG
        assert f(batch=0, n=0, **nothing) == lib.ERR_ARG
        # n, D and Q = 1025 are refused after the pointer checks
        assert f(batch=1, n=1025) == lib.ERR_UNSUPPORTED
        assert f(batch=1, n=1025, b=None) == lib.ERR_ARG
        assert f(batch=1, n=1025, D=0, Q=0, y=None, a=None, **dict(none, ld=p)) == lib.ERR_UNSUPPORTED
        assert f(batch=1, D=1025) == lib.ERR_UNSUPPORTED
        assert b"ntarget" in L.matinv_last_error()
        assert f(batch=1, Q=1025) == lib.ERR_UNSUPPORTED
        assert b"nquery" in L.matinv_last_error()
        assert f(batch=0x80000000) == lib.ERR_ARG
        assert b"batch" in L.matinv_last_error()


def test_api_argument_validation():
    """api.multi_target_batched refuses what it can see before the library is called"""
    torch = pytest.importorskip("torch")
    api = pkg("api")
    n = 4
    B = torch.eye(n, dtype=torch.float64).reshape(-1).repeat(2)
    Y = torch.zeros(2 * 3 * n, dtype=torch.float64)
    with pytest.raises(ValueError):  # CPU tensors
        api.multi_target_batched(n, B, None, Y)
    if torch.cuda.is_available():
        B, Y = B.cuda(), Y.cuda()
        with pytest.raises(ValueError, match="want holds"):
            api.multi_target_batched(n, B, None, Y, want=("alpha", "var"))
        with pytest.raises(ValueError, match="no output"):
            api.multi_target_batched(n, B, None, Y, want=())
        with pytest.raises(ValueError, match="need the targets"):
            api.multi_target_batched(n, B, None, None, want=("quad",))
        with pytest.raises(ValueError, match="mean needs"):
            api.multi_target_batched(n, B, None, Y, want=("mean",))
        with pytest.raises(ValueError, match="Ys needs"):
            api.multi_target_batched(n, B, None, Y[:n], want=("alpha",))
        with pytest.raises(TypeError):
            api.multi_target_batched(n, B, None, Y.float())
        with pytest.raises(ValueError, match="Cs needs"):
            api.multi_target_batched(n, B, Y[:n], Y)
        with pytest.raises(ValueError, match="info"):
            api.multi_target_batched(n, B, None, Y, info=torch.zeros(2, dtype=torch.int64, device="cuda"))
    # the host form validates before it needs a device
    Bn, Yn = np.tile(np.eye(n).reshape(-1), 2), np.zeros(2 * 3 * n)
    with pytest.raises(ValueError, match="want must name"):
        api.multi_target_batched_host(n, Bn, None, Yn, want=())
    with pytest.raises(ValueError, match="want must name"):
        api.multi_target_batched_host(n, Bn, None, Yn, want=("var",))
    with pytest.raises(ValueError, match="need the targets"):
        api.multi_target_batched_host(n, Bn, None, None, want=("logml",))
    with pytest.raises(ValueError, match="mean needs"):
        api.multi_target_batched_host(n, Bn, None, Yn, want=("mean",))
    with pytest.raises(ValueError, match="Ys needs"):
        api.multi_target_batched_host(n, Bn, None, Yn[:n], want=("alpha",))
    with pytest.raises(TypeError):
        api.multi_target_batched_host(n, Bn, None, Yn.astype(np.float32))
    with pytest.raises(ValueError, match="Cs smaller"):
        api.multi_target_batched_host(n, Bn, Yn[:n], Yn)


@pytest.mark.parametrize("f64", [True, False])
def test_multi_target_dispatch_names(f64):
    api = pkg("api")
    dt, t, c = (api.F64, "f64", "double") if f64 else (api.F32, "f32", "float")
    eight = "true, true, true, true, true, true, true, true"
    assert api.multi_target_kernel_name(dt, 1) == f"matinv_spd_tile_{t}<1, false, {eight}>"
    assert api.multi_target_kernel_name(dt, 15) == f"matinv_spd_tile_{t}<1, false, {eight}>"
    assert api.multi_target_kernel_name(dt, 16) == f"matinv_spd_tile_{t}<1, true, {eight}>"
    assert api.multi_target_kernel_name(dt, 17) == f"matinv_spd_tile_{t}<2, false, {eight}>"
    assert api.multi_target_kernel_name(dt, 96) == f"matinv_spd_tile_{t}<6, true, {eight}>"
    assert api.multi_target_kernel_name(dt, 97) == f"matinv_chol_global<{c}, {eight}>"
    assert api.multi_target_kernel_name(dt, 1024) == f"matinv_chol_global<{c}, {eight}>"
    assert api.multi_target_kernel_name(dt, 0) == "" == api.multi_target_kernel_name(dt, 1025)
    assert api.multi_target_kernel_name(9, 32) == "" == api.multi_target_kernel_name(-1, 200)
    assert api.multi_target_kernel_name(np.float64 if f64 else np.float32, 33) == api.multi_target_kernel_name(dt, 33)


def test_host_form_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    api = pkg("api")
    lib = pkg("_lib")
    B = np.eye(20).reshape(-1)
    y = np.ones(3 * 20)
    calls = (lambda: api.multi_target_batched_host(20, B, np.ones(20), y, y),
             lambda: api.multi_target_batched_host(20, B, None, y),
             lambda: api.multi_target_batched_host(20, B, None, None, want=("logdet",)))
    for call in calls:
        with pytest.raises(lib.MatinvError) as err:
            call()
        assert err.value.code in (lib.ERR_NO_DEVICE, lib.ERR_HIP)
        assert lib.lib().matinv_last_error()


MULTI_TARGET_FORMS = (r"matinv_spd_tile_f(64|32)<\d+, (true|false), true, true, true, true, true, true, true, true>",
                      r"matinv_chol_global<(double|float), true, true, true, true, true, true, true, true>")


@pytest.mark.skipif(audit.NM is None, reason="no nm on this machine")
def test_every_multi_target_name_is_a_compiled_kernel_and_every_multi_target_form_is_named():
    """what test_instantiations_cpu checks for the routes of the generated sweep, for the multi-target forms: exact names, both directions"""
    api = pkg("api")
    named = {api.multi_target_kernel_name(dt, n) for dt in (api.F64, api.F32) for n in range(1, 1025)}
    assert "" not in named and len(named) == 2 * (12 + 1)
    assert all(any(re.fullmatch(p, s) for p in MULTI_TARGET_FORMS) for s in named)
    missing = sorted(named - audit.STUBS)
    assert not missing, f"named by matinv_multi_target_kernel_name but not compiled: {missing}"
    compiled = {s for s in audit.STUBS if any(re.fullmatch(p, s) for p in MULTI_TARGET_FORMS)}
    assert compiled, "no multi-target form is compiled"
    assert not sorted(compiled - named), f"compiled multi-target forms no n reaches: {sorted(compiled - named)}"
    # the seven earlier audits do not take a multi-target form for one of theirs, nor the reverse
    import test_colour_cpu
    import test_logml_grad_cpu
    import test_loo_cpu
    import test_loo_grad_cpu
    import test_predict_cov_cpu
    import test_predict_cpu
    import test_whiten_cpu
    others = test_loo_cpu.LOO_FORMS + test_logml_grad_cpu.GRAD_FORMS + test_predict_cpu.PREDICT_FORMS + \
        test_predict_cov_cpu.PREDICT_COV_FORMS + test_loo_grad_cpu.LOO_GRAD_FORMS + test_colour_cpu.COLOUR_FORMS + \
        test_whiten_cpu.WHITEN_FORMS
    assert not any(re.fullmatch(p, s) for p in others for s in named)
    theirs = {s for s in audit.STUBS if any(re.fullmatch(p, s) for p in others)}
    assert theirs and not any(re.fullmatch(p, s) for p in MULTI_TARGET_FORMS for s in theirs)


@pytest.mark.parametrize("n", [1, 16, 17, 97])
def test_reference_is_the_gaussian_log_density_and_the_conditional_mean(n):
    """D = 1: logml is the log-density of N(0, M) at y from slogdet and solve, and mean is the conditional mean of the joint Gaussian
    [y; f] ~ N(0, [[M, A^T], [A, E]]): E[f | y] = A M^-1 y, whatever E"""
    B, c, Ys, As, full = MT.case(n, "float64", True)
    ref = MT.take(full, 1, MT.QMAX)
    M, y, a = ref["M"], ref["y"][:, 0], ref["a"]
    sol = np.linalg.solve(M, y[:, :, None])[:, :, 0]
    assert np.abs(ref["alpha"][:, 0] - sol).max() < 1e-12 * max(1.0, np.abs(sol).max())
    assert np.abs(np.einsum("kij,kj->ki", M, ref["alpha"][:, 0]) - y).max() < 1e-12 * max(1.0, np.abs(y).max())
    sign, logdet = np.linalg.slogdet(M)
    assert (sign == 1).all()
    assert np.abs(ref["logdet"].astype(np.float64) - logdet).max() < 1e-12 * max(1.0, np.abs(logdet).max())
    quad = (y * sol).sum(axis=1)
    direct = -0.5 * (quad + logdet + n * np.log(2 * np.pi))
    assert np.abs(ref["logml"][:, 0].astype(np.float64) - direct).max() < 1e-12 * max(1.0, np.abs(direct).max())
    assert np.abs(ref["quad"][:, 0] - quad).max() < 1e-12 * max(1.0, quad.max())
    # the conditional mean of the joint Gaussian by its precision matrix: with J = inv([[M, A^T], [A, E]]), E[f | y] = -J_ff^-1 J_fy y
    Q = a.shape[1]
    for k in range(min(3, M.shape[0])):
        E = a[k] @ np.linalg.solve(M[k], a[k].T) + np.eye(Q)  # any E that keeps the joint covariance SPD
        J = np.linalg.inv(np.block([[M[k], a[k].T], [a[k], E]]))
        cond_mean = -np.linalg.solve(J[n:, n:], J[n:, :n] @ y[k])
        assert np.abs(ref["mean"][k, 0] - cond_mean).max() < 1e-9 * max(1.0, np.abs(cond_mean).max())
    # the slices of the shared reference are the reference of the sliced inputs
    part = MT.reference(MT.model(B, c, n), MT.first(Ys, n, MT.DMAX, 16), MT.first(As, n, MT.QMAX, 17), n, 16, 17)
    took = MT.take(full, 16, 17)
    for k in ("alpha", "quad", "logml", "mean"):
        assert np.array_equal(np.asarray(part[k], dtype=np.float64), np.asarray(took[k], dtype=np.float64)), k


@pytest.mark.parametrize("n", MT.TILE_SIZES + MT.GLOBAL_SIZES + [1024])
def test_float32_numpy_stays_inside_the_fp32_bounds(n):
    """the bounds are derived, not fitted: a float32 numpy evaluation of the reference formulas must pass them at every size and (D, Q)
    the GPU tests use, with and without c, before they are held against the kernels"""
    u = MT.U[np.dtype(np.float32)]
    for with_c in (True, False) if n < 1024 else (True,):
        B, c, Ys, As, full = MT.case(n, "float32", with_c)
        for D, Q in (MT.DQ + ((33, 0),) if n < 1024 else (MT.DQ_1024,)):
            y, a = MT.first(Ys, n, MT.DMAX, D), MT.first(As, n, MT.QMAX, Q) if Q else None
            MT.check(MT.float32_evaluation(B, c, y, a, n, D, Q), MT.take(full, D, Q), n, u, what="float32 numpy")


def test_bounds_fail_a_wrong_result():
    """an alpha wrong by one part in a thousand, a mean of the wrong target and a logdet off by 1e-6 fail their bounds"""
    n = 17
    B, c, Ys, As, full = MT.case(n, "float64", True)
    u = MT.U[np.dtype(np.float64)]
    for wrong in (dict(alpha=full["alpha"] * 1.001), dict(mean=np.roll(full["mean"], 1, axis=1)),
                  dict(logdet=full["logdet"].astype(np.float64) + 1e-6)):
        with pytest.raises(AssertionError):
            MT.check(wrong, full, n, u, what="wrong on purpose")
