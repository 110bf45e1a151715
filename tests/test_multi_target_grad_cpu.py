"""CPU-side checks of the gradients of the multi-output GP log marginal likelihood (matinv_multi_target_grad_batched*): exports, argument
errors, dispatch names, the audit of the compiled forms that the generated instantiation sweep cannot make (the forms carry the names of
the SPD inversion kernels with nine more template arguments), the meaning of the reference (central finite differences of sum_t logml_t,
and the single-target gradient at D = 1), and the check that the bounds of tests/_multi_target_grad_worker.py hold for a float32 numpy
evaluation of the reference formulas. No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import _logml_grad_worker as LG
import _multi_target_grad_worker as MG
import _multi_target_worker as MT
import test_instantiations_cpu as audit
from conftest import pkg

NAMES = ["matinv_multi_target_grad_batched", "matinv_multi_target_grad_kernel_name", "matinv_multi_target_grad_batched_host"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_multi_target_grad_symbols_exported():
    lib = pkg("_lib")
    L = lib.lib()
    header = open(os.path.join(ROOT, "include", "matinv.h")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in lib.NATIVE_NAMES
        assert re.search(rf"\b{name}\(", header), name
    api = pkg("api")
    for name in ("multi_target_grad_batched", "multi_target_grad_batched_host", "multi_target_grad_kernel_name"):
        assert callable(getattr(api, name))
    assert L.matinv_abi_version() == 2


def test_multi_target_grad_argument_errors_without_device():
    """every rule of the contract in include/matinv.h, in the order of matinv_multi_target_batched"""
    lib = pkg("_lib")
    L = lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def dev(dtype=0, n=4, D=2, P=2, b=p, c=p, y=p, dm=p, g=p, gc=p, lm=p, al=p, batch=2):
        return L.matinv_multi_target_grad_batched(dtype, n, D, P, b, c, y, dm, g, gc, lm, al, batch, None, None)

    def host(dtype=0, n=4, D=2, P=2, b=p, c=p, y=p, dm=p, g=p, gc=p, lm=p, al=p, batch=2):
        return L.matinv_multi_target_grad_batched_host(dtype, n, D, P, b, c, y, dm, g, gc, lm, al, batch, None)

    none = dict(g=None, gc=None, lm=None, al=None)
    nothing = dict(b=None, c=None, y=None, dm=None, **none)
    for f in (dev, host):
        assert f(n=0) == lib.ERR_ARG
        assert b"n must be" in L.matinv_last_error()
        assert f(dtype=2) == lib.ERR_ARG
        assert f(b=None) == lib.ERR_ARG
        assert f(**none) == lib.ERR_ARG
        assert b"output" in L.matinv_last_error()
        # Y and D are needed for every output
        for one in ("g", "gc", "lm", "al"):
            only = dict(none, **{one: p})
            assert f(y=None, **only) == lib.ERR_ARG
            assert b"dYs" in L.matinv_last_error()
            assert f(D=0, **only) == lib.ERR_ARG
            assert b"ntarget" in L.matinv_last_error()
        # dM and P are needed with grad, and only with it
        assert f(dm=None) == lib.ERR_ARG
        assert b"dDMs" in L.matinv_last_error()
        assert f(P=0) == lib.ERR_ARG
        assert b"nparam" in L.matinv_last_error()
        assert f(P=-1, dm=None, g=None) == lib.ERR_ARG
        # the order of the other GP entry points: n before dtype, the counts before the pointers, the outputs before the limits
        assert f(n=0, dtype=2) == lib.ERR_ARG and b"n must be" in L.matinv_last_error()
        assert f(P=0, dm=None) == lib.ERR_ARG and b"nparam" in L.matinv_last_error()
        assert f(D=0, b=None) == lib.ERR_ARG and b"ntarget" in L.matinv_last_error()
        assert f(n=1025, **none) == lib.ERR_ARG and b"output" in L.matinv_last_error()
        # batch == 0 is a no-op even with NULL pointers; n and dtype are still checked
        assert f(batch=0, **nothing) == lib.OK
        assert f(batch=0, dtype=5, **nothing) == lib.ERR_ARG
        assert f(batch=0, n=0, **nothing) == lib.ERR_ARG
        # n, D and P = 1025 are refused after the pointer checks
        assert f(batch=1, n=1025) == lib.ERR_UNSUPPORTED
        assert f(batch=1, n=1025, b=None) == lib.ERR_ARG
        assert f(batch=1, n=1025, P=0, dm=None, **dict(none, gc=p)) == lib.ERR_UNSUPPORTED
        assert f(batch=1, D=1025) == lib.ERR_UNSUPPORTED
        assert b"ntarget" in L.matinv_last_error()
        assert f(batch=1, P=1025) == lib.ERR_UNSUPPORTED
        assert b"nparam" in L.matinv_last_error()
        assert f(batch=0x80000000) == lib.ERR_ARG
        assert b"batch" in L.matinv_last_error()


def test_api_argument_validation():
    """api.multi_target_grad_batched refuses what it can see before the library is called"""
    torch = pytest.importorskip("torch")
    api = pkg("api")
    n = 4
    B = torch.eye(n, dtype=torch.float64).reshape(-1).repeat(2)
    Y = torch.zeros(2 * 3 * n, dtype=torch.float64)
    dM = torch.zeros(2 * 2 * n * n, dtype=torch.float64)
    with pytest.raises(ValueError):  # CPU tensors
        api.multi_target_grad_batched(n, B, None, Y, dM)
    if torch.cuda.is_available():
        B, Y, dM = B.cuda(), Y.cuda(), dM.cuda()
        with pytest.raises(ValueError, match="want holds"):
            api.multi_target_grad_batched(n, B, None, Y, dM, want=("grad", "quad"))
        with pytest.raises(ValueError, match="no output"):
            api.multi_target_grad_batched(n, B, None, Y, dM, want=())
        with pytest.raises(ValueError, match="needs the targets"):
            api.multi_target_grad_batched(n, B, None, None, dM, want=("gradc",))
        with pytest.raises(ValueError, match="grad needs"):
            api.multi_target_grad_batched(n, B, None, Y, None)
        with pytest.raises(ValueError, match="Ys needs"):
            api.multi_target_grad_batched(n, B, None, Y[:n], dM, want=("alpha",))
        with pytest.raises(ValueError, match="dMs needs"):
            api.multi_target_grad_batched(n, B, None, Y, dM[:n * n])
        with pytest.raises(TypeError):
            api.multi_target_grad_batched(n, B, None, Y.float(), dM)
        with pytest.raises(ValueError, match="Cs needs"):
            api.multi_target_grad_batched(n, B, Y[:n], Y, dM)
        with pytest.raises(ValueError, match="info"):
            api.multi_target_grad_batched(n, B, None, Y, dM, info=torch.zeros(2, dtype=torch.int64, device="cuda"))
    # the host form validates before it needs a device
    Bn, Yn, dMn = np.tile(np.eye(n).reshape(-1), 2), np.zeros(2 * 3 * n), np.zeros(2 * 2 * n * n)
    with pytest.raises(ValueError, match="want must name"):
        api.multi_target_grad_batched_host(n, Bn, None, Yn, dMn, want=())
    with pytest.raises(ValueError, match="want must name"):
        api.multi_target_grad_batched_host(n, Bn, None, Yn, dMn, want=("quad",))
    with pytest.raises(ValueError, match="needs the targets"):
        api.multi_target_grad_batched_host(n, Bn, None, None, dMn, want=("logml",))
    with pytest.raises(ValueError, match="grad needs"):
        api.multi_target_grad_batched_host(n, Bn, None, Yn, None, want=("grad",))
    with pytest.raises(ValueError, match="Ys needs"):
        api.multi_target_grad_batched_host(n, Bn, None, Yn[:n], dMn, want=("alpha",))
    with pytest.raises(TypeError):
        api.multi_target_grad_batched_host(n, Bn, None, Yn.astype(np.float32), dMn)
    with pytest.raises(ValueError, match="Cs smaller"):
        api.multi_target_grad_batched_host(n, Bn, Yn[:n], Yn, dMn)


@pytest.mark.parametrize("f64", [True, False])
def test_multi_target_grad_dispatch_names(f64):
    api = pkg("api")
    dt, t, c = (api.F64, "f64", "double") if f64 else (api.F32, "f32", "float")
    nine = "true, true, true, true, true, true, true, true, true"
    assert api.multi_target_grad_kernel_name(dt, 1) == f"matinv_spd_tile_{t}<1, false, {nine}>"
    assert api.multi_target_grad_kernel_name(dt, 16) == f"matinv_spd_tile_{t}<1, true, {nine}>"
    assert api.multi_target_grad_kernel_name(dt, 17) == f"matinv_spd_tile_{t}<2, false, {nine}>"
    assert api.multi_target_grad_kernel_name(dt, 96) == f"matinv_spd_tile_{t}<6, true, {nine}>"
    assert api.multi_target_grad_kernel_name(dt, 97) == f"matinv_chol_global<{c}, {nine}>"
    assert api.multi_target_grad_kernel_name(dt, 1024) == f"matinv_chol_global<{c}, {nine}>"
    assert api.multi_target_grad_kernel_name(dt, 0) == "" == api.multi_target_grad_kernel_name(dt, 1025)
    assert api.multi_target_grad_kernel_name(9, 32) == "" == api.multi_target_grad_kernel_name(-1, 200)
    assert api.multi_target_grad_kernel_name(np.float64 if f64 else np.float32, 33) == api.multi_target_grad_kernel_name(dt, 33)


def test_host_form_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    api = pkg("api")
    lib = pkg("_lib")
    B = np.eye(20).reshape(-1)
    y = np.ones(3 * 20)
    calls = (lambda: api.multi_target_grad_batched_host(20, B, np.ones(20), y, np.ones(2 * 400)),
             lambda: api.multi_target_grad_batched_host(20, B, None, y, None),
             lambda: api.multi_target_grad_batched_host(20, B, None, y, None, want=("gradc",)))
    for call in calls:
        with pytest.raises(lib.MatinvError) as err:
            call()
        assert err.value.code in (lib.ERR_NO_DEVICE, lib.ERR_HIP)
        assert lib.lib().matinv_last_error()


MULTI_TARGET_GRAD_FORMS = (r"matinv_spd_tile_f(64|32)<\d+, (true|false), true, true, true, true, true, true, true, true, true>",
                           r"matinv_chol_global<(double|float), true, true, true, true, true, true, true, true, true>")


@pytest.mark.skipif(audit.NM is None, reason="no nm on this machine")
def test_every_gradient_name_is_a_compiled_kernel_and_every_gradient_form_is_named():
    """what test_instantiations_cpu checks for the routes of the generated sweep, for the multi-target gradient forms: exact names, both
    directions"""
    api = pkg("api")
    named = {api.multi_target_grad_kernel_name(dt, n) for dt in (api.F64, api.F32) for n in range(1, 1025)}
    assert "" not in named and len(named) == 2 * (12 + 1)
    assert all(any(re.fullmatch(p, s) for p in MULTI_TARGET_GRAD_FORMS) for s in named)
    missing = sorted(named - audit.STUBS)
    assert not missing, f"named by matinv_multi_target_grad_kernel_name but not compiled: {missing}"
    compiled = {s for s in audit.STUBS if any(re.fullmatch(p, s) for p in MULTI_TARGET_GRAD_FORMS)}
    assert compiled, "no multi-target gradient form is compiled"
    assert not sorted(compiled - named), f"compiled multi-target gradient forms no n reaches: {sorted(compiled - named)}"
    # the inverse's route names claim the new forms by the prefix rule of test_instantiations_cpu
    for s in named:
        base = re.sub(r"(, true){9}>$", ">", s)
        assert audit.matches(base, s), (base, s)
    # the eight earlier audits do not take a gradient form for one of theirs, nor the reverse
    import test_colour_cpu
    import test_logml_grad_cpu
    import test_loo_cpu
    import test_loo_grad_cpu
    import test_multi_target_cpu
    import test_predict_cov_cpu
    import test_predict_cpu
    import test_whiten_cpu
    others = test_loo_cpu.LOO_FORMS + test_logml_grad_cpu.GRAD_FORMS + test_predict_cpu.PREDICT_FORMS + \
        test_predict_cov_cpu.PREDICT_COV_FORMS + test_loo_grad_cpu.LOO_GRAD_FORMS + test_colour_cpu.COLOUR_FORMS + \
        test_whiten_cpu.WHITEN_FORMS + test_multi_target_cpu.MULTI_TARGET_FORMS
    assert not any(re.fullmatch(p, s) for p in others for s in named)
    theirs = {s for s in audit.STUBS if any(re.fullmatch(p, s) for p in others)}
    assert theirs and not any(re.fullmatch(p, s) for p in MULTI_TARGET_GRAD_FORMS for s in theirs)


@pytest.mark.parametrize("n", [5, 17])
def test_reference_is_the_gradient_of_the_reference_sum_of_logml(n):
    """central finite differences of sum_t logml_t in float64, D = 3, P = 2: M +- h dM_p for grad, c_i +- h for gradc; h = 1e-5, relative
    agreement 1e-6"""
    D, P, h = 3, 2, 1e-5
    B, c, Ys, dMs, full = MG.case(n, "float64", True)
    ref = MG.take(full, dMs, n, D, P)
    M, y, dM = ref["M"], ref["y"], ref["dM"]
    for k in range(M.shape[0]):
        scale = max(1.0, np.abs(ref["grad"][k]).max(), np.abs(ref["gradc"][k]).max())
        for p in range(P):
            fd = (MG.sum_logml(M[k] + h * dM[k, p], y[k]) - MG.sum_logml(M[k] - h * dM[k, p], y[k])) / (2 * h)
            assert abs(fd - ref["grad"][k, p]) <= 1e-6 * scale, (n, k, p, fd, ref["grad"][k, p])
        for i in range(n):
            e = np.zeros((n, n))
            e[i, i] = h
            fd = (MG.sum_logml(M[k] + e, y[k]) - MG.sum_logml(M[k] - e, y[k])) / (2 * h)
            assert abs(fd - ref["gradc"][k, i]) <= 1e-6 * scale, (n, k, i, fd, ref["gradc"][k, i])
        # sum_logml is the sum of the reference logml
        direct = MG.sum_logml(M[k], y[k])
        assert abs(direct - float(ref["logml"][k].sum())) <= 1e-10 * max(1.0, abs(direct))


@pytest.mark.parametrize("n", [1, 16, 17, 97])
def test_one_target_is_the_single_target_gradient(n):
    """D = 1: grad, gradc and alpha are those of _logml_grad_worker.reference"""
    B, c, Ys, dMs, full = MG.case(n, "float64", True)
    ref = MG.take(full, dMs, n, 1, MG.PMAX)
    one = LG.reference(B, c, MG.first(Ys, n, MG.DMAX, 1), dMs, n, MG.PMAX)
    for k, got, want in (("grad", ref["grad"], one["grad"]), ("gradc", ref["gradc"], one["gradc"]), ("alpha", ref["alpha"][:, 0], one["alpha"]),
                         ("G", ref["G"], one["G"])):
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (n, k)


@pytest.mark.parametrize("n", MG.TILE_SIZES + MG.GLOBAL_SIZES + [1024])
def test_float32_numpy_stays_inside_the_fp32_bounds(n):
    """the bounds are derived, not fitted: a float32 numpy evaluation of the reference formulas must pass them at every size and (D, P)
    the GPU tests use, with and without c, before they are held against the kernels"""
    u = MG.U[np.dtype(np.float32)]
    for with_c in (True, False) if n < 1024 else (True,):
        B, c, Ys, dMs, full = MG.case(n, "float32", with_c)
        for D, P in (MG.DP if n < 1024 else (MG.DP_1024,)):
            y, dm = MG.first(Ys, n, MG.DMAX, D), MG.first_derivs(dMs, n, MG.PMAX, P)
            MG.check(MG.float32_evaluation(B, c, y, dm, n, D, P), MG.take(full, dMs, n, D, P), n, u, what="float32 numpy")


def test_bounds_fail_a_wrong_result():
    """a grad wrong by one part in a thousand, the gradc of the wrong element and a grad with K counted once, not D times, fail"""
    n, D, P = 17, 3, 2
    B, c, Ys, dMs, full = MG.case(n, "float64", True)
    ref = MG.take(full, dMs, n, D, P)
    u = MG.U[np.dtype(np.float64)]
    once = 0.5 * np.einsum("kij,kpij->kp", ref["G"] + (D - 1) * ref["K"], ref["dM"])
    for wrong in (dict(grad=ref["grad"] * 1.001), dict(gradc=np.roll(ref["gradc"], 1, axis=1)), dict(grad=once)):
        with pytest.raises(AssertionError):
            MG.check(wrong, ref, n, u, what="wrong on purpose")
