"""CPU-side checks of the gradients of the trend GP's restricted log marginal likelihood (matinv_trend_grad_batched*): exports, argument
errors, dispatch names, the audit of the compiled forms that the generated instantiation sweep cannot make (the forms carry the names of
the SPD inversion kernels with eleven more template arguments), the meaning of the reference (central finite differences of
_trend_worker's sum_t logml_t, and the projection G H = 0), and the checks that the bounds of tests/_trend_grad_worker.py hold for a
float32 numpy evaluation of the reference formulas and fail wrong results. No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import _trend_grad_worker as TG
import test_instantiations_cpu as audit
from conftest import pkg

NAMES = ["matinv_trend_grad_batched", "matinv_trend_grad_kernel_name", "matinv_trend_grad_batched_host"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trend_grad_symbols_exported_and_named_in_the_header():
    lib = pkg("_lib")
    L = lib.lib()
    header = open(os.path.join(ROOT, "include", "matinv.h")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in lib.NATIVE_NAMES
        assert re.search(rf"\b{name}\(", header), name
    api = pkg("api")
    for name in ("trend_grad_batched", "trend_grad_batched_host", "trend_grad_kernel_name"):
        assert callable(getattr(api, name))
    assert L.matinv_abi_version() == 2


def test_trend_grad_argument_errors_without_device():
    """every rule of the contract in include/matinv.h: the order of matinv_trend_batched, with the lines of the gradient family for
    nparam and dDMs; each refusal by return code and by a substring of matinv_last_error()"""
    lib = pkg("_lib")
    L = lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def dev(dtype=0, n=4, K=2, D=2, P=2, b=p, c=p, h=p, y=p, dm=p, g=p, gc=p, lm=p, al=p, be=p, batch=2):
        return L.matinv_trend_grad_batched(dtype, n, K, D, P, b, c, h, y, dm, g, gc, lm, al, be, batch, None, None)

    def host(dtype=0, n=4, K=2, D=2, P=2, b=p, c=p, h=p, y=p, dm=p, g=p, gc=p, lm=p, al=p, be=p, batch=2):
        return L.matinv_trend_grad_batched_host(dtype, n, K, D, P, b, c, h, y, dm, g, gc, lm, al, be, batch, None)

    def refused(rc, code, text):
        assert rc == code, (rc, code, text, L.matinv_last_error())
        assert text in L.matinv_last_error(), (text, L.matinv_last_error())

    none = dict(g=None, gc=None, lm=None, al=None, be=None)
    nothing = dict(b=None, c=None, h=None, y=None, dm=None, **none)
    for f in (dev, host):
        refused(f(n=0), lib.ERR_ARG, b"n must be")
        assert f(dtype=2) == lib.ERR_ARG
        # the basis count: checked with n and dtype, before the empty batch returns
        for K in (0, -1, 17):
            refused(f(K=K, n=32), lib.ERR_ARG, b"nbasis must be in 1 .. 16")
            refused(f(K=K, n=32, batch=0, **nothing), lib.ERR_ARG, b"nbasis must be in 1 .. 16")
        refused(f(K=5, n=4), lib.ERR_ARG, b"exceeds n=4")
        refused(f(K=5, n=4, batch=0, **nothing), lib.ERR_ARG, b"exceeds n=4")
        # D: every output needs the targets
        refused(f(D=0), lib.ERR_ARG, b"ntarget must be >= 1")
        refused(f(D=1025, batch=1), lib.ERR_UNSUPPORTED, b"ntarget=1025")
        # P: >= 0, >= 1 with grad, <= 1024
        refused(f(P=-1, dm=None, g=None), lib.ERR_ARG, b"nparam must be")
        refused(f(P=0), lib.ERR_ARG, b"nparam must be")
        refused(f(P=1025, batch=1), lib.ERR_UNSUPPORTED, b"nparam=1025")
        # the pointers
        refused(f(b=None), lib.ERR_ARG, b"null device pointer")
        refused(f(h=None), lib.ERR_ARG, b"null device pointer")
        refused(f(**none), lib.ERR_ARG, b"no output requested")
        for one in none:
            refused(f(y=None, **dict(none, **{one: p})), lib.ERR_ARG, b"dYs is null")
            refused(f(D=0, **dict(none, **{one: p})), lib.ERR_ARG, b"ntarget")
        refused(f(dm=None), lib.ERR_ARG, b"dDMs is null")
        # without grad P = 0 and dDMs = NULL pass the argument checks: the call gets as far as the device (or runs)
        assert f(P=0, dm=None, g=None, n=1025, batch=1) == lib.ERR_UNSUPPORTED
        # the order: n before dtype, the counts before the pointers, the outputs before the limits
        refused(f(n=0, dtype=2), lib.ERR_ARG, b"n must be")
        refused(f(n=0, K=0), lib.ERR_ARG, b"n must be")
        refused(f(K=0, D=0), lib.ERR_ARG, b"nbasis")
        refused(f(D=0, b=None), lib.ERR_ARG, b"ntarget")
        refused(f(P=0, dm=None), lib.ERR_ARG, b"nparam")
        refused(f(n=1025, **none), lib.ERR_ARG, b"output")
        refused(f(batch=1, n=1025), lib.ERR_UNSUPPORTED, b"n=1025")
        assert f(batch=1, n=1025, b=None) == lib.ERR_ARG
        refused(f(batch=1, n=1025, D=1025), lib.ERR_UNSUPPORTED, b"n=1025")
        refused(f(batch=1, D=1025, P=1025), lib.ERR_UNSUPPORTED, b"ntarget=1025")
        # batch
        refused(f(batch=0x80000000), lib.ERR_ARG, b"batch")
        assert f(batch=0, **nothing) == lib.OK
        assert f(batch=0, dtype=5, **nothing) == lib.ERR_ARG
        assert f(batch=0, n=0, **nothing) == lib.ERR_ARG


def test_api_argument_validation():
    """api.trend_grad_batched refuses what it can see before the library is called"""
    torch = pytest.importorskip("torch")
    api = pkg("api")
    n = 4
    B = torch.eye(n, dtype=torch.float64).reshape(-1).repeat(2)
    H = torch.ones(2 * 2 * n, dtype=torch.float64)
    Y = torch.zeros(2 * 3 * n, dtype=torch.float64)
    dM = torch.zeros(2 * 2 * n * n, dtype=torch.float64)
    with pytest.raises(ValueError):  # CPU tensors
        api.trend_grad_batched(n, B, None, H, Y, dM)
    if torch.cuda.is_available():
        B, H, Y, dM = B.cuda(), H.cuda(), Y.cuda(), dM.cuda()
        with pytest.raises(ValueError, match="want holds"):
            api.trend_grad_batched(n, B, None, H, Y, dM, want=("grad", "quad"))
        with pytest.raises(ValueError, match="no output"):
            api.trend_grad_batched(n, B, None, H, Y, dM, want=())
        with pytest.raises(ValueError, match="basis vectors"):
            api.trend_grad_batched(n, B, None, None, Y, dM)
        with pytest.raises(ValueError, match="needs the targets"):
            api.trend_grad_batched(n, B, None, H, None, dM, want=("gradc",))
        with pytest.raises(ValueError, match="grad needs"):
            api.trend_grad_batched(n, B, None, H, Y, None)
        with pytest.raises(ValueError, match="nbasis must be"):
            api.trend_grad_batched(n, B, None, H, Y, dM, nbasis=5)
        with pytest.raises(ValueError, match="Hs needs"):
            api.trend_grad_batched(n, B, None, H[:n], Y, dM, nbasis=2)
        with pytest.raises(ValueError, match="Ys needs"):
            api.trend_grad_batched(n, B, None, H, Y[:n], dM, want=("alpha",))
        with pytest.raises(ValueError, match="dMs needs"):
            api.trend_grad_batched(n, B, None, H, Y, dM[:n * n])
        with pytest.raises(TypeError):
            api.trend_grad_batched(n, B, None, H, Y.float(), dM)
        with pytest.raises(ValueError, match="Cs needs"):
            api.trend_grad_batched(n, B, Y[:n], H, Y, dM)
        with pytest.raises(ValueError, match="info"):
            api.trend_grad_batched(n, B, None, H, Y, dM, info=torch.zeros(2, dtype=torch.int64, device="cuda"))
    # the host form validates before it needs a device
    Bn, Hn, Yn, dMn = np.tile(np.eye(n).reshape(-1), 2), np.ones(2 * 2 * n), np.zeros(2 * 3 * n), np.zeros(2 * 2 * n * n)
    with pytest.raises(ValueError, match="want must name"):
        api.trend_grad_batched_host(n, Bn, None, Hn, Yn, dMn, want=())
    with pytest.raises(ValueError, match="want must name"):
        api.trend_grad_batched_host(n, Bn, None, Hn, Yn, dMn, want=("quad",))
    with pytest.raises(ValueError, match="basis vectors"):
        api.trend_grad_batched_host(n, Bn, None, None, Yn, dMn)
    with pytest.raises(ValueError, match="needs the targets"):
        api.trend_grad_batched_host(n, Bn, None, Hn, None, dMn, want=("logml",))
    with pytest.raises(ValueError, match="grad needs"):
        api.trend_grad_batched_host(n, Bn, None, Hn, Yn, None, want=("grad",))
    with pytest.raises(ValueError, match="nbasis must be"):
        api.trend_grad_batched_host(n, Bn, None, Hn, Yn, dMn, nbasis=17)
    with pytest.raises(ValueError, match="Ys needs"):
        api.trend_grad_batched_host(n, Bn, None, Hn, Yn[:n], dMn, want=("alpha",), ntarget=3)
    with pytest.raises(TypeError):
        api.trend_grad_batched_host(n, Bn, None, Hn, Yn.astype(np.float32), dMn)
    with pytest.raises(ValueError, match="Cs smaller"):
        api.trend_grad_batched_host(n, Bn, Yn[:n], Hn, Yn, dMn)


def test_host_form_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    api = pkg("api")
    lib = pkg("_lib")
    B = np.eye(20).reshape(-1)
    H = np.ones(2 * 20)
    y = np.ones(3 * 20)
    calls = (lambda: api.trend_grad_batched_host(20, B, np.ones(20), H, y, np.ones(2 * 400)),
             lambda: api.trend_grad_batched_host(20, B, None, H, y, None),
             lambda: api.trend_grad_batched_host(20, B, None, H, y, None, want=("gradc",)))
    for call in calls:
        with pytest.raises(lib.MatinvError) as err:
            call()
        assert err.value.code in (lib.ERR_NO_DEVICE, lib.ERR_HIP)
        assert lib.lib().matinv_last_error()


ELEVEN = ", true" * 11
TREND_GRAD_FORMS = (r"matinv_spd_tile_f(64|32)<\d+, (true|false)" + ELEVEN + ">", r"matinv_chol_global<(double|float)" + ELEVEN + ">")


@pytest.mark.parametrize("f64", [True, False])
def test_trend_grad_dispatch_names(f64):
    api = pkg("api")
    dt, t, c = (api.F64, "f64", "double") if f64 else (api.F32, "f32", "float")
    assert api.trend_grad_kernel_name(dt, 1) == f"matinv_spd_tile_{t}<1, false{ELEVEN}>"
    assert api.trend_grad_kernel_name(dt, 16) == f"matinv_spd_tile_{t}<1, true{ELEVEN}>"
    assert api.trend_grad_kernel_name(dt, 17) == f"matinv_spd_tile_{t}<2, false{ELEVEN}>"
    assert api.trend_grad_kernel_name(dt, 96) == f"matinv_spd_tile_{t}<6, true{ELEVEN}>"
    assert api.trend_grad_kernel_name(dt, 97) == f"matinv_chol_global<{c}{ELEVEN}>"
    assert api.trend_grad_kernel_name(dt, 1024) == f"matinv_chol_global<{c}{ELEVEN}>"
    # a refused request has the name ""
    assert api.trend_grad_kernel_name(dt, 0) == "" == api.trend_grad_kernel_name(dt, 1025)
    assert api.trend_grad_kernel_name(9, 32) == "" == api.trend_grad_kernel_name(-1, 200)
    assert api.trend_grad_kernel_name(np.float64 if f64 else np.float32, 33) == api.trend_grad_kernel_name(dt, 33)


@pytest.mark.skipif(audit.NM is None, reason="no nm on this machine")
def test_every_trend_grad_name_is_a_compiled_kernel_and_every_trend_grad_form_is_named():
    """what test_instantiations_cpu checks for the routes of the generated sweep, for the trend gradient forms: exact names, both
    directions"""
    api = pkg("api")
    named = {api.trend_grad_kernel_name(dt, n) for dt in (api.F64, api.F32) for n in range(1, 1025)}
    assert "" not in named and len(named) == 2 * (12 + 1)
    assert all(any(re.fullmatch(p, s) for p in TREND_GRAD_FORMS) for s in named)
    missing = sorted(named - audit.STUBS)
    assert not missing, f"named by matinv_trend_grad_kernel_name but not compiled: {missing}"
    compiled = {s for s in audit.STUBS if any(re.fullmatch(p, s) for p in TREND_GRAD_FORMS)}
    assert compiled, "no trend gradient form is compiled"
    assert not sorted(compiled - named), f"compiled trend gradient forms no n reaches: {sorted(compiled - named)}"
    # the inverse's route names claim the new forms by the prefix rule of test_instantiations_cpu
    for s in named:
        base = re.sub(r"(, true){11}>$", ">", s)
        assert audit.matches(base, s), (base, s)
    # the earlier audits do not take a trend gradient form for one of theirs, nor the reverse
    import test_colour_cpu
    import test_logml_grad_cpu
    import test_loo_cpu
    import test_loo_grad_cpu
    import test_multi_target_cpu
    import test_multi_target_grad_cpu
    import test_predict_cov_cpu
    import test_predict_cpu
    import test_trend_cpu
    import test_whiten_cpu
    others = test_loo_cpu.LOO_FORMS + test_logml_grad_cpu.GRAD_FORMS + test_predict_cpu.PREDICT_FORMS + \
        test_predict_cov_cpu.PREDICT_COV_FORMS + test_loo_grad_cpu.LOO_GRAD_FORMS + test_colour_cpu.COLOUR_FORMS + \
        test_whiten_cpu.WHITEN_FORMS + test_multi_target_cpu.MULTI_TARGET_FORMS + test_multi_target_grad_cpu.MULTI_TARGET_GRAD_FORMS + \
        test_trend_cpu.TREND_FORMS
    assert not any(re.fullmatch(p, s) for p in others for s in named)
    theirs = {s for s in audit.STUBS if any(re.fullmatch(p, s) for p in others)}
    assert theirs and not any(re.fullmatch(p, s) for p in TREND_GRAD_FORMS for s in theirs)


FD_SHAPES = [(5, (1, 1, 1)), (17, (3, 17, 2)), (33, (4, 33, 3))]


@pytest.mark.parametrize("n,kdp", FD_SHAPES)
def test_reference_is_the_gradient_of_the_trend_reference_sum_of_logml(n, kdp):
    """central finite differences of _trend_worker's reference sum_t logml_t in float64: M +- h dM_p for grad, c_i +- h for gradc, step
    h = 1e-5 ||M||_2 / ||dM||_2 (the perturbation is 1e-5 ||M||_2 in the 2-norm; for c_i, ||dM|| = 1), relative agreement 1e-6. The
    truncation error of the central difference is of relative order (h ||dM|| ||Kinv||)^2 = (1e-5 cond2(M))^2 for the log det M and the
    quadratic term; the REML term log det A = log det(H^T Kinv H) sees the same perturbation of Kinv through a K x K matrix of condition
    <= 100 (asserted on every case), and cond2(M) <= 3 here, so the same step serves it: 1e-10 cond2(M)^2 cond2(A) stays far below
    1e-6."""
    K, D, P = kdp
    K = TG.clip(K, n)
    B, c, Hs, Ys, dMs, full = TG.case(n, "float64", True, K)
    ref = TG.take(full, dMs, n, D, P)
    assert ref["cond"].max() <= 3
    M, dM = ref["M"], ref["dM"]
    y = TG.first(Ys, n, TG.DMAX, D).reshape(-1, D * n)
    H = np.asarray(Hs).reshape(-1, K * n)
    worst = 0.0
    for k in range(0, M.shape[0], 4):  # every fourth matrix of the batch: three or four of them
        scale = max(1.0, np.abs(ref["grad"][k]).max(), np.abs(ref["gradc"][k]).max())
        mnorm = np.linalg.norm(M[k], 2)
        f = lambda m: TG.sum_logml(m, H[k], y[k], n, K, D)  # noqa: E731
        for p in range(P):
            h = 1e-5 * mnorm / np.linalg.norm(dM[k, p], 2)
            fd = (f(M[k] + h * dM[k, p]) - f(M[k] - h * dM[k, p])) / (2 * h)
            worst = max(worst, abs(fd - ref["grad"][k, p]) / scale)
            assert abs(fd - ref["grad"][k, p]) <= 1e-6 * scale, (n, k, p, fd, ref["grad"][k, p])
        h = 1e-5 * mnorm
        for i in range(n):
            e = np.zeros((n, n))
            e[i, i] = h
            fd = (f(M[k] + e) - f(M[k] - e)) / (2 * h)
            worst = max(worst, abs(fd - ref["gradc"][k, i]) / scale)
            assert abs(fd - ref["gradc"][k, i]) <= 1e-6 * scale, (n, k, i, fd, ref["gradc"][k, i])
        # sum_logml is the sum of the reference logml
        direct = f(M[k])
        assert abs(direct - float(ref["logml"][k].sum())) <= 1e-10 * max(1.0, abs(direct))
    print(f"  finite differences n={n} K={K} D={D} P={P}: worst relative difference {worst:.2e}")


def projection_case(n, K, D, dtname="float64"):
    """the shared case with dM_b = h_b h_b^T, b < K: (reference, reference without the U U^T term)"""
    B, c, Hs, Ys, _, full = TG.case(n, dtname, True, K)
    h = np.asarray(Hs, dtype=np.float64).reshape(-1, K, n)
    dm = np.einsum("kbi,kbj->kbij", h, h).reshape(-1)
    tr = TG.T.take(full, D, 0)
    return TG.reference(tr, dm, n, K), TG.reference(tr, dm, n, K, projection=False)


@pytest.mark.parametrize("n,kdp", FD_SHAPES + [(64, (16, 16, 2)), (96, (4, 33, 3)), (130, (4, 33, 3))])
def test_the_projection_makes_the_gradient_along_the_basis_vanish(n, kdp):
    """G H = 0 (P H = 0 and H^T alpha_t = 0), so for dM_b = h_b h_b^T the reference grad_b = 1/2 h_b^T G h_b is zero within its own
    bound, in either precision's bound. A reference without the U U^T term -- what any zero-mean gradient entry point would give on
    the trend's alpha -- is off by D / 2 h_b^T Kinv H A^-1 H^T Kinv h_b: more than 100 bounds. That holds for the fp64 bound at every
    shape here (5e9 bounds and more) and for the fp32 bound at n <= 33 (134 bounds at n = 33); from n = 64 on the fp32 bound, which
    grows with n sqrt(n) ||dM||_F, is within a factor 100 of the term (10 to 40 bounds at n = 64, K = 16), so those shapes are held
    against the fp64 bound only"""
    K, D, _ = kdp
    K = TG.clip(K, n)
    ref, flat = projection_case(n, K, D)
    for dt in (np.float64, np.float32) if n <= 33 else (np.float64,):
        b = TG.bounds(ref, n, TG.U[np.dtype(dt)])["grad"]
        assert (np.abs(ref["grad"]) <= b).all(), (n, dt, float((np.abs(ref["grad"]) / b).max()))
        miss = np.abs(flat["grad"] - ref["grad"]) / b
        print(f"  projection n={n} K={K} D={D} {np.dtype(dt).name}: |grad| / bound {float((np.abs(ref['grad']) / b).max()):.2e}, "
              f"without U U^T off by {float(miss.min()):.3g} to {float(miss.max()):.3g} bounds")
        assert (miss > 100).all(), (n, dt, float(miss.min()))


@pytest.mark.parametrize("n", TG.TILE_SIZES + TG.GLOBAL_SIZES + [1024])
def test_float32_numpy_stays_inside_the_fp32_bounds(n):
    """the bounds are derived, not fitted: a float32 numpy evaluation of the reference formulas must pass them at every size and
    (K, D, P) the GPU tests use, with and without c, before they are held against the kernels"""
    u = TG.U[np.dtype(np.float32)]
    for with_c in (True, False) if n < 1024 else (True,):
        for K, D, P in (TG.shapes_of(n) if n < 1024 else (TG.KDP_1024,)):
            B, c, Hs, Ys, dMs, full = TG.case(n, "float32", with_c, K)
            y, dm = TG.first(Ys, n, TG.DMAX, D), TG.first_derivs(dMs, n, TG.PMAX, P)
            TG.check(TG.float32_evaluation(B, c, Hs, y, dm, n, K, D, P), TG.take(full, dMs, n, D, P), n, u, what="float32 numpy")


def test_bounds_fail_a_wrong_result():
    """the alpha of the zero-mean model, a G without the factor D on P, and a single-element dM read at the transposed position of an
    asymmetric pattern (the upper triangle, which the kernels must not read) all fail"""
    n, K, D, P = 17, 3, 3, 2
    B, c, Hs, Ys, dMs, full = TG.case(n, "float64", True, K)
    ref = TG.take(full, dMs, n, D, P)
    u = TG.U[np.dtype(np.float64)]
    once = 0.5 * np.einsum("kij,kpij->kp", ref["G"] + (D - 1) * ref["Pmat"], ref["dM"])
    wrong = [dict(alpha=ref["Ky"]), dict(grad=once), dict(gradc=0.5 * np.einsum("kii->ki", ref["G"] + (D - 1) * ref["Pmat"]))]
    # dM = e_i e_j^T, i > j, in the lower triangle only (column-major: element (i, j) at j n + i): the kernel reads it and grad = G_ij;
    # one that read the upper triangle would see zero
    batch = ref["M"].shape[0]
    i, j = 11, 4
    dm = np.zeros((batch, 1, n * n))
    dm[:, 0, j * n + i] = 1.0
    single = TG.reference(TG.T.take(full, D, 0), dm.reshape(-1), n, 1)
    assert np.allclose(single["grad"][:, 0], ref["G"][:, i, j])
    TG.check(dict(grad=ref["G"][:, i, j]), single, n, u, what="single element")
    for w, r in [(x, ref) for x in wrong] + [(dict(grad=np.zeros((batch, 1))), single)]:
        with pytest.raises(AssertionError):
            TG.check(w, r, n, u, what="wrong on purpose")
