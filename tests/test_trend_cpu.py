"""CPU-side checks of the GP regression with a linear trend (matinv_trend_batched*): exports, argument errors, dispatch names, the audit of
the compiled trend kernel forms that the generated instantiation sweep cannot make (the forms carry the names of the SPD inversion kernels
with ten more template arguments), the meaning of the reference (it is the vague-prior limit of the zero-mean formulas), the check that the
bounds of tests/_trend_worker.py hold for a float32 numpy evaluation of the reference formulas, and that they fail wrong results.
No GPU needed."""
import ctypes
import re

import numpy as np
import pytest

import _trend_worker as T
import test_instantiations_cpu as audit
from conftest import pkg

NAMES = ["matinv_trend_batched", "matinv_trend_kernel_name", "matinv_trend_batched_host"]
OUT = ("be", "cb", "al", "qd", "lm", "mn", "vr")


def test_trend_symbols_exported_and_named_in_the_header():
    import os
    lib = pkg("_lib")
    L = lib.lib()
    header = open(os.path.join(T.ROOT, "include", "matinv.h")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in lib.NATIVE_NAMES
        assert re.search(rf"\b{name}\(", header), name
    api = pkg("api")
    for name in ("trend_batched", "trend_batched_host", "trend_kernel_name"):
        assert callable(getattr(api, name))
    assert L.matinv_abi_version() == 2


def test_trend_argument_errors_without_device():
    """every rule of the contract in include/matinv.h, in the order of matinv_multi_target_batched"""
    lib = pkg("_lib")
    L = lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def dev(dtype=0, n=4, K=2, D=2, Q=2, b=p, c=p, h=p, y=p, a=p, g=p, e=p, be=p, cb=p, al=p, qd=p, lm=p, mn=p, vr=p, batch=2):
        return L.matinv_trend_batched(dtype, n, K, D, Q, b, c, h, y, a, g, e, be, cb, al, qd, lm, mn, vr, batch, None, None)

    def host(dtype=0, n=4, K=2, D=2, Q=2, b=p, c=p, h=p, y=p, a=p, g=p, e=p, be=p, cb=p, al=p, qd=p, lm=p, mn=p, vr=p, batch=2):
        return L.matinv_trend_batched_host(dtype, n, K, D, Q, b, c, h, y, a, g, e, be, cb, al, qd, lm, mn, vr, batch, None)

    none = dict.fromkeys(OUT)
    nothing = dict(b=None, c=None, h=None, y=None, a=None, g=None, e=None, **none)
    for f in (dev, host):
        assert f(n=0) == lib.ERR_ARG
        assert b"n must be" in L.matinv_last_error()
        assert f(dtype=2) == lib.ERR_ARG
        # 1 <= nbasis <= 16 and nbasis <= n
        for K in (0, -1, 17):
            assert f(n=32, K=K) == lib.ERR_ARG
            assert b"nbasis" in L.matinv_last_error()
        assert f(n=4, K=5) == lib.ERR_ARG
        assert b"nbasis" in L.matinv_last_error()
        assert f(b=None) == lib.ERR_ARG
        assert f(h=None) == lib.ERR_ARG
        assert f(**none) == lib.ERR_ARG
        assert b"output" in L.matinv_last_error()
        # Y and D are needed with beta, alpha, quad, logml and mean, and only with them
        for one in ("be", "al", "qd", "lm", "mn"):
            only = dict(none, **{one: p})
            assert f(y=None, **only) == lib.ERR_ARG
            assert b"dYs" in L.matinv_last_error()
            assert f(D=0, **only) == lib.ERR_ARG
            assert b"ntarget" in L.matinv_last_error()
        # A, G and Q are needed with mean and var, and only with them; E with var only
        for one in ("mn", "vr"):
            only = dict(none, **{one: p})
            assert f(a=None, **only) == lib.ERR_ARG
            assert b"dAs" in L.matinv_last_error()
            assert f(g=None, **only) == lib.ERR_ARG
            assert b"dGs" in L.matinv_last_error()
            assert f(Q=0, **only) == lib.ERR_ARG
            assert b"nquery" in L.matinv_last_error()
        assert f(e=None) == lib.ERR_ARG
        assert b"dEs" in L.matinv_last_error()
        # the order of the other GP entry points: n before dtype, the counts before the pointers, the outputs before the limits
        assert f(n=0, dtype=2) == lib.ERR_ARG and b"n must be" in L.matinv_last_error()
        assert f(Q=0, a=None) == lib.ERR_ARG and b"nquery" in L.matinv_last_error()
        assert f(n=1025, **none) == lib.ERR_ARG and b"output" in L.matinv_last_error()
        # batch == 0 is a no-op even with NULL pointers; n, dtype and nbasis are still checked
        assert f(batch=0, **nothing) == lib.OK
        assert f(batch=0, dtype=5, **nothing) == lib.ERR_ARG
        assert f(batch=0, n=0, **nothing) == lib.ERR_ARG
        assert f(batch=0, K=17, n=32, **nothing) == lib.ERR_ARG
        # n, D and Q = 1025 are refused after the pointer checks
        assert f(batch=1, n=1025) == lib.ERR_UNSUPPORTED
        assert f(batch=1, n=1025, b=None) == lib.ERR_ARG
        assert f(batch=1, n=1025, D=0, Q=0, y=None, a=None, g=None, e=None, **dict(none, cb=p)) == lib.ERR_UNSUPPORTED
        assert f(batch=1, D=1025) == lib.ERR_UNSUPPORTED
        assert b"ntarget" in L.matinv_last_error()
        assert f(batch=1, Q=1025) == lib.ERR_UNSUPPORTED
        assert b"nquery" in L.matinv_last_error()
        assert f(batch=0x80000000) == lib.ERR_ARG
        assert b"batch" in L.matinv_last_error()


def test_api_argument_validation():
    """api.trend_batched refuses what it can see before the library is called"""
    torch = pytest.importorskip("torch")
    api = pkg("api")
    n = 4
    B = torch.eye(n, dtype=torch.float64).reshape(-1).repeat(2)
    H = torch.ones(2 * n, dtype=torch.float64)
    Y = torch.zeros(2 * 3 * n, dtype=torch.float64)
    with pytest.raises(ValueError):  # CPU tensors
        api.trend_batched(n, B, None, H, Y)
    if torch.cuda.is_available():
        B, H, Y = B.cuda(), H.cuda(), Y.cuda()
        with pytest.raises(ValueError, match="want holds"):
            api.trend_batched(n, B, None, H, Y, want=("alpha", "logdet"))
        with pytest.raises(ValueError, match="no output"):
            api.trend_batched(n, B, None, H, Y, want=())
        with pytest.raises(ValueError, match="need the targets"):
            api.trend_batched(n, B, None, H, None, want=("quad",))
        with pytest.raises(ValueError, match="mean and var need"):
            api.trend_batched(n, B, None, H, Y, want=("mean",))
        with pytest.raises(ValueError, match="var needs"):
            api.trend_batched(n, B, None, H, Y, As=Y, Gs=Y, want=("var",))
        with pytest.raises(ValueError, match="nbasis"):
            api.trend_batched(n, B, None, H, Y, nbasis=5)
        with pytest.raises(ValueError, match="Ys needs"):
            api.trend_batched(n, B, None, H, Y[:n], want=("alpha",))
        with pytest.raises(TypeError):
            api.trend_batched(n, B, None, H, Y.float())
        with pytest.raises(ValueError, match="Cs needs"):
            api.trend_batched(n, B, Y[:n], H, Y)
        with pytest.raises(ValueError, match="info"):
            api.trend_batched(n, B, None, H, Y, info=torch.zeros(2, dtype=torch.int64, device="cuda"))
    # the host form validates before it needs a device
    Bn, Hn, Yn = np.tile(np.eye(n).reshape(-1), 2), np.ones(2 * n), np.zeros(2 * 3 * n)
    with pytest.raises(ValueError, match="no output"):
        api.trend_batched_host(n, Bn, None, Hn, Yn, want=())
    with pytest.raises(ValueError, match="want holds"):
        api.trend_batched_host(n, Bn, None, Hn, Yn, want=("logdet",))
    with pytest.raises(ValueError, match="need the targets"):
        api.trend_batched_host(n, Bn, None, Hn, None, want=("logml",))
    with pytest.raises(ValueError, match="mean and var need"):
        api.trend_batched_host(n, Bn, None, Hn, Yn, want=("mean",))
    with pytest.raises(ValueError, match="var needs"):
        api.trend_batched_host(n, Bn, None, Hn, Yn, As=Yn, Gs=Yn, want=("var",))
    with pytest.raises(ValueError, match="basis vectors"):
        api.trend_batched_host(n, Bn, None, None, Yn)
    with pytest.raises(ValueError, match="nbasis"):
        api.trend_batched_host(n, Bn, None, np.ones(2 * 5 * n), Yn)
    with pytest.raises(ValueError, match="Ys needs"):
        api.trend_batched_host(n, Bn, None, Hn, Yn[:n], want=("alpha",))
    with pytest.raises(TypeError):
        api.trend_batched_host(n, Bn, None, Hn, Yn.astype(np.float32))
    with pytest.raises(ValueError, match="Cs smaller"):
        api.trend_batched_host(n, Bn, Yn[:n], Hn, Yn)


@pytest.mark.parametrize("f64", [True, False])
def test_trend_dispatch_names(f64):
    api = pkg("api")
    dt, t, c = (api.F64, "f64", "double") if f64 else (api.F32, "f32", "float")
    ten = ", ".join(["true"] * 10)
    assert api.trend_kernel_name(dt, 1) == f"matinv_spd_tile_{t}<1, false, {ten}>"
    assert api.trend_kernel_name(dt, 16) == f"matinv_spd_tile_{t}<1, true, {ten}>"
    assert api.trend_kernel_name(dt, 17) == f"matinv_spd_tile_{t}<2, false, {ten}>"
    assert api.trend_kernel_name(dt, 96) == f"matinv_spd_tile_{t}<6, true, {ten}>"
    assert api.trend_kernel_name(dt, 97) == f"matinv_chol_global<{c}, {ten}>"
    assert api.trend_kernel_name(dt, 1024) == f"matinv_chol_global<{c}, {ten}>"
    assert api.trend_kernel_name(dt, 0) == "" == api.trend_kernel_name(dt, 1025)
    assert api.trend_kernel_name(9, 32) == "" == api.trend_kernel_name(-1, 200)
    assert api.trend_kernel_name(np.float64 if f64 else np.float32, 33) == api.trend_kernel_name(dt, 33)


def test_host_form_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    api = pkg("api")
    lib = pkg("_lib")
    B = np.eye(20).reshape(-1)
    h = np.ones(20)
    y = np.ones(3 * 20)
    calls = (lambda: api.trend_batched_host(20, B, np.ones(20), h, y, y, np.ones(3), np.ones(3)),
             lambda: api.trend_batched_host(20, B, None, h, y),
             lambda: api.trend_batched_host(20, B, None, h, want=("covbeta",)))
    for call in calls:
        with pytest.raises(lib.MatinvError) as err:
            call()
        assert err.value.code in (lib.ERR_NO_DEVICE, lib.ERR_HIP)
        assert lib.lib().matinv_last_error()


TREND_FORMS = (r"matinv_spd_tile_f(64|32)<\d+, (true|false), true, true, true, true, true, true, true, true, true, true>",
               r"matinv_chol_global<(double|float), true, true, true, true, true, true, true, true, true, true>")


@pytest.mark.skipif(audit.NM is None, reason="no nm on this machine")
def test_every_trend_name_is_a_compiled_kernel_and_every_trend_form_is_named():
    """what test_instantiations_cpu checks for the routes of the generated sweep, for the trend forms: exact names, both directions"""
    api = pkg("api")
    named = {api.trend_kernel_name(dt, n) for dt in (api.F64, api.F32) for n in range(1, 1025)}
    assert "" not in named and len(named) == 2 * (12 + 1)
    assert all(any(re.fullmatch(p, s) for p in TREND_FORMS) for s in named)
    missing = sorted(named - audit.STUBS)
    assert not missing, f"named by matinv_trend_kernel_name but not compiled: {missing}"
    compiled = {s for s in audit.STUBS if any(re.fullmatch(p, s) for p in TREND_FORMS)}
    assert compiled, "no trend form is compiled"
    assert not sorted(compiled - named), f"compiled trend forms no n reaches: {sorted(compiled - named)}"
    # the audits of the multi-target forms and of their gradient forms do not take a trend form for one of theirs, nor the reverse
    import test_multi_target_cpu
    import test_multi_target_grad_cpu
    others = test_multi_target_cpu.MULTI_TARGET_FORMS + test_multi_target_grad_cpu.MULTI_TARGET_GRAD_FORMS
    assert not any(re.fullmatch(p, s) for p in others for s in named)
    theirs = {s for s in audit.STUBS if any(re.fullmatch(p, s) for p in others)}
    assert theirs and not any(re.fullmatch(p, s) for p in TREND_FORMS for s in theirs)


def zero_mean_limit(ref, b, n, K):
    """mean, var and logml of the ordinary zero-mean formulas with M + b H H^T, a + b H g, e + b g^T g; logml after adding
    K / 2 (log b + log 2 pi)"""
    H, M = ref["H"], ref["M"]
    Mb = M + b * H @ H.transpose(0, 2, 1)
    ab = ref["a"] + b * np.einsum("kib,kqb->kqi", H, ref["g"])
    eb = ref["e"] + b * np.einsum("kqb,kqb->kq", ref["g"], ref["g"])
    Kb = np.linalg.inv(Mb)
    alpha = np.einsum("kij,ktj->kti", Kb, ref["y"])
    mean = np.einsum("kqi,kti->ktq", ab, alpha)
    var = eb - np.einsum("kqi,kij,kqj->kq", ab, Kb, ab)
    quad = np.einsum("kti,kti->kt", ref["y"], alpha)
    logml = -(quad + np.linalg.slogdet(Mb)[1][:, None] + n * T.LOG2PI) / 2 + K / 2 * (np.log(b) + T.LOG2PI)
    return dict(mean=mean, var=var, logml=logml)


@pytest.mark.parametrize("n,K", [(2, 1), (17, 3), (33, 16), (64, 4), (130, 16)])
def test_reference_is_the_vague_prior_limit(n, K):
    """R&W 2.7: a prior beta ~ N(0, b I) adds b H H^T to the covariance of y, b H g to the cross-covariance and b g^T g to the prior
    variance; the reference is the limit b -> infinity, approached in first order: the deviation at b = 1e4 is ten times that at 1e5
    (asserted: between 8 and 12 times), and below 1e-4 relative at b = 1e5. Relative means: against the largest magnitude of the output
    for mean and logml; for var against the terms it is the sum of, |e| + a^T Kinv a + r^T A^-1 r -- the inputs choose e so that var
    lands in 0.1 .. 1 whatever the size of r^T A^-1 r (up to 93 here), and the deviation, r^T A^-2 r / b in first order, scales with
    that term, not with what is left after the cancellation."""
    dt = np.float64
    B, c, _ = T.L.inputs(n, 5, dt, True)
    mdl = T.model(B, c, n)
    Hs, Ys, As, Gs, Es = T.vectors(n, 5, K, 3, 4, dt, 4242 + n, lambda h: T.basis_model(mdl, h, n, K))
    ref = T.reference(T.basis_model(mdl, Hs, n, K), Ys, As, Gs, Es, n, K, 3, 4)
    scale = dict(mean=np.abs(ref["mean"]).max(), logml=np.abs(ref["logml"].astype(np.float64)).max(),
                 var=np.abs(ref["e"]) + ref["aKa"] + ref["rar"])
    dev = {}
    for b in (1e4, 1e5):
        lim = zero_mean_limit(ref, b, n, K)
        dev[b] = {k: (np.abs(lim[k] - np.asarray(ref[k], dtype=np.float64)) / scale[k]).max() for k in ("mean", "var", "logml")}
    print(n, K, dev)
    for k in ("mean", "var", "logml"):
        assert dev[1e5][k] < 1e-4, (k, dev[1e5][k])
        assert 8 <= dev[1e4][k] / dev[1e5][k] <= 12, (k, dev[1e4][k] / dev[1e5][k])
    # H^T alpha = 0, and both forms of quad agree
    assert np.abs(np.einsum("kib,kti->ktb", ref["H"], ref["alpha"])).max() < 1e-10 * np.abs(ref["alpha"]).max() * np.abs(ref["H"]).max() * n
    res = ref["y"] - np.einsum("kib,ktb->kti", ref["H"], ref["beta"])
    assert np.abs(np.einsum("kti,kij,ktj->kt", res, ref["Kinv"], res) - ref["quad"]).max() < 1e-10 * np.abs(ref["quad"]).max()


def test_slices_of_the_shared_reference_are_the_reference_of_the_sliced_inputs():
    n, K = 33, 4
    cs = T.case(n, "float64", True, K)
    Hs, Ys, As, Gs, Es = T.inputs_of(cs, n, K, 16, 17)
    part = T.reference(T.basis_model(T.matrices(n, "float64", True)[2], Hs, n, K), Ys, As, Gs, Es, n, K, 16, 17)
    took = T.take(cs[7], 16, 17)
    for k in T.OUTPUTS:
        assert np.array_equal(np.asarray(part[k], dtype=np.float64), np.asarray(took[k], dtype=np.float64)), k


@pytest.mark.parametrize("n", T.TILE_SIZES + T.GLOBAL_SIZES + [1024])
def test_float32_numpy_stays_inside_the_fp32_bounds(n):
    """the bounds are derived, not fitted: a float32 numpy evaluation of the reference formulas must pass them at every size and
    (K, D, Q) the GPU tests use, with and without c, before they are held against the kernels"""
    u = T.U[np.dtype(np.float32)]
    for with_c in (True, False) if n < 1024 else (True,):
        for K, D, Q in (T.shapes_of(n) if n < 1024 else (T.KDQ_1024,)):
            cs = T.case(n, "float32", with_c, K)
            inp = T.inputs_of(cs, n, K, D, Q)
            T.check(T.float32_evaluation(cs[0], cs[1], *inp, n, K, D, Q), T.take(cs[7], D, Q), n, u, what="float32 numpy")


def test_bounds_fail_a_wrong_result():
    """logml without log det A, logml with n in place of n - K, mean without g^T beta, var without r^T A^-1 r, alpha of the uncorrected
    Kinv y, and a beta wrong by one part in a thousand all fail their bounds"""
    n, K = 33, 4
    cs = T.case(n, "float64", True, K)
    full = cs[7]
    u = T.U[np.dtype(np.float64)]
    T.check({k: np.asarray(full[k], dtype=np.float64) for k in T.OUTPUTS}, full, n, u, what="the reference itself")
    ldA = full["logdetA"].astype(np.float64)[:, None]
    logml = np.asarray(full["logml"], dtype=np.float64)
    wrongs = (dict(logml=logml + ldA / 2),
              dict(logml=logml - K * T.LOG2PI / 2),
              dict(mean=full["mean"] - np.einsum("kqb,ktb->ktq", full["g"], full["beta"])),
              dict(var=full["var"] - full["rar"]),
              dict(alpha=full["Ky"]),
              dict(beta=full["beta"] * 1.001))
    for wrong in wrongs:
        with pytest.raises(AssertionError):
            T.check(wrong, full, n, u, what="wrong on purpose")
