"""CPU-side checks of the leave-one-out cross-validation of the trend GP (matinv_trend_loo_batched*): exports and prototypes, argument
refusals, dispatch names against the compiled stubs (the forms carry the names of the SPD inversion kernels with twelve more template
arguments), the meaning of the reference (n brute-force fits on n - 1 points with _trend_worker.reference), and the checks that the bounds
of tests/_trend_loo_worker.py hold for a float32 numpy evaluation of the reference formulas and fail wrong results. No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import _trend_loo_worker as TL
import _trend_worker as T
import test_instantiations_cpu as audit
from conftest import pkg

NAMES = ["matinv_trend_loo_batched", "matinv_trend_loo_kernel_name", "matinv_trend_loo_batched_host"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = ", true" * 12 + ">"


def test_trend_loo_symbols_exported_with_their_prototypes():
    lib = pkg("_lib")
    L = lib.lib()
    header = open(os.path.join(ROOT, "include", "matinv.h")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in lib.NATIVE_NAMES
        assert re.search(rf"\b{name}\(", header), name
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    assert L.matinv_trend_loo_batched.argtypes == [ci] * 4 + [vp] * 7 + [sz, vp, vp] and L.matinv_trend_loo_batched.restype is ci
    assert L.matinv_trend_loo_batched_host.argtypes == [ci] * 4 + [vp] * 7 + [sz, vp] and L.matinv_trend_loo_batched_host.restype is ci
    assert L.matinv_trend_loo_kernel_name.argtypes == [ci, ci] and L.matinv_trend_loo_kernel_name.restype is ctypes.c_char_p
    # the header declares what the prototypes say: four ints, seven pointers, the batch, info (and the stream)
    m = re.search(r"int matinv_trend_loo_batched\(([^;]*)\);", header)
    assert m and [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == \
        ["dtype", "n", "nbasis", "ntarget", "dBs", "dCs", "dHs", "dYs", "dMean", "dVar", "dLogPL", "batch", "dInfo", "stream"]
    m = re.search(r"int matinv_trend_loo_batched_host\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == 13
    api = pkg("api")
    for name in ("trend_loo_batched", "trend_loo_batched_host", "trend_loo_kernel_name"):
        assert callable(getattr(api, name))
    assert L.matinv_abi_version() == 2


def test_trend_loo_kernel_names_are_compiled_stubs():
    api = pkg("api")
    seen = set()
    for dt in (np.float64, np.float32):
        for n in range(2, 1025):
            name = api.trend_loo_kernel_name(dt, n)
            assert name.endswith(TAIL) and name.startswith("matinv_spd_tile_f" if n <= 96 else "matinv_chol_global<"), (n, name)
            seen.add(name)
    assert seen <= audit.STUBS, sorted(seen - audit.STUBS)  # exactly a stub, not a prefix of one
    forms = {s for s in audit.STUBS if s.endswith(TAIL) and s.count("true") + s.count("false") in (12, 13) and
             (s.startswith("matinv_chol_global<") and s.count("true") == 12 or s.startswith("matinv_spd_tile_f") and
              len(s[s.index("<") + 1:-1].split(", ")) == 14)}
    assert len(forms) == 26 and forms == seen, sorted(forms ^ seen)
    # no held-out fit at n = 1 (nbasis >= 1), nothing beyond 1024, no other dtype
    for dt in (np.float64, np.float32):
        for n in (-1, 0, 1, 1025, 4096):
            assert api.trend_loo_kernel_name(dt, n) == ""
    L = pkg("_lib").lib()
    assert L.matinv_trend_loo_kernel_name(2, 32) == b"" == L.matinv_trend_loo_kernel_name(-1, 32)


def test_trend_loo_argument_refusals_without_device():
    lib = pkg("_lib")
    L = lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def dev(dtype=0, n=4, K=2, D=2, b=p, c=p, h=p, y=p, mn=p, vr=p, lp=p, batch=2):
        return L.matinv_trend_loo_batched(dtype, n, K, D, b, c, h, y, mn, vr, lp, batch, None, None)

    def host(dtype=0, n=4, K=2, D=2, b=p, c=p, h=p, y=p, mn=p, vr=p, lp=p, batch=2):
        return L.matinv_trend_loo_batched_host(dtype, n, K, D, b, c, h, y, mn, vr, lp, batch, None)

    def refused(rc, code, text):
        assert rc == code, (rc, code, text, L.matinv_last_error())
        assert text in L.matinv_last_error(), (text, L.matinv_last_error())

    none = dict(mn=None, vr=None, lp=None)
    nothing = dict(b=None, c=None, h=None, y=None, **none)
    for f in (dev, host):
        refused(f(n=0), lib.ERR_ARG, b"n must be")
        assert f(dtype=2) == lib.ERR_ARG
        for K in (0, -1, 17):
            refused(f(K=K, n=32), lib.ERR_ARG, b"nbasis must be in 1 .. 16")
            refused(f(K=K, n=32, batch=0, **nothing), lib.ERR_ARG, b"nbasis must be in 1 .. 16")
        # n <= nbasis: no held-out fit
        for n, K in ((4, 4), (4, 5), (1, 1), (16, 16)):
            refused(f(K=K, n=n), lib.ERR_ARG, b"no held-out fit")
            refused(f(K=K, n=n, batch=0, **nothing), lib.ERR_ARG, b"no held-out fit")
        refused(f(**none), lib.ERR_ARG, b"no output requested")
        refused(f(b=None), lib.ERR_ARG, b"null device pointer")
        refused(f(h=None), lib.ERR_ARG, b"null device pointer")
        # mean and logpl need the targets, var does not
        for one in ("mn", "lp"):
            refused(f(D=0, **dict(none, **{one: p})), lib.ERR_ARG, b"ntarget must be >= 1")
            refused(f(y=None, **dict(none, **{one: p})), lib.ERR_ARG, b"dYs is null")
        refused(f(D=1025, batch=1), lib.ERR_UNSUPPORTED, b"ntarget=1025")
        # the var-only call passes every argument check with D = 0 and no Y: it is refused for its size alone
        refused(f(D=0, y=None, mn=None, lp=None, n=1025, batch=1), lib.ERR_UNSUPPORTED, b"n=1025")
        refused(f(batch=1, n=1025), lib.ERR_UNSUPPORTED, b"n=1025")
        assert f(batch=1, n=1025, b=None) == lib.ERR_ARG
        refused(f(batch=0x80000000), lib.ERR_ARG, b"batch")
        assert f(batch=0, **nothing) == lib.OK
        assert f(batch=0, dtype=5, **nothing) == lib.ERR_ARG
        assert f(batch=0, n=0, **nothing) == lib.ERR_ARG


def test_api_argument_validation():
    api = pkg("api")
    n = 4
    Bn, Hn, Yn = np.tile(np.eye(n).reshape(-1), 2), np.ones(2 * 2 * n), np.zeros(2 * 3 * n)
    with pytest.raises(ValueError, match="want holds"):
        api.trend_loo_batched_host(n, Bn, None, Hn, Yn, want=("mean", "quad"))
    with pytest.raises(ValueError, match="no output"):
        api.trend_loo_batched_host(n, Bn, None, Hn, Yn, want=())
    with pytest.raises(ValueError, match="basis vectors"):
        api.trend_loo_batched_host(n, Bn, None, None, Yn)
    with pytest.raises(ValueError, match="need the targets"):
        api.trend_loo_batched_host(n, Bn, None, Hn, None, want=("mean",))
    with pytest.raises(ValueError, match="nbasis must be"):
        api.trend_loo_batched_host(n, Bn, None, Hn, Yn, nbasis=4)
    with pytest.raises(ValueError, match="Hs needs"):
        api.trend_loo_batched_host(n, Bn, None, Hn[:n], Yn, nbasis=2)
    with pytest.raises(ValueError, match="Ys needs"):
        api.trend_loo_batched_host(n, Bn, None, Hn, Yn[:n], ntarget=3)
    with pytest.raises(TypeError):
        api.trend_loo_batched_host(n, Bn, None, Hn, Yn.astype(np.float32))
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError):  # CPU tensors
        api.trend_loo_batched(n, torch.tensor(Bn), None, torch.tensor(Hn), torch.tensor(Yn))


def brute_force(M, H, y):
    """mean[t, i], var[i]: the trend GP refitted on the n - 1 other points (_trend_worker.reference), predicting point i with
    a = M[-i, i], e = M_ii, g = H[i, :]"""
    n, K = H.shape
    D = y.shape[0]
    mean, var, bm_, bv_ = np.empty((D, n)), np.empty(n), np.empty((D, n)), np.empty(n)
    for i in range(n):
        keep = np.array([j for j in range(n) if j != i])
        Mi = M[np.ix_(keep, keep)]
        sv = np.linalg.svd(Mi, compute_uv=False)
        mdl = {"M": Mi[None], "Kinv": np.linalg.inv(Mi)[None], "cond": np.array([sv[0] / sv[-1]]), "knorm": np.array([1 / sv[-1]]),
               "logdet": np.array([np.linalg.slogdet(Mi)[1]], dtype=np.longdouble)}
        # _trend_worker.basis_model without its condition on cond2(A): the held-out fits are what they are, and their bounds say so
        Hi = H[keep][None]
        KH = mdl["Kinv"] @ Hi
        A = Hi.transpose(0, 2, 1) @ KH
        A = (A + A.transpose(0, 2, 1)) / 2
        sa = np.linalg.svd(A, compute_uv=False)
        bm = dict(mdl, H=Hi, KH=KH, A=A, Ainv=np.linalg.inv(A), condA=sa[:, 0] / sa[:, -1], anorm=1.0 / sa[:, -1],
                  hnorm=np.linalg.norm(Hi, 2, axis=(1, 2)), khnorm=np.linalg.norm(KH, 2, axis=(1, 2)),
                  logdetA=np.array([np.linalg.slogdet(A[0])[1]], dtype=np.longdouble))
        ref = T.reference(bm, np.ascontiguousarray(y[:, keep]).reshape(-1), M[keep, i].copy(), H[i].copy(), np.array([M[i, i]]), n - 1, K, D,
                          1)
        b = T.bounds(ref, n - 1, 2.0 ** -53)
        mean[:, i], var[i] = ref["mean"][0, :, 0], ref["var"][0, 0]
        bm_[:, i], bv_[i] = b["mean"][0, :, 0], b["var"][0, 0]
    return mean, var, bm_, bv_


@pytest.mark.parametrize("n", [2, 3, 17, 33])
def test_reference_against_brute_force(n):
    """Dubrule's identities against n refits on n - 1 points, every held-out i of two matrices, three targets; and logpl against the sum
    of the Gaussian log-densities"""
    K = min(TL.clip(16, n), n - 1)  # 1, 2, 3, 16
    D = 3
    # an identity of exact arithmetic: no leverage condition (at n = 3, K = 2 every point has a high one); the bounds carry it
    B, c, Hs, Ys, full = TL.case(n, "float64", True, K, check_leverage=False)
    ref = TL.take(full, D)
    b = TL.bounds(ref, n, 2.0 ** -53)
    for k in (0, 1):
        M, H, y = ref["M"][k], ref["H"][k], ref["y"][k]
        mean, var, bmean, bvar = brute_force(M, H, y)
        em = np.abs(mean - ref["mean"][k]) / (bmean + b["mean"][k])
        ev = np.abs(var - ref["var"][k]) / (bvar + b["var"][k])
        print(f"  n={n} K={K} matrix {k}: worst |brute - LOO| / (sum of bounds) mean {em.max():.3g} var {ev.max():.3g}; relative "
              f"{(np.abs(var - ref['var'][k]) / var).max():.3g}")
        assert (em <= 1).all() and (ev <= 1).all()
        dens = (-0.5 * np.log(2 * np.pi * ref["var"][k])[None] - 0.5 * (y - ref["mean"][k]) ** 2 / ref["var"][k][None]).sum(axis=1)
        assert np.abs(dens - ref["logpl"][k]).max() <= 1e-12 * np.abs(dens).max() + b["logpl"][k].max()


def cases_of(n):
    for K, D in TL.shapes_of(n):
        for with_c in (True, False):
            yield K, D, with_c


@pytest.mark.parametrize("n", TL.TILE_SIZES + TL.GLOBAL_SIZES)
def test_float32_evaluation_is_inside_the_fp32_bounds(n):
    """at every size and (K, D) the GPU tests use; also asserts the two input conditions (cond2(A), leverage) of every fp32 and fp64 case"""
    for K, D, with_c in cases_of(n):
        TL.case(n, "float64", with_c, K)
        B, c, Hs, Ys, full = TL.case(n, "float32", with_c, K)
        out = TL.float32_evaluation(B, c, Hs, T.first(Ys, n, TL.DMAX, D), n, K, D)
        TL.check(out, TL.take(full, D), n, TL.U[np.dtype(np.float32)], what="float32 numpy" + (" c" if with_c else ""))


@pytest.mark.parametrize("n", [17, 33, 96, 130])
def test_bounds_reject_wrong_results(n):
    K, D = min(TL.clip(4, n), n - 1), 3
    for dtname in ("float64", "float32"):
        B, c, Hs, Ys, full = TL.case(n, dtname, True, K)
        ref = TL.take(full, D)
        u = TL.U[np.dtype(dtname)]
        y, pd, al = ref["y"], ref["pd"], ref["alpha"]

        def outputs(pd_w, al_w):
            return dict(mean=(y - al_w / pd_w[:, None, :]).reshape(-1), var=(1 / pd_w).reshape(-1),
                        logpl=((0.5 * np.log(pd_w)[:, None, :] - 0.5 * al_w ** 2 / pd_w[:, None, :]).sum(axis=2) - 0.5 * n * TL.LOG2PI).reshape(-1))

        def fails(out, names):
            rs = TL.ratios(out, ref, n, u)
            for k in names:
                assert rs[k].max() > 1, (n, dtname, k, float(rs[k].max()))

        # the zero-mean answer: Kinv for P, Kinv y for alpha
        fails(outputs(ref["kd"], ref["Ky"]), TL.OUTPUTS)
        # one basis vector dropped
        Hd = np.ascontiguousarray(np.asarray(Hs).reshape(-1, K, n)[:, :K - 1]).reshape(-1) if K > 1 else None
        if Hd is not None:
            rd = TL.reference(T.reference(T.basis_model(T.model(B, c, n), Hd, n, K - 1), T.first(Ys, n, TL.DMAX, D), None, None, None, n,
                                          K - 1, D, 0), n, check_leverage=False)
            fails(outputs(rd["pd"], rd["alpha"]), TL.OUTPUTS)
        # alpha not detrended, P right
        fails(outputs(pd, ref["Ky"]), ("mean", "logpl"))
        # and the right answer passes
        TL.check(outputs(pd, al), ref, n, u, what="exact")


@pytest.mark.parametrize("n", [2, 17, 64, 96, 97])
def test_exact_degenerate_inputs_give_zero_in_both_precisions(n):
    for dt in (np.float32, np.float64):
        for cols in TL.degenerate_columns(n):
            pd = TL.model_order_pd(n, cols, dt)
            zero = np.flatnonzero(pd == 0)
            assert sorted(zero) == sorted(cols) and (np.delete(pd, zero) == 1).all(), (n, dt, cols, pd)
