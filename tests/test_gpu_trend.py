"""GPU tests of the GP regression with a linear trend (matinv_trend_batched): all seven outputs against float64 / longdouble numpy (bounds
derived in tests/_trend_worker.py, not fitted), which outputs are requested, bit locality (target and query position, D, Q, Y, batch, grid
rounds, workspace chunks), the not-positive-definite and the rank-deficient contract, the agreement with the composed route and with
centring for a constant trend, and the host form.

Worst err / bound seen on an MI355X is printed by every run ("Regression with a linear trend", Accuracy)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _trend_worker as T
from conftest import pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
api = pkg("api")
lib = pkg("_lib")
U = T.U
DTYPES = (np.float64, np.float32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER = dict(beta=None, alpha=None, quad=1, logml=1, mean=T.QMAX)  # elements per target (beta: K, alpha: n)


def gpu(n, B, c, Hs, Ys, As, Gs, Es, want=T.OUTPUTS, **kw):
    """(dict of numpy outputs, info)"""
    return T.run(api, torch, n, B, c, Hs, Ys, As, Gs, Es, want=want, **kw)


def name_of(dt, n):
    name = api.trend_kernel_name(dt, n)
    assert name.startswith("matinv_spd_tile_f" if n <= 96 else "matinv_chol_global<")
    assert name.endswith(", true" * 10 + ">")
    return name


def accuracy(n, dt, with_c, shapes):
    for K, D, Q in shapes:
        cs = T.case(n, np.dtype(dt).name, with_c, K)
        out, info = gpu(n, cs[0], cs[1], *T.inputs_of(cs, n, K, D, Q), K=K, D=D, Q=Q)
        assert not info.any(), (n, dt, info)
        assert all(v.dtype == np.dtype(dt) for v in out.values())
        T.check(out, T.take(cs[7], D, Q), n, U[np.dtype(dt)], what=name_of(dt, n) + (" c" if with_c else ""))
        cb = out["covbeta"].reshape(-1, K, K)
        assert np.array_equal(cb, cb.transpose(0, 2, 1)), (n, dt, K)  # bitwise symmetric


@pytest.mark.parametrize("n", T.TILE_SIZES + T.GLOBAL_SIZES)
def test_accuracy(n):
    for dt in DTYPES:
        for with_c in (True, False):
            accuracy(n, dt, with_c, T.shapes_of(n))


@pytest.mark.parametrize("dt", DTYPES)
def test_accuracy_1024(dt):
    accuracy(1024, dt, True, (T.KDQ_1024,))


@pytest.mark.parametrize("n", [33, 64, 96, 130])
def test_optional_outputs(n):
    for dt in DTYPES:
        K, D, Q = 3, 17, 16
        cs = T.case(n, np.dtype(dt).name, True, K)
        B, c = cs[0], cs[1]
        Hs, y, a, g, e = T.inputs_of(cs, n, K, D, Q)
        out, info = gpu(n, B, c, Hs, y, a, g, e)
        assert not info.any()
        # each output alone and a few pairs, with only the inputs they need: the bits of the all-outputs call
        for want in [(k,) for k in T.OUTPUTS] + [("alpha", "mean"), ("beta", "var"), ("covbeta", "logml")]:
            targets = bool(set(want) & {"beta", "alpha", "quad", "logml", "mean"})
            queries = bool(set(want) & {"mean", "var"})
            o, i = gpu(n, B, c, Hs, y if targets else None, a if queries else None, g if queries else None,
                       e if "var" in want else None, want=want, K=K)
            T.same_bits(o, {k: out[k] for k in want}, (n, dt, want))
            assert not i.any()
        # the raw C entry point on tensors larger than the call: the tails and the info tail stay as they were; covbeta alone with
        # dYs = dAs = NULL and ntarget = nquery = 0
        batch = B.size // (n * n)
        sizes = dict(beta=batch * D * K, covbeta=batch * K * K, alpha=batch * D * n, quad=batch * D, logml=batch * D, mean=batch * D * Q,
                     var=batch * Q)
        t = lambda x: torch.tensor(np.ascontiguousarray(x)).cuda()  # noqa: E731
        ins = [t(x) for x in (B, c, Hs, y, a, g, e)]
        outs = {k: torch.full((sizes[k] + 7,), -7.5, dtype=ins[0].dtype, device="cuda") for k in T.OUTPUTS}
        info = torch.full((batch + 3,), -7, dtype=torch.int32, device="cuda")
        alone = torch.full((sizes["covbeta"] + 7,), -7.5, dtype=ins[0].dtype, device="cuda")
        ptr = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
        code = api.F64 if dt is np.float64 else api.F32
        torch.cuda.synchronize()
        rc = lib.lib().matinv_trend_batched(code, n, K, D, Q, *[ptr(x) for x in ins], *[ptr(outs[k]) for k in T.OUTPUTS], batch, ptr(info),
                                            None)
        rc2 = lib.lib().matinv_trend_batched(code, n, K, 0, 0, ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), None, None, None, None, None,
                                             ptr(alone), None, None, None, None, None, batch, None, None)
        torch.cuda.synchronize()
        assert rc == lib.OK and rc2 == lib.OK
        for k in T.OUTPUTS:
            got = outs[k].cpu().numpy()
            assert np.array_equal(got[:sizes[k]], out[k]) and (got[sizes[k]:] == -7.5).all(), (n, dt, k)
        got = alone.cpu().numpy()
        assert np.array_equal(got[:sizes["covbeta"]], out["covbeta"]) and (got[sizes["covbeta"]:] == -7.5).all(), (n, dt)
        got = info.cpu().numpy()
        assert not got[:batch].any() and (got[batch:] == -7).all()


@pytest.mark.parametrize("n", [33, 64, 95, 130])
def test_locality(n):
    for dt in DTYPES:
        K = 4
        cs = T.case(n, np.dtype(dt).name, True, K)
        B, c, Hs, Ys, As, Gs, Es, _ = cs
        batch = B.size // (n * n)
        out, info = gpu(n, B, c, Hs, Ys, As, Gs, Es, K=K)  # D = 33, Q = 33
        assert not info.any()
        per = dict(PER, beta=K, alpha=n)
        o33 = {k: out[k].reshape(batch, T.DMAX, per[k]) for k in per}
        fixed = ("covbeta", "var")  # depend on neither D nor Y
        # a target alone gives the bits it has as target 0, 15, 16 and 32 of D = 33
        for t in (0, 15, 16, 32):
            o1, _ = gpu(n, B, c, Hs, T.first(Ys, n, T.DMAX, [t]), As, Gs, Es, K=K)
            for k in per:
                assert np.array_equal(o1[k].reshape(batch, per[k]), o33[k][:, t]), (n, dt, t, k)
            for k in fixed:
                assert np.array_equal(o1[k], out[k]), (n, dt, t, k)
        # ... and targets 16 .. 32 as a call of their own, in other lanes and another group
        o17, _ = gpu(n, B, c, Hs, T.first(Ys, n, T.DMAX, slice(16, 33)), As, Gs, Es, K=K)
        for k in per:
            assert np.array_equal(o17[k].reshape(batch, 17, per[k]), o33[k][:, 16:]), (n, dt, k)
        # var and covbeta without any target, and with other targets
        o0, _ = gpu(n, B, c, Hs, None, As, Gs, Es, want=fixed, K=K)
        T.same_bits(o0, {k: out[k] for k in fixed}, (n, dt, "no targets"))
        other = T.vectors(n, batch, K, 5, 1, dt, 31 + n)[1]
        o5, _ = gpu(n, B, c, Hs, other, As, Gs, Es, K=K)
        T.same_bits({k: o5[k] for k in fixed}, {k: out[k] for k in fixed}, (n, dt, "other targets"))
        # the same for the queries, in mean and in var
        m33, v33 = o33["mean"], out["var"].reshape(batch, T.QMAX)
        pick = lambda j: (T.first(As, n, T.QMAX, j), T.first(Gs, K, T.QMAX, j), T.first(Es, 1, T.QMAX, j))  # noqa: E731
        for j in (0, 15, 16, 32):
            o1, _ = gpu(n, B, c, Hs, Ys, *pick([j]), want=("mean", "var"), K=K)
            assert np.array_equal(o1["mean"].reshape(batch, T.DMAX), m33[:, :, j]), (n, dt, j)
            assert np.array_equal(o1["var"].reshape(batch), v33[:, j]), (n, dt, j)
        o17, _ = gpu(n, B, c, Hs, Ys, *pick(slice(16, 33)), want=("mean", "var"), K=K)
        assert np.array_equal(o17["mean"].reshape(batch, T.DMAX, 17), m33[:, :, 16:]), (n, dt)
        assert np.array_equal(o17["var"].reshape(batch, 17), v33[:, 16:]), (n, dt)
        # matrix k alone
        k1 = batch - 2
        row = lambda x: x.reshape(batch, -1)[k1]  # noqa: E731
        ok, ik = gpu(n, *(row(x) for x in (B, c, Hs, Ys, As, Gs, Es)), K=K)
        T.same_bits(ok, {k: row(v) for k, v in out.items()}, (n, dt, "matrix alone"))
        assert ik[0] == 0
        cb = out["covbeta"].reshape(batch, K, K)
        assert np.array_equal(cb, cb.transpose(0, 2, 1))


@pytest.mark.parametrize("n", [17, 64, 100])
def test_not_positive_definite(n):
    """_loo_worker.break_three on M gives info n, 2, 1. Matrix 2 has h_2 = h_1 bit for bit (K = 3), so A is singular: asserted for BOTH
    dtypes is info == n + 2 exactly, not only n < info <= n + K. The reason: with two identical basis vectors the kernels form A_11, A_21
    and A_22 by the same operations on the same operands, so the three are equal bit for bit, and the factorisation of A updates with the
    IEEE quotient A_21 / A_11, which is exactly 1: pivot 2 is exactly 0 in either precision, whatever a float64 factorisation that
    squares a rounded L_21 would find."""
    K, D, Q = 3, 17, 16
    for dt in DTYPES:
        for with_c in (True, False):
            cs = T.case(n, np.dtype(dt).name, with_c, K)
            B, c = cs[0], cs[1]
            Hs, y, a, g, e = T.inputs_of(cs, n, K, D, Q)
            out, _ = gpu(n, B, c, Hs, y, a, g, e)
            Bb, cb, Hb = np.array(B), (None if c is None else np.array(c)), np.array(Hs)
            want_info = T.break_three(Bb, cb, n, (1, 3, 4))
            assert want_info == {1: n, 3: 2, 4: 1}
            batch = B.size // (n * n)
            Hb.reshape(batch, K, n)[2, 1] = Hb.reshape(batch, K, n)[2, 0]
            ob, info = gpu(n, Bb, cb, Hb, y, a, g, e)
            assert info[2] == n + 2, (n, dt, info)
            T.check_with_rejects(ob, info, Bb, cb, Hb, y, a, g, e, n, K, D, Q, dt, want_info, name_of(dt, n) + " rejects", singular=(2,))
            # the neighbours keep their bits
            ok = [k for k in range(batch) if k not in want_info and k != 2]
            for k in T.OUTPUTS:
                assert np.array_equal(ob[k].reshape(batch, -1)[ok], out[k].reshape(batch, -1)[ok]), (n, dt, k)
            # each output alone reports the same info and is NaN there as well
            for k in T.OUTPUTS:
                targets, queries = k in ("beta", "alpha", "quad", "logml", "mean"), k in ("mean", "var")
                o1, i1 = gpu(n, Bb, cb, Hb, y if targets else None, a if queries else None, g if queries else None,
                             e if k == "var" else None, want=(k,), K=K)
                assert np.array_equal(i1, info) and np.array_equal(o1[k], ob[k], equal_nan=True), (n, dt, k)


def composed(n, dt, B, c, Hs, y, a, g, e, K, D, Q):
    """the route a user had before: multi_target_batched on [H | Y] for Kinv [H | Y] and log det M, predict_batched for e - a^T Kinv a,
    and the K x K algebra in float64 numpy"""
    batch = B.size // (n * n)
    t = lambda x: torch.tensor(np.ascontiguousarray(x)).cuda()  # noqa: E731
    hy = np.concatenate([Hs.reshape(batch, K, n), y.reshape(batch, D, n)], axis=1).reshape(-1)
    al, _, ld, _, _ = api.multi_target_batched(n, t(B), t(c), t(hy), want=("alpha", "logdet"))
    _, pv = api.predict_batched(n, t(B), t(c), None, t(a), t(e), want=("var",))
    torch.cuda.synchronize()
    f = np.float64
    sol = al.cpu().numpy().astype(f).reshape(batch, K + D, n)
    KH, Ky = sol[:, :K].transpose(0, 2, 1), sol[:, K:]
    H, yy = Hs.astype(f).reshape(batch, K, n).transpose(0, 2, 1), y.astype(f).reshape(batch, D, n)
    aa, gg = a.astype(f).reshape(batch, Q, n), g.astype(f).reshape(batch, Q, K)
    A = H.transpose(0, 2, 1) @ KH
    Ainv = np.linalg.inv((A + A.transpose(0, 2, 1)) / 2)
    beta = np.einsum("kbc,kic,kti->ktb", Ainv, H, Ky)
    alpha = Ky - np.einsum("kib,ktb->kti", KH, beta)
    quad = np.einsum("kti,kti->kt", yy, alpha)
    logml = -(quad + (ld.cpu().numpy().astype(f) + np.linalg.slogdet(A)[1])[:, None] + (n - K) * T.LOG2PI) / 2
    r = gg - np.einsum("kib,kqi->kqb", KH, aa)
    return dict(beta=beta, covbeta=Ainv, alpha=alpha, quad=quad, logml=logml,
                mean=np.einsum("kqi,kti->ktq", aa, alpha) + np.einsum("kqb,ktb->ktq", gg, beta),
                var=pv.cpu().numpy().astype(f).reshape(batch, Q) + np.einsum("kqb,kbc,kqc->kq", r, Ainv, r))


@pytest.mark.parametrize("n", [16, 64, 96, 130])
def test_agreement_with_the_composed_route(n):
    """each side is within one bound of the reference, so they are within two of each other"""
    K, D, Q = 3, 17, 16
    for dt in DTYPES:
        cs = T.case(n, np.dtype(dt).name, True, K)
        B, c = cs[0], cs[1]
        inp = T.inputs_of(cs, n, K, D, Q)
        out, info = gpu(n, B, c, *inp)
        assert not info.any()
        other = composed(n, dt, B, c, *inp, K, D, Q)
        ref = T.take(cs[7], D, Q)
        u = U[np.dtype(dt)]
        T.check({k: v.reshape(-1) for k, v in other.items()}, ref, n, u, what=f"composed route n={n}")
        b = T.bounds(ref, n, u)
        shp = T.shapes(ref, n)
        for k, v in other.items():
            diff = np.abs(out[k].reshape(shp[k]).astype(np.float64) - v.reshape(shp[k]))
            assert (diff <= 2 * b[k]).all(), (n, dt, k, float((diff / b[k]).max()))


@pytest.mark.parametrize("n", [16, 64, 96, 130])
def test_constant_trend_against_centring(n):
    """K = 1, h = 1, g = 1: mean equals multi_target_batched on y - beta 1, plus beta, within two bounds"""
    K, D, Q = 1, 17, 16
    for dt in DTYPES:
        cs = T.case(n, np.dtype(dt).name, True, K)
        B, c = cs[0], cs[1]
        Hs, y, a, g, e = T.inputs_of(cs, n, K, D, Q)
        assert (Hs == 1).all() and (g == 1).all()
        out, info = gpu(n, B, c, Hs, y, a, g, e, want=("beta", "mean"))
        assert not info.any()
        batch = B.size // (n * n)
        beta = out["beta"].reshape(batch, D, 1)
        centred = (y.reshape(batch, D, n) - beta).astype(dt).reshape(-1)
        t = lambda x: torch.tensor(np.ascontiguousarray(x)).cuda()  # noqa: E731
        res = api.multi_target_batched(n, t(B), t(c), t(centred), t(a), want=("mean",))
        torch.cuda.synchronize()
        mean = res[4].cpu().numpy().reshape(batch, D, Q).astype(np.float64) + beta.astype(np.float64)
        ref = T.take(cs[7], D, Q)
        b = T.bounds(ref, n, U[np.dtype(dt)])["mean"]
        diff = np.abs(out["mean"].reshape(batch, D, Q).astype(np.float64) - mean)
        print(f"  centring n={n} {np.dtype(dt).name}: worst diff / bound {float((diff / b).max()):.4f}")
        assert (diff <= 2 * b).all(), (n, dt, float((diff / b).max()))


@pytest.mark.parametrize("n", [40, 100])
def test_host_form_equals_device_form(n):
    K, D, Q = 3, 17, 16
    for dt in DTYPES:
        cs = T.case(n, np.dtype(dt).name, True, K)
        B, c = cs[0], cs[1]
        inp = T.inputs_of(cs, n, K, D, Q)
        out, _ = gpu(n, B, c, *inp)
        res = api.trend_batched_host(n, B, c, *inp)
        assert not res[7].any()
        T.same_bits(dict(zip(T.OUTPUTS, res[:7])), out, (n, dt, "host"))
        res = api.trend_batched_host(n, B, c, inp[0], want=("covbeta",))
        assert all(res[i] is None for i in (0, 2, 3, 4, 5, 6)) and not res[7].any() and np.array_equal(res[1], out["covbeta"])


def test_grid_stride_and_chunking():
    """one process with the grid held to one round of resident workgroups and the workspace cap at 1 MiB: tests/_trend_worker.py"""
    e = dict(os.environ)
    e.update({"MATINV_TILE_GRID_MULT": "1", "MATINV_BLOCKED_WS_MB": "1"})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_trend_worker.py")], capture_output=True, text=True, env=e, timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "trend-worker ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
