"""GPU tests of GP prediction from coordinates (matinv_ard_predict_batched): mean and var against float64 numpy (bounds derived in
tests/_ard_predict_worker.py, not fitted) for both covariance functions, the identity at the training points that ties the call to
ard_logml_batched, agreement with predict_batched on torch-built matrices, equal bits over which outputs are requested, shared inputs,
the host form, the batch, the number of queries and their order, the not-positive-definite and NaN-query contracts, and grid rounds and
workspace chunks."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _ard_predict_worker as AP
import _ard_worker as A
from conftest import pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
api = pkg("api")
U = AP.U
DTYPES = (np.float64, np.float32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu(n, X, y, theta, Xq, kind, want=AP.OUTPUTS, d=None):
    """(dict of numpy outputs, info)"""
    return AP.run(api, torch, n, X, y, theta, Xq, kind, want=want, d=d)


def name_of(dt, kind, n):
    name = api.ard_predict_kernel_name(dt, kind, n)
    assert name.startswith("matinv_logdet_tile_f" if n <= 96 else "matinv_logdet_global<") and name.endswith(", true, true>")
    return name


def accuracy(n, d, dt, kind, qs=AP.QS):
    X, y, th, Xq, ref = AP.case(n, d, np.dtype(dt).name, kind)
    worst = {}
    for Q in qs:
        out, info = gpu(n, X, y, th, Xq[:, :Q], kind)
        assert not info.any(), (n, d, Q, dt, kind, info)
        assert all(v.dtype == np.dtype(dt) and v.size == th.shape[0] * Q for v in out.values())
        for k, v in AP.check(out, AP.first_queries(ref, Q), n, dt, what=f"{name_of(dt, kind, n)} d={d}").items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


@pytest.mark.parametrize("n", A.TILE_SIZES + A.GLOBAL_SIZES)
def test_accuracy(n):
    worst = {}
    for dt in DTYPES:
        for kind in A.KINDS:
            for d in AP.DIMS:
                for k, v in accuracy(n, d, dt, kind).items():
                    worst[(np.dtype(dt).name, k)] = max(worst.get((np.dtype(dt).name, k), 0.0), v)
    print(f"n={n} worst err/bound: " + " ".join(f"{a}:{k}={v:.4f}" for (a, k), v in sorted(worst.items())))


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
def test_accuracy_1024(dt):
    accuracy(1024, A.DIM_1024, dt, A.SE if dt is np.float64 else A.MATERN52, qs=(AP.QMAX,))


@pytest.mark.parametrize("n", [1, 17, 33, 64, 96, 130])
def test_identity_at_the_training_points(n):
    """queries ON training points: a_j is column i of M without the noise, so mean_j = (M alpha)_i - sn2 alpha_i = y_i - sn2 alpha_i with
    the alpha of ard_logml_batched. The two sides meet within the sum of the bound of mean and of sn2 times the bound of alpha, plus
    the float64 rounding of forming the right-hand side here (exp, product, difference: 3 u64 |sn2 alpha_i| + u64 |rhs|): no numpy
    reference of the outputs is involved"""
    d = 3
    u64 = U[np.dtype(np.float64)]
    pts = sorted({0, min(15, n - 1), min(16, n - 1), n - 1} | {min(16 * t + 7, n - 1) for t in range((n + 15) // 16)})
    for dt in DTYPES:
        for kind in A.KINDS:
            u = U[np.dtype(dt)]
            X, y, th, aref = A.case(n, d, np.dtype(dt).name, kind)
            batch = th.shape[0]
            Xq = np.ascontiguousarray(X[:, pts])
            out, info = gpu(n, X, y, th, Xq, kind, want=("mean",))
            assert not info.any()
            alpha = A.run(api, torch, n, X, y, th, kind, want=("alpha",))[0]["alpha"].reshape(batch, n).astype(np.float64)
            ref = AP.reference(X, y, th, Xq, n, d, len(pts), kind, u, dt)
            assert all((ref["a"][:, j, i] == ref["sf2"] * A.element(np.float64(0.0), kind)[0]).all() for j, i in enumerate(pts))
            b_mean, _ = AP.bounds(ref, n, u)
            b_alpha = A.bounds(aref, n, d, kind, u, dt)["alpha"]
            sn2 = np.exp(th[:, d + 1].astype(np.float64))[:, None]
            rhs = y[:, pts].astype(np.float64) - sn2 * alpha[:, pts]
            slack = b_mean + sn2 * b_alpha[:, pts] + u64 * (3 * np.abs(sn2 * alpha[:, pts]) + np.abs(rhs))
            diff = np.abs(out["mean"].reshape(batch, -1).astype(np.float64) - rhs)
            print(f"  identity n={n} {np.dtype(dt).name} kind={kind}: worst diff/slack {float((diff / slack).max()):.4f}")
            assert (diff <= slack).all(), (n, dt, kind, float((diff / slack).max()))


@pytest.mark.parametrize("n", [16, 64, 96, 130])
def test_agreement_with_the_existing_route(n):
    """M, A and the prior variances built in torch float64 from the same inputs, rounded to the dtype, through predict_batched: each
    side is within its own bound of the reference (the rounding of those inputs is below the generation error the bounds hold), so the
    two sides lie within the sum of their bounds"""
    d, Q = 2, 17
    for dt in DTYPES:
        for kind in A.KINDS:
            u = U[np.dtype(dt)]
            X, y, th, Xq, _ = AP.case(n, d, np.dtype(dt).name, kind)
            Xq = Xq[:, :Q]
            ref = AP.reference(X, y, th, Xq, n, d, Q, kind, u, dt)
            out, info = gpu(n, X, y, th, Xq, kind)
            assert not info.any()
            t64 = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")  # noqa: E731
            tX, tQ, tth = t64(X), t64(Xq), t64(th)
            sf2, ell, sn2 = tth[:, 0].exp(), tth[:, 1:d + 1].exp(), tth[:, d + 1].exp()
            z, zq = tX / ell[:, None, :], tQ / ell[:, None, :]

            def phi(s):
                if kind == A.SE:
                    return torch.exp(-0.5 * s)
                a = torch.sqrt(5.0 * s)
                return (1.0 + a + 5.0 / 3.0 * s) * torch.exp(-a)

            tdt = torch.float64 if dt is np.float64 else torch.float32
            M = sf2[:, None, None] * phi(((z[:, :, None, :] - z[:, None, :, :]) ** 2).sum(dim=3)) + \
                sn2[:, None, None] * torch.eye(n, device="cuda", dtype=torch.float64)
            Aq = sf2[:, None, None] * phi(((zq[:, :, None, :] - z[:, None, :, :]) ** 2).sum(dim=3))  # (batch, Q, n)
            E = sf2[:, None].expand(-1, Q)
            c = lambda x: x.to(tdt).contiguous().reshape(-1)  # noqa: E731
            mean, var = api.predict_batched(n, c(M), None, c(t64(y)), c(Aq), c(E))
            torch.cuda.synchronize()
            other = dict(mean=mean.cpu().numpy(), var=var.cpu().numpy())
            AP.check(other, ref, n, dt, what=f"existing route n={n}")
            for k, b in zip(AP.OUTPUTS, AP.bounds(ref, n, u)):
                diff = np.abs(out[k].reshape(-1, Q).astype(np.float64) - other[k].reshape(-1, Q).astype(np.float64))
                assert (diff <= 2 * b).all(), (n, dt, kind, k, float((diff / b).max()))


@pytest.mark.parametrize("n", [33, 96, 130])
def test_bits_over_requests_queries_and_batch(n):
    d = 3
    for dt in DTYPES:
        for kind in A.KINDS:
            X, y, th, Xq, _ = AP.case(n, d, np.dtype(dt).name, kind)
            batch, Q = th.shape[0], AP.QMAX
            out, info = gpu(n, X, y, th, Xq, kind)
            assert not info.any()
            both = {k: v.reshape(batch, Q) for k, v in out.items()}
            # mean alone, var alone (then y is not needed)
            o, i = gpu(n, X, y, th, Xq, kind, want=("mean",))
            AP.same_bits(o, {"mean": out["mean"]}, (n, dt, kind, "mean alone"))
            for yy in (y, None):
                o, i = gpu(n, X, yy, th, Xq, kind, want=("var",))
                AP.same_bits(o, {"var": out["var"]}, (n, dt, kind, "var alone"))
                assert not i.any()
            # a matrix alone
            k1 = batch - 2
            o1, i1 = gpu(n, X[k1:k1 + 1], y[k1:k1 + 1], th[k1:k1 + 1], Xq[k1:k1 + 1], kind)
            AP.same_bits(o1, {k: v[k1] for k, v in both.items()}, (n, dt, kind, "matrix alone"))
            assert i1[0] == 0
            # Q = 33 against its first 17, 16 and 1
            for q in (17, 16, 1):
                oq, _ = gpu(n, X, y, th, Xq[:, :q], kind)
                AP.same_bits(oq, {k: np.ascontiguousarray(v[:, :q]) for k, v in both.items()}, (n, dt, kind, "first queries", q))
            # a permutation of the queries permutes the outputs
            pp = np.random.default_rng(5).permutation(Q)
            op, _ = gpu(n, X, y, th, Xq[:, pp], kind)
            AP.same_bits(op, {k: np.ascontiguousarray(v[:, pp]) for k, v in both.items()}, (n, dt, kind, "queries permuted"))


@pytest.mark.parametrize("n", [33, 96, 130])
def test_shared_inputs_and_host_form(n):
    """one point set, target vector and query set for the batch (stride 0) against the same inputs replicated, in every combination the
    strides allow, and the host form against the device form: equal bits"""
    d, batch, Q = 3, 7, 17
    for dt in DTYPES:
        kind = A.MATERN52 if dt is np.float64 else A.SE
        X, y, th = A.inputs(n, d, batch, dt, shared=True)
        Xq = AP.queries(n, d, batch, Q, dt, shared=True)
        rep = lambda x: np.repeat(x, batch, axis=0)  # noqa: E731
        full, ifull = gpu(n, rep(X), rep(y), th, rep(Xq), kind)
        assert not ifull.any()
        AP.check(full, AP.reference(X, y, th, Xq, n, d, Q, kind, U[np.dtype(dt)], dt), n, dt, what=name_of(dt, kind, n) + " shared")
        for sx in (True, False):
            for sy in (True, False):
                for sq in (True, False):
                    o, i = gpu(n, X[0] if sx else rep(X), y[0] if sy else rep(y), th, Xq[0] if sq else rep(Xq), kind, d=d)
                    AP.same_bits(o, full, (n, dt, "shared", sx, sy, sq))
                    assert not i.any()
        mean, var, info = api.ard_predict_batched_host(n, X[0], y[0], th, Xq[0], kind=kind)
        assert not info.any()
        AP.same_bits(dict(mean=mean, var=var), full, (n, dt, "host, shared"))
        mean, var, info = api.ard_predict_batched_host(n, rep(X), rep(y), th, rep(Xq), kind=kind)
        AP.same_bits(dict(mean=mean, var=var), full, (n, dt, "host"))
        mean, var, info = api.ard_predict_batched_host(n, rep(X), None, th, Xq[0], kind=kind, want=("var",))
        assert mean is None and not info.any() and np.array_equal(var, full["var"])


@pytest.mark.parametrize("n", [17, 64, 96, 100])
def test_rejects(n):
    """a NaN coordinate in training point j of three matrices (j at the first column, in a middle tile, at the last column): info is
    ard_logml_batched's, every output of those matrices NaN, the neighbours keep their bits. A NaN coordinate in a query: that query NaN,
    info 0, every other query keeps its bits"""
    d, Q = 2, 17
    for dt in DTYPES:
        for kind in A.KINDS:
            X, y, th, Xq, _ = AP.case(n, d, np.dtype(dt).name, kind)
            Xq = Xq[:, :Q]
            batch = th.shape[0]
            out, _ = gpu(n, X, y, th, Xq, kind)
            Xb, want_info = AP.nan_points(X, n, {1: 0, 3: n // 2 + 3, 4: n - 1})
            assert want_info == {1: 1, 3: n // 2 + 4, 4: n}
            ob, info = gpu(n, Xb, y, th, Xq, kind)
            AP.check_with_rejects(ob, info, Xb, y, th, Xq, n, d, Q, kind, dt, want_info, name_of(dt, kind, n) + " rejects")
            assert np.array_equal(info, A.run(api, torch, n, Xb, y, th, kind, want=("logml",))[1])
            ok = [k for k in range(batch) if k not in want_info]
            for k in AP.OUTPUTS:  # the neighbours keep their bits; each output alone is NaN there as well
                assert np.array_equal(ob[k].reshape(batch, -1)[ok], out[k].reshape(batch, -1)[ok]), (n, dt, k)
                o1, i1 = gpu(n, Xb, y, th, Xq, kind, want=(k,))
                assert np.array_equal(i1, info) and np.array_equal(o1[k], ob[k], equal_nan=True), (n, dt, k)
            # NaN queries: the first of a group, the last of a group, the last of all
            Xn = np.array(Xq)
            hit = {0: 0, 2: 15, batch - 1: Q - 1}
            for k, j in hit.items():
                Xn[k, j, 0] = np.nan
            on, i_n = gpu(n, X, y, th, Xn, kind)
            assert not i_n.any()
            mask = np.zeros((batch, Q), dtype=bool)
            for k, j in hit.items():
                mask[k, j] = True
            for k in AP.OUTPUTS:
                got, clean = on[k].reshape(batch, Q), out[k].reshape(batch, Q)
                assert np.isnan(got[mask]).all() and np.array_equal(got[~mask], clean[~mask]), (n, dt, kind, k)


def test_grid_stride_and_chunking(tmp_path):
    """the calls of _ard_predict_worker.STRIDE_CASES under the default switches, checked against the reference and saved; then one
    process with the grid held to one round of resident workgroups and the workspace cap at 1 MiB must give the same bits"""
    saved = {}
    for i, (n, d, Q, batch, dt, kind, shared, rejects) in enumerate(AP.STRIDE_CASES):
        X, y, th, Xq, want_info = AP.stride_inputs(n, d, Q, batch, dt, kind, shared, rejects)
        s = (lambda x: x[0]) if shared else (lambda x: x)
        out, info = gpu(n, s(X), s(y), th, s(Xq), kind, d=d)
        AP.check_with_rejects(out, info, X, y, th, Xq, n, d, Q, kind, dt, want_info, f"{name_of(dt, kind, n)} batch={batch}", sample=200)
        saved[AP.stride_key(i, "info")] = info
        for k, v in out.items():
            saved[AP.stride_key(i, k)] = v
    path = os.path.join(tmp_path, "default_call.npz")
    np.savez(path, **saved)
    e = dict(os.environ)
    e.update({"MATINV_TILE_GRID_MULT": "1", "MATINV_BLOCKED_WS_MB": "1"})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_ard_predict_worker.py"), path], capture_output=True, text=True, env=e,
                       timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "ard-predict-worker ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
