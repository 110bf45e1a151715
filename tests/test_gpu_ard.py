"""GPU tests of the GP log marginal likelihood and its gradient from coordinates (matinv_ard_logml_batched): the three outputs against
longdouble / float64 numpy (bounds derived in tests/_ard_worker.py, not fitted) for both covariance functions, shared inputs, which
outputs are requested, bit locality and the symmetries of the model, the tile-edge structure (a diagonal matrix plus one 2 x 2 block at
every tile edge, against its closed form), the ties to logml_batched and logml_grad_batched on numpy-generated matrices, the
not-positive-definite contract, the host form, and grid rounds and workspace chunks."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _ard_worker as A
from conftest import pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
api = pkg("api")
lib = pkg("_lib")
U = A.U
DTYPES = (np.float64, np.float32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = ", true" * 13 + ">"


def gpu(n, X, y, theta, kind, want=A.OUTPUTS, d=None):
    """(dict of numpy outputs, info)"""
    return A.run(api, torch, n, X, y, theta, kind, want=want, d=d)


def name_of(dt, kind, n):
    name = api.ard_logml_kernel_name(dt, kind, n)
    assert name.startswith("matinv_spd_tile_f" if n <= 96 else "matinv_chol_global<") and name.endswith(TAIL)
    return name


def accuracy(n, d, dt, kind):
    X, y, th, ref = A.case(n, d, np.dtype(dt).name, kind)
    out, info = gpu(n, X, y, th, kind)
    assert not info.any(), (n, d, dt, kind, info)
    assert all(v.dtype == np.dtype(dt) for v in out.values())
    return A.check(out, ref, n, d, kind, dt, what=name_of(dt, kind, n))


@pytest.mark.parametrize("n", A.TILE_SIZES + A.GLOBAL_SIZES)
def test_accuracy(n):
    worst = {}
    for dt in DTYPES:
        for kind in A.KINDS:
            for d in A.DIMS:
                for k, v in accuracy(n, d, dt, kind).items():
                    worst[(np.dtype(dt).name, k)] = max(worst.get((np.dtype(dt).name, k), 0.0), v)
    print(f"n={n} worst err/bound: " + " ".join(f"{a}:{k}={v:.4f}" for (a, k), v in sorted(worst.items())))


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
def test_accuracy_1024(dt):
    accuracy(1024, A.DIM_1024, dt, A.SE if dt is np.float64 else A.MATERN52)


@pytest.mark.parametrize("n", [33, 96, 130])
def test_shared_inputs(n):
    """one point set and one target vector for the batch (stride 0) against the same inputs replicated: equal bits"""
    d, batch = 3, 7
    for dt in DTYPES:
        for kind in A.KINDS:
            X, y, th = A.inputs(n, d, batch, dt, shared=True)
            out, info = gpu(n, X[0], y[0], th, kind, d=d)
            assert not info.any()
            rep, irep = gpu(n, np.repeat(X, batch, axis=0), np.repeat(y, batch, axis=0), th, kind)
            A.same_bits(out, rep, (n, dt, kind, "shared"))
            assert not irep.any()
            # shared points with per-matrix targets, and the other way round
            _, yb, _ = A.inputs(n, d, batch, dt, seed=77)
            o1, _ = gpu(n, X[0], yb, th, kind, d=d)
            o2, _ = gpu(n, np.repeat(X, batch, axis=0), yb, th, kind)
            A.same_bits(o1, o2, (n, dt, kind, "shared X"))
            A.check(out, A.reference(X, y, th, n, d, kind), n, d, kind, dt, what=name_of(dt, kind, n) + " shared")


@pytest.mark.parametrize("n", [33, 96, 130])
def test_optional_outputs(n):
    d = 3
    for dt in DTYPES:
        kind = A.MATERN52
        X, y, th, _ = A.case(n, d, np.dtype(dt).name, kind)
        out, info = gpu(n, X, y, th, kind)
        assert not info.any()
        for want in [(k,) for k in A.OUTPUTS] + [("logml", "grad"), ("grad", "alpha"), ("logml", "alpha")]:
            o, i = gpu(n, X, y, th, kind, want=want)
            A.same_bits(o, {k: out[k] for k in want}, (n, dt, want))
            assert not i.any()
        # the raw C entry point on tensors larger than the call: the tails and the info tail stay as they were
        batch = th.shape[0]
        sizes = dict(logml=batch, grad=batch * (d + 2), alpha=batch * n)
        t = lambda x: torch.tensor(np.ascontiguousarray(x)).cuda()  # noqa: E731
        ins = [t(X), t(y), t(th)]
        outs = {k: torch.full((sizes[k] + 7,), -7.5, dtype=ins[0].dtype, device="cuda") for k in A.OUTPUTS}
        info = torch.full((batch + 3,), -7, dtype=torch.int32, device="cuda")
        ptr = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
        torch.cuda.synchronize()
        rc = lib.lib().matinv_ard_logml_batched(api.F64 if dt is np.float64 else api.F32, kind, n, d, ptr(ins[0]), n * d, ptr(ins[1]), n,
                                                ptr(ins[2]), *[ptr(outs[k]) for k in A.OUTPUTS], batch, ptr(info), None)
        torch.cuda.synchronize()
        assert rc == lib.OK
        for k in A.OUTPUTS:
            got = outs[k].cpu().numpy()
            assert np.array_equal(got[:sizes[k]], out[k]) and (got[sizes[k]:] == -7.5).all(), (n, dt, k)
        got = info.cpu().numpy()
        assert not got[:batch].any() and (got[batch:] == -7).all()


@pytest.mark.parametrize("n", [33, 95, 130])
def test_locality_and_symmetry(n):
    d = 3
    for dt in DTYPES:
        for kind in A.KINDS:
            u = U[np.dtype(dt)]
            X, y, th, ref = A.case(n, d, np.dtype(dt).name, kind)
            batch = th.shape[0]
            out, info = gpu(n, X, y, th, kind)
            assert not info.any()
            b = A.bounds(ref, n, d, kind, u, dt)
            shp = A.shapes(n, d)
            # matrix k alone
            k1 = batch - 2
            o1, i1 = gpu(n, X[k1:k1 + 1], y[k1:k1 + 1], th[k1:k1 + 1], kind)
            A.same_bits(o1, {k: v.reshape(batch, -1)[k1] for k, v in out.items()}, (n, dt, kind, "matrix alone"))
            assert i1[0] == 0
            # a coordinate column of zeros appended, with any length scale: no bit of logml, alpha or the other gradients changes, and
            # the new dimension has a gradient of exactly 0
            X0 = np.concatenate([X, np.zeros((batch, n, 1), dtype=dt)], axis=2)
            th0 = np.concatenate([th[:, :d + 1], np.full((batch, 1), 0.37, dtype=dt), th[:, d + 1:]], axis=1)
            o0, i0 = gpu(n, X0, y, th0, kind)
            assert not i0.any()
            g0 = o0["grad"].reshape(batch, d + 3)
            assert np.array_equal(o0["logml"], out["logml"]) and np.array_equal(o0["alpha"], out["alpha"]), (n, dt, kind)
            assert np.array_equal(np.delete(g0, d + 1, axis=1), out["grad"].reshape(batch, d + 2)), (n, dt, kind)
            assert (g0[:, d + 1] == 0).all(), (n, dt, kind)
            # the dimensions permuted consistently: s is summed in another order, grad[1 .. d] permuted, within two bounds
            perm = [2, 0, 1]
            op, _ = gpu(n, X[:, :, perm], y, th[:, [0] + [1 + p for p in perm] + [d + 1]], kind)
            gp = op["grad"].reshape(shp["grad"]).astype(np.float64)
            g = out["grad"].reshape(shp["grad"]).astype(np.float64)
            cols = [0] + [1 + p for p in perm] + [d + 1]
            assert (np.abs(gp - g[:, cols]) <= 2 * b["grad"][:, cols]).all(), (n, dt, kind)
            assert (np.abs(op["logml"].astype(np.float64) - out["logml"].astype(np.float64)) <= 2 * b["logml"]).all()
            # the points permuted consistently with y: logml and grad within two bounds, alpha permuted within two bounds
            pp = np.random.default_rng(5).permutation(n)
            oq, _ = gpu(n, X[:, pp], y[:, pp], th, kind)
            assert (np.abs(oq["grad"].reshape(shp["grad"]).astype(np.float64) - g) <= 2 * b["grad"]).all(), (n, dt, kind)
            assert (np.abs(oq["logml"].astype(np.float64) - out["logml"].astype(np.float64)) <= 2 * b["logml"]).all()
            a = out["alpha"].reshape(batch, n).astype(np.float64)
            assert (np.abs(oq["alpha"].reshape(batch, n).astype(np.float64) - a[:, pp]) <= 2 * b["alpha"][:, pp]).all(), (n, dt, kind)


def edge_pairs(n):
    """(i, j), i > j, on both sides of every 16-wide tile edge, the corners and the last row"""
    pairs = [(n - 1, 0), (1, 0), (n - 1, n - 2)]
    for e in range(16, n, 16):
        pairs += [(e, e - 1), (e, 0), (n - 1, e), (n - 1, e - 1), (e + 1, e) if e + 1 < n else (e, e - 2)]
    return sorted(set(p for p in pairs if p[0] > p[1]))


@pytest.mark.parametrize("n", [33, 96, 130])
def test_tile_edge_structure(n):
    """all points 1000 apart on a plane (s >= 1e6: phi and psi underflow to 0 in both dtypes and both kinds) but one pair (i, j) 0.75
    apart along dimension 0; l = 1 exactly, so z, the difference and s = 0.5625 are exact. M is diagonal plus one 2 x 2 block, one matrix
    of the batch per pair: logml and grad against the closed form of that block, within the bounds"""
    d, side = 2, 12
    pairs = edge_pairs(n)
    batch = len(pairs)
    for dt in DTYPES:
        for kind in A.KINDS:
            rng = np.random.default_rng(31 + n)
            grid = np.stack([1000.0 * (np.arange(n) % side), 1000.0 * (np.arange(n) // side)], axis=1)
            X = np.repeat(grid[None], batch, axis=0)
            for k, (i, j) in enumerate(pairs):
                X[k, i] = X[k, j] + np.array([0.75, 0.0])
            sf2, sn2 = rng.uniform(0.5, 2.0, batch), rng.uniform(0.3, 0.6, batch)
            th = np.stack([np.log(sf2), np.zeros(batch), np.zeros(batch), np.log(sn2)], axis=1).astype(dt)
            X, y = X.astype(dt), rng.standard_normal((batch, n)).astype(dt)
            ref = A.reference(X, y, th, n, d, kind)
            off = ref["M"] - np.einsum("kii->ki", ref["M"])[:, :, None] * np.eye(n)
            assert all(np.count_nonzero(off[k]) == 2 and off[k, i, j] != 0 for k, (i, j) in enumerate(pairs))
            out, info = gpu(n, X, y, th, kind)
            assert not info.any()
            A.check(out, ref, n, d, kind, dt, what=name_of(dt, kind, n) + " one pair")
            # the closed form: singles -1/2 (y^2 / a + log a), the pair through the 2 x 2 inverse
            b = A.bounds(ref, n, d, kind, U[np.dtype(dt)], dt)
            yy = y.astype(np.float64)
            g = out["grad"].reshape(batch, d + 2).astype(np.float64)
            for k, (i, j) in enumerate(pairs):
                a = ref["sf2"][k] + ref["sn2"][k]
                phi, psi, _ = A.element(np.float64(0.5625), kind)
                c = ref["sf2"][k] * phi
                det = a * a - c * c
                ai = (a * yy[k, i] - c * yy[k, j]) / det
                aj = (a * yy[k, j] - c * yy[k, i]) / det
                rest = np.delete(yy[k], [i, j])
                logml = -0.5 * ((rest ** 2).sum() / a + (n - 2) * np.log(a) + yy[k, i] * ai + yy[k, j] * aj + np.log(det) + n * A.LOG2PI)
                assert abs(float(out["logml"][k]) - logml) <= b["logml"][k] + 1e-13 * abs(logml), (n, dt, kind, i, j)
                gl = (ai * aj + c / det) * ref["sf2"][k] * psi * 0.5625  # G_ij dM_1[i, j]: the pair and its mirror, times 1/2
                assert abs(g[k, 1] - gl) <= b["grad"][k, 1] + 1e-13 * abs(gl), (n, dt, kind, i, j, g[k, 1], gl)
                assert g[k, 2] == 0.0, (n, dt, kind, i, j)  # the pair does not differ in dimension 1, and everything else is 0 * finite


@pytest.mark.parametrize("n", [16, 64, 96, 130])
def test_agreement_with_existing_routes(n):
    """logml_batched and logml_grad_batched on the numpy-generated M and dM_p rounded to the dtype: each side is within its own bound of
    the reference (the rounding of their input is below the generation error the bounds of _ard_worker hold), so the two sides lie within
    the sum of their bounds"""
    d = 2
    for dt in DTYPES:
        for kind in A.KINDS:
            X, y, th, ref = A.case(n, d, np.dtype(dt).name, kind)
            batch = th.shape[0]
            out, info = gpu(n, X, y, th, kind)
            assert not info.any()
            t = lambda x: torch.tensor(np.ascontiguousarray(x)).cuda()  # noqa: E731
            M = t(ref["M"].astype(dt).reshape(-1))
            dM = t(ref["dM"].astype(dt).reshape(-1))
            yd = t(y.reshape(-1))
            logml = api.logml_batched(n, M, None, yd)
            grad, _, alpha = api.logml_grad_batched(n, M, None, yd, dM, want=("grad", "alpha"))
            torch.cuda.synchronize()
            other = dict(logml=logml.cpu().numpy(), grad=grad.cpu().numpy(), alpha=alpha.cpu().numpy())
            A.check(other, ref, n, d, kind, dt, what=f"existing routes n={n}")
            b = A.bounds(ref, n, d, kind, U[np.dtype(dt)], dt)
            shp = A.shapes(n, d)
            for k, v in other.items():
                diff = np.abs(out[k].reshape(shp[k]).astype(np.float64) - v.reshape(shp[k]).astype(np.float64))
                assert (diff <= 2 * b[k]).all(), (n, dt, kind, k, float((diff / b[k]).max()))
            assert batch == A.batch_of(n)


@pytest.mark.parametrize("n", [17, 64, 96, 100])
def test_rejects(n):
    """a NaN coordinate in point j of three matrices: j at the first column, in the middle of a tile, at the last column"""
    d = 2
    for dt in DTYPES:
        for kind in A.KINDS:
            X, y, th, _ = A.case(n, d, np.dtype(dt).name, kind)
            out, _ = gpu(n, X, y, th, kind)
            Xb, want_info = A.nan_points(X, n, {1: 0, 3: n // 2 + 3, 4: n - 1})
            assert want_info == {1: 1, 3: n // 2 + 4, 4: n}
            ob, info = gpu(n, Xb, y, th, kind)
            A.check_with_rejects(ob, info, Xb, y, th, n, d, kind, dt, want_info, name_of(dt, kind, n) + " rejects")
            batch = info.size
            ok = [k for k in range(batch) if k not in want_info]
            for k in A.OUTPUTS:  # the neighbours keep their bits
                assert np.array_equal(ob[k].reshape(batch, -1)[ok], out[k].reshape(batch, -1)[ok]), (n, dt, k)
            for k in A.OUTPUTS:  # each output alone is NaN there as well
                o1, i1 = gpu(n, Xb, y, th, kind, want=(k,))
                assert np.array_equal(i1, info) and np.array_equal(o1[k], ob[k], equal_nan=True), (n, dt, k)


@pytest.mark.parametrize("n", [40, 100])
def test_host_form_equals_device_form(n):
    d = 3
    for dt in DTYPES:
        X, y, th, _ = A.case(n, d, np.dtype(dt).name, A.SE)
        out, _ = gpu(n, X, y, th, A.SE)
        lm, g, al, info = api.ard_logml_batched_host(n, X, y, th, kind=A.SE)
        assert not info.any()
        A.same_bits(dict(logml=lm, grad=g, alpha=al), out, (n, dt, "host"))
        lm, g, al, info = api.ard_logml_batched_host(n, X, y, th, kind=A.SE, want=("grad",))
        assert lm is None and al is None and not info.any() and np.array_equal(g, out["grad"])
        # a shared point set is staged once
        Xs, ys, ths = A.inputs(n, d, 5, dt, shared=True)
        o, _ = gpu(n, Xs[0], ys[0], ths, A.MATERN52, d=d)
        lm, g, al, info = api.ard_logml_batched_host(n, Xs[0], ys[0], ths, kind=A.MATERN52)
        A.same_bits(dict(logml=lm, grad=g, alpha=al), o, (n, dt, "host, shared"))


def test_grid_stride_and_chunking(tmp_path):
    """the calls of _ard_worker.STRIDE_CASES under the default switches, checked against the reference and saved; then one process with
    the grid held to one round of resident workgroups and the workspace cap at 1 MiB must give the same bits"""
    saved = {}
    for i, (n, d, batch, dt, kind, shared, rejects) in enumerate(A.STRIDE_CASES):
        X, y, th, want_info = A.stride_inputs(n, d, batch, dt, kind, shared, rejects)
        out, info = gpu(n, X[0] if shared else X, y[0] if shared else y, th, kind, d=d)
        A.check_with_rejects(out, info, X, y, th, n, d, kind, dt, want_info, f"{name_of(dt, kind, n)} batch={batch}", sample=200)
        saved[A.stride_key(i, "info")] = info
        for k, v in out.items():
            saved[A.stride_key(i, k)] = v
    path = os.path.join(tmp_path, "default_call.npz")
    np.savez(path, **saved)
    e = dict(os.environ)
    e.update({"MATINV_TILE_GRID_MULT": "1", "MATINV_BLOCKED_WS_MB": "1"})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_ard_worker.py"), path], capture_output=True, text=True, env=e,
                       timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "ard-worker ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
