"""GPU tests of the gradients of the trend GP's restricted log marginal likelihood (matinv_trend_grad_batched): all five outputs against
float64 / longdouble numpy (bounds derived in tests/_trend_grad_worker.py, not fitted), the bits of trend_batched, which outputs are
requested (the workspace against the dAlpha read-back of the target groups), bit locality, structured derivatives (the identity, single
elements at the tile edges, and h_b h_b^T, along which the gradient vanishes), the not-positive-definite and the rank-deficient contract,
the composed route, the host form, and grid rounds and workspace chunks.

Worst err / bound seen on an MI355X (printed by every run; DESIGN.md, "Gradients of the restricted log marginal likelihood of the
trend model", Error bounds): tile fp64 grad 0.013, gradc 0.014, logml 0.15, alpha 0.13, beta 0.25; tile fp32 0.041, 0.044, 0.11, 0.12,
0.30, all at n = 1; from n = 15 on grad stays below 0.0012, gradc below 0.004, logml below 0.043 and alpha and beta below 0.015; the
global forms below 0.014 everywhere."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import _trend_grad_worker as TG
import _trend_worker as T
from conftest import pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
api = pkg("api")
lib = pkg("_lib")
U = TG.U
DTYPES = (np.float64, np.float32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu(n, B, c, Hs, Ys, dMs, want=TG.OUTPUTS, **kw):
    """(dict of numpy outputs, info)"""
    return TG.run(api, torch, n, B, c, Hs, Ys, dMs, want=want, **kw)


def name_of(dt, n):
    name = api.trend_grad_kernel_name(dt, n)
    assert name.startswith("matinv_spd_tile_f" if n <= 96 else "matinv_chol_global<")
    assert name.endswith(", true" * 11 + ">")
    return name


def inputs(n, dt, with_c, K, D, P):
    """(B, c, Hs, y, dM, reference) of the first D targets and P derivative matrices of the shared case with K basis vectors"""
    B, c, Hs, Ys, dMs, full = TG.case(n, np.dtype(dt).name, with_c, K)
    return B, c, Hs, TG.first(Ys, n, TG.DMAX, D), (TG.first_derivs(dMs, n, TG.PMAX, P) if P else None), TG.take(full, dMs, n, D, P)


def accuracy(n, dt, with_c, shapes):
    for K, D, P in shapes:
        B, c, Hs, y, dm, ref = inputs(n, dt, with_c, K, D, P)
        out, info = gpu(n, B, c, Hs, y, dm, K=K)
        assert not info.any(), (n, dt, info)
        assert all(v.dtype == np.dtype(dt) for v in out.values())
        TG.check(out, ref, n, U[np.dtype(dt)], what=name_of(dt, n) + (" c" if with_c else ""))


@pytest.mark.parametrize("n", TG.TILE_SIZES + TG.GLOBAL_SIZES)
def test_accuracy(n):
    for dt in DTYPES:
        for with_c in (True, False):
            accuracy(n, dt, with_c, TG.shapes_of(n))


@pytest.mark.parametrize("dt", DTYPES)
def test_accuracy_1024(dt):
    accuracy(1024, dt, True, (TG.KDP_1024,))


@pytest.mark.parametrize("n", [1, 33, 64, 95, 130])
def test_bits_of_trend_batched(n):
    D = 33
    for dt in DTYPES:
        for with_c in (True, False):
            K = TG.clip(4, n)
            B, c, Hs, y, dm, _ = inputs(n, dt, with_c, K, D, 1)
            out, info = gpu(n, B, c, Hs, y, dm, K=K)
            parent, pinfo = T.run(api, torch, n, B, c, Hs, y, None, None, None, want=("beta", "alpha", "logml"), K=K)
            assert np.array_equal(info, pinfo)
            TG.same_bits({k: out[k] for k in ("beta", "alpha", "logml")}, parent, (n, dt, with_c))


@pytest.mark.parametrize("n", [33, 96, 130])
@pytest.mark.parametrize("D", [16, 17, 33])
def test_optional_outputs(n, D):
    K, P = 3, 2
    for dt in DTYPES:
        B, c, Hs, y, dm, _ = inputs(n, dt, True, K, D, P)
        out, info = gpu(n, B, c, Hs, y, dm, K=K)
        assert not info.any()
        # every non-empty subset of the outputs: the bits of the all-outputs call. Without alpha the groups of targets come back from
        # the library's workspace, with it from dAlpha
        for r in range(1, len(TG.OUTPUTS)):
            for want in itertools.combinations(TG.OUTPUTS, r):
                o, i = gpu(n, B, c, Hs, y, dm if "grad" in want else None, want=want, K=K)
                TG.same_bits(o, {k: out[k] for k in want}, (n, dt, want))
                assert not i.any()
        # gradc alone with P = 0 and dDMs = NULL
        o, _ = gpu(n, B, c, Hs, y, None, want=("gradc",), K=K, P=0)
        assert np.array_equal(o["gradc"], out["gradc"])
        # the raw C entry point on tensors larger than the call: the tails and the info tail stay as they were
        batch = B.size // (n * n)
        sizes = dict(grad=batch * P, gradc=batch * n, logml=batch * D, alpha=batch * D * n, beta=batch * D * K)
        t = lambda x: torch.tensor(np.ascontiguousarray(x)).cuda()  # noqa: E731
        ins = [t(B), t(c), t(Hs), t(y), t(dm)]
        outs = {k: torch.full((sizes[k] + 7,), -7.5, dtype=ins[0].dtype, device="cuda") for k in TG.OUTPUTS}
        info = torch.full((batch + 3,), -7, dtype=torch.int32, device="cuda")
        ptr = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
        torch.cuda.synchronize()
        rc = lib.lib().matinv_trend_grad_batched(api.F64 if dt is np.float64 else api.F32, n, K, D, P, *[ptr(x) for x in ins],
                                                 *[ptr(outs[k]) for k in TG.OUTPUTS], batch, ptr(info), None)
        torch.cuda.synchronize()
        assert rc == lib.OK
        for k in TG.OUTPUTS:
            got = outs[k].cpu().numpy()
            assert np.array_equal(got[:sizes[k]], out[k]) and (got[sizes[k]:] == -7.5).all(), (n, dt, k)
        got = info.cpu().numpy()
        assert not got[:batch].any() and (got[batch:] == -7).all()


@pytest.mark.parametrize("n", [33, 95, 130])
@pytest.mark.parametrize("D", [17, 33])
def test_locality(n, D):
    K, P = 4, 3
    for dt in DTYPES:
        B, c, Hs, y, dm, _ = inputs(n, dt, True, K, D, P)
        batch = B.size // (n * n)
        out, info = gpu(n, B, c, Hs, y, dm, K=K)
        assert not info.any()
        # matrix k alone, and the batch in two calls
        k1 = batch - 2
        row = lambda x: x.reshape(batch, -1)[k1]  # noqa: E731
        ok, ik = gpu(n, row(B), row(c), row(Hs), row(y), row(dm), K=K)
        TG.same_bits(ok, {k: row(v) for k, v in out.items()}, (n, dt, "matrix alone"))
        assert ik[0] == 0
        part = lambda x, lo, hi: x.reshape(batch, -1)[lo:hi].reshape(-1)  # noqa: E731
        for lo, hi in ((0, 3), (3, batch)):
            o, _ = gpu(n, *(part(x, lo, hi) for x in (B, c, Hs, y, dm)), K=K)
            TG.same_bits(o, {k: part(v, lo, hi) for k, v in out.items()}, (n, dt, lo))
        # the neighbours replaced: matrix k1 keeps its bits
        other = [np.array(x).reshape(batch, -1) for x in (B, c, Hs, y, dm)]
        for x in other[2:]:  # the neighbours' basis, targets and dM halved: still valid problems, other bits everywhere
            keep = x[k1].copy()
            x *= 0.5
            x[k1] = keep
        on, _ = gpu(n, *(x.reshape(-1) for x in other), K=K)
        for k in TG.OUTPUTS:
            assert np.array_equal(on[k].reshape(batch, -1)[k1], out[k].reshape(batch, -1)[k1]), (n, dt, k)
        # grad[k, p] depends on dM_p alone: p alone, and P = 3 in another order against its positions
        g3 = out["grad"].reshape(batch, P)
        for p in range(P):
            o1, _ = gpu(n, B, c, Hs, y, TG.first_derivs(dm, n, P, [p]), want=("grad",), K=K)
            assert np.array_equal(o1["grad"], g3[:, p]), (n, dt, p)
        o3, _ = gpu(n, B, c, Hs, y, TG.first_derivs(dm, n, P, [2, 0, 1]), want=("grad",), K=K)
        assert np.array_equal(o3["grad"].reshape(batch, P), g3[:, [2, 0, 1]]), (n, dt)


def edge_pairs(n):
    """(i, j), i >= j, on both sides of every 16-wide tile edge, the corners and the last row"""
    pairs = [(0, 0), (n - 1, 0), (n - 1, n - 1)]
    for e in range(16, n, 16):
        pairs += [(e - 1, e - 1), (e, e - 1), (e, e), (e, 0), (n - 1, e), (n - 1, e - 1)]
    return sorted(set(pairs))


@pytest.mark.parametrize("n", [17, 33, 64, 96, 130])
def test_structured_derivatives(n):
    K, D = 3, 17
    for dt in DTYPES:
        u = U[np.dtype(dt)]
        B, c, Hs, y, _, _ = inputs(n, dt, True, K, D, 0)
        batch = B.size // (n * n)
        tr = T.take(TG.case(n, np.dtype(dt).name, True, K)[5], D, 0)
        pairs = edge_pairs(n)
        mats = [np.eye(n)]
        for i, j in pairs:  # dM = e_i e_j^T + e_j e_i^T
            m = np.zeros((n, n))
            m[i, j] += 1
            m[j, i] += 1
            mats.append(m)
        fixed = np.broadcast_to(np.stack(mats)[None], (batch, len(mats), n, n))
        h = np.asarray(Hs, dtype=np.float64).reshape(batch, K, n)
        hh = np.einsum("kbi,kbj->kbij", h, h)  # dM = h_b h_b^T: G H = 0, so grad vanishes
        P = len(mats) + K
        dm = np.ascontiguousarray(np.concatenate([fixed, hh], axis=1)).astype(dt).reshape(-1)
        ref = TG.reference(tr, dm, n, P)
        out, info = gpu(n, B, c, Hs, y, dm, K=K)
        assert not info.any()
        TG.check(out, ref, n, u, what=f"{name_of(dt, n)} structured dM")
        b = TG.bounds(ref, n, u)
        g = out["grad"].reshape(batch, P).astype(np.float64)
        gc = out["gradc"].reshape(batch, n).astype(np.float64)
        # dM = I: grad = sum_i gradc_i, each side within its bound
        assert (np.abs(g[:, 0] - gc.sum(axis=1)) <= b["grad"][:, 0] + b["gradc"].sum(axis=1)).all(), (n, dt)
        # dM = e_i e_j^T + e_j e_i^T: grad = G_ij
        for p, (i, j) in enumerate(pairs, start=1):
            assert (np.abs(g[:, p] - ref["G"][:, i, j]) <= b["grad"][:, p]).all(), (n, dt, i, j)
        # dM = h_b h_b^T (as rounded to dt): |grad| within the bound of a gradient that is zero but for that rounding
        tail = slice(len(mats), P)
        print(f"  {name_of(dt, n)} h h^T: worst |grad| / bound {float((np.abs(g[:, tail]) / b['grad'][:, tail]).max()):.4f}")
        assert (np.abs(g[:, tail]) <= b["grad"][:, tail] + np.abs(ref["grad"][:, tail])).all(), (n, dt)
        assert (np.abs(ref["grad"][:, tail]) <= b["grad"][:, tail]).all(), (n, dt)
        # an upper triangle filled with NaN, in B and in every dM, changes no bit (column-major: element (r, c) at c n + r, so the
        # strictly upper part r < c is the strictly lower part of the flat matrix read row by row)
        upper = np.tril(np.ones((n, n), dtype=bool), -1).reshape(-1)
        poison = lambda flat: np.where(upper[None], np.nan, flat.reshape(-1, n * n)).astype(dt).reshape(-1)  # noqa: E731
        on, i_n = gpu(n, poison(B), c, Hs, y, poison(dm), K=K)
        TG.same_bits(on, out, (n, dt, "NaN above the diagonal"))
        assert not i_n.any()


@pytest.mark.parametrize("n", [16, 64, 96, 130])
def test_not_positive_definite(n):
    """_loo_worker.break_three on M gives info n, 2, 1. Matrix 2 has h_2 = h_1 bit for bit (K = 3): A_11, A_21 and A_22 are equal bit for
    bit and the factorisation of A updates with the IEEE quotient A_21 / A_11 = 1, so pivot 2 is exactly 0 in either precision and info is
    n + 2 exactly (tests/test_gpu_trend.py)"""
    K, D, P = 3, 17, 2
    for dt in DTYPES:
        for with_c in (True, False):
            B, c, Hs, y, dm, _ = inputs(n, dt, with_c, K, D, P)
            out, _ = gpu(n, B, c, Hs, y, dm, K=K)
            Bb, cb, Hb = np.array(B), (None if c is None else np.array(c)), np.array(Hs)
            want_info = TG.break_three(Bb, cb, n, (1, 3, 4))
            assert want_info == {1: n, 3: 2, 4: 1}
            batch = B.size // (n * n)
            Hb.reshape(batch, K, n)[2, 1] = Hb.reshape(batch, K, n)[2, 0]
            want_info[2] = n + 2
            ob, info = gpu(n, Bb, cb, Hb, y, dm, K=K)
            TG.check_with_rejects(ob, info, Bb, cb, Hb, y, dm, n, K, D, P, dt, want_info, name_of(dt, n) + " rejects")
            # the neighbours keep their bits
            ok = [k for k in range(batch) if k not in want_info]
            for k in TG.OUTPUTS:
                assert np.array_equal(ob[k].reshape(batch, -1)[ok], out[k].reshape(batch, -1)[ok]), (n, dt, k)
            # each output alone reports the same info and is NaN there as well
            for k in TG.OUTPUTS:
                o1, i1 = gpu(n, Bb, cb, Hb, y, dm if k == "grad" else None, want=(k,), K=K)
                assert np.array_equal(i1, info) and np.array_equal(o1[k], ob[k], equal_nan=True), (n, dt, k)


def composed(n, dt, B, c, Hs, y, dm, K, D, P):
    """the route a user had before: inverse_batched for Kinv, then P = Kinv - Kinv H A^-1 H^T Kinv, alpha = P y, G and the contractions in
    torch, in the working precision"""
    batch = B.size // (n * n)
    t = lambda x: torch.tensor(np.ascontiguousarray(x)).cuda()  # noqa: E731
    M = torch.tensor(T.G.image(B, c, n).astype(dt)).cuda()  # what the kernel reads: the lower triangle mirrored, B_ii + c_i rounded in dt
    info = torch.empty(batch, dtype=torch.int32, device="cuda")
    Kinv = api.inverse_batched(M.reshape(-1), n, api.ALGO_CHOLESKY, info=info).reshape(batch, n, n)
    Kinv = (Kinv + Kinv.transpose(1, 2)) / 2
    H = t(Hs).reshape(batch, K, n).transpose(1, 2)
    Y = t(y).reshape(batch, D, n)
    KH = Kinv @ H
    Pm = Kinv - KH @ torch.linalg.solve(H.transpose(1, 2) @ KH, KH.transpose(1, 2))
    alpha = torch.einsum("kij,ktj->kti", Pm, Y)
    Gm = torch.einsum("kti,ktj->kij", alpha, alpha) - D * Pm
    dM = torch.tensor(TG.sym_lower(dm, n).reshape(batch, P, n, n).astype(dt)).cuda()
    grad = 0.5 * torch.einsum("kij,kpij->kp", Gm, dM)
    gradc = 0.5 * torch.diagonal(Gm, dim1=1, dim2=2)
    torch.cuda.synchronize()
    assert not info.cpu().numpy().any()
    return dict(grad=grad.cpu().numpy(), gradc=gradc.cpu().numpy(), alpha=alpha.cpu().numpy())


@pytest.mark.parametrize("n", [16, 64, 96, 130])
def test_agreement_with_the_composed_route(n):
    """inverse_batched + torch algebra in the working precision: within two bounds of the fused call"""
    K, D, P = 3, 17, 2
    for dt in DTYPES:
        B, c, Hs, y, dm, ref = inputs(n, dt, True, K, D, P)
        out, info = gpu(n, B, c, Hs, y, dm, K=K)
        assert not info.any()
        other = composed(n, dt, B, c, Hs, y, dm, K, D, P)
        b = TG.bounds(ref, n, U[np.dtype(dt)])
        shp = TG.shapes(ref, n)
        for k, v in other.items():
            diff = np.abs(out[k].reshape(shp[k]).astype(np.float64) - v.reshape(shp[k]).astype(np.float64))
            print(f"  composed route n={n} {np.dtype(dt).name} {k}: worst diff / bound {float((diff / b[k]).max()):.4f}")
            assert (diff <= 2 * b[k]).all(), (n, dt, k, float((diff / b[k]).max()))


@pytest.mark.parametrize("n", [40, 100])
def test_host_form_equals_device_form(n):
    K, D, P = 3, 17, 2
    for dt in DTYPES:
        B, c, Hs, y, dm, _ = inputs(n, dt, True, K, D, P)
        out, _ = gpu(n, B, c, Hs, y, dm, K=K)
        res = api.trend_grad_batched_host(n, B, c, Hs, y, dm, nbasis=K)
        assert not res[5].any()
        TG.same_bits(dict(zip(TG.OUTPUTS, res[:5])), out, (n, dt, "host"))
        res = api.trend_grad_batched_host(n, B, c, Hs, y, None, want=("gradc",), nbasis=K)
        assert all(res[i] is None for i in (0, 2, 3, 4)) and not res[5].any() and np.array_equal(res[1], out["gradc"])
        # info may be NULL
        batch = B.size // (n * n)
        g = np.empty(batch * P, dtype=dt)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        rc = lib.lib().matinv_trend_grad_batched_host(api.F64 if dt is np.float64 else api.F32, n, K, D, P, p(B), p(c), p(Hs), p(y), p(dm), p(g),
                                                      None, None, None, None, batch, None)
        assert rc == lib.OK and np.array_equal(g, out["grad"])


def test_grid_stride_and_chunking(tmp_path):
    """the calls of _trend_grad_worker.STRIDE_CASES under the default switches, checked against the reference and saved; then one process
    with the grid held to one round of resident workgroups and the workspace cap at 1 MiB must give the same bits"""
    saved = {}
    for i, (n, batch, K, D, P, dt, with_c, rejects_at, singular_at) in enumerate(TG.STRIDE_CASES):
        B, c, Hs, Ys, dMs, want_info = TG.stride_inputs(n, batch, K, D, P, dt, with_c, rejects_at, singular_at)
        out, info = gpu(n, B, c, Hs, Ys, dMs, K=K)
        TG.check_with_rejects(out, info, B, c, Hs, Ys, dMs, n, K, D, P, dt, want_info, f"{name_of(dt, n)} batch={batch}")
        saved[TG.stride_key(i, "info")] = info
        for k, v in out.items():
            saved[TG.stride_key(i, k)] = v
    path = os.path.join(tmp_path, "default_call.npz")
    np.savez(path, **saved)
    e = dict(os.environ)
    e.update({"MATINV_TILE_GRID_MULT": "1", "MATINV_BLOCKED_WS_MB": "1"})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_trend_grad_worker.py"), path], capture_output=True, text=True, env=e,
                       timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "trend-grad-worker ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
