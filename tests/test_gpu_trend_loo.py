"""GPU tests of the leave-one-out cross-validation of the trend GP (matinv_trend_loo_batched): the three outputs against float64 numpy
(bounds derived in tests/_trend_loo_worker.py, not fitted), the held-out fits through trend_batched, which outputs are requested, bit
locality in the targets and in the batch, the host form, the not-positive-definite, the rank-deficient and the degenerate hold-out
contract, grid rounds and workspace chunks, and the argument refusals.

Worst err / bound seen on an MI355X (printed by every run; DESIGN.md, "Leave-one-out cross-validation of the trend model", Error bounds):
tile fp64 mean 0.029, var 0.051, logpl 0.061; tile fp32 0.052, 0.040, 0.051, the mean and logpl figures at n = 2 (from n = 15 on mean
stays below 0.01 and logpl below 0.031); the global forms below 0.033 everywhere.

The point index in the code n + K + i counts from 1, as the pivot codes do, so that it never equals n + K (pivot K of A): the unit vector
e_5 of the near-degenerate case, an index from 0, reports n + K + 6. Where the issue's near-degenerate case asks var_5 >= 1 / b, this
test asks var_5 >= 1 / (P_55 + b): the computed P_55 is at most the true one plus its bound b, which is 1 / b only where P_55 drowns in b
(in fp64 b is 1e-13 against P_55 = 9e-7); where b < P_55 it asks in addition that var_5 lies within the worker's bound."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import _trend_loo_worker as TL
import _trend_worker as T
from conftest import pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
api = pkg("api")
lib = pkg("_lib")
U = TL.U
DTYPES = (np.float64, np.float32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu(n, B, c, Hs, Ys, want=TL.OUTPUTS, **kw):
    """(dict of numpy outputs, info)"""
    return TL.run(api, torch, n, B, c, Hs, Ys, want=want, **kw)


def name_of(dt, n):
    name = api.trend_loo_kernel_name(dt, n)
    assert name.startswith("matinv_spd_tile_f" if n <= 96 else "matinv_chol_global<")
    assert name.endswith(", true" * 12 + ">")
    return name


def inputs(n, dt, with_c, K, D):
    """(B, c, Hs, y, reference) of the first D targets of the shared case with K basis vectors; D = 0: no targets"""
    B, c, Hs, Ys, full = TL.case(n, np.dtype(dt).name, with_c, K)
    return B, c, Hs, (T.first(Ys, n, TL.DMAX, D) if D else None), TL.take(full, D)


def accuracy(n, dt, with_c, shapes):
    for K, D in shapes:
        B, c, Hs, y, ref = inputs(n, dt, with_c, K, D)
        out, info = gpu(n, B, c, Hs, y, K=K, D=D)
        assert not info.any(), (n, dt, info)
        assert all(v.dtype == np.dtype(dt) for v in out.values())
        TL.check(out, ref, n, U[np.dtype(dt)], what=name_of(dt, n) + (" c" if with_c else ""))


@pytest.mark.parametrize("n", TL.TILE_SIZES + TL.GLOBAL_SIZES)
def test_accuracy(n):
    for dt in DTYPES:
        for with_c in (True, False):
            accuracy(n, dt, with_c, TL.shapes_of(n))


@pytest.mark.parametrize("dt", DTYPES)
def test_accuracy_1024(dt):
    n, (K, D) = 1024, TL.KD_1024
    B, c, _ = TL.L.inputs(n, 2, dt, True)
    Hs, Ys, _, _, _ = T.vectors(n, 2, K, D, 1, dt, 9024)
    out, info = gpu(n, B, c, Hs, Ys, K=K, D=D)
    assert not info.any()
    TL.check(out, TL.reference_of(B, c, Hs, Ys, n, K, D), n, U[np.dtype(dt)], what=name_of(dt, n))


@pytest.mark.parametrize("n", [17, 65])
def test_held_out_fits_through_trend_batched(n):
    """removing a point crosses a tile edge (17 -> 16, 65 -> 64): the n held-out systems of one matrix as ONE trend_batched batch of
    size n - 1 with one query each; mean and var agree within the sum of the two bounds"""
    K, D = 3, 2
    for dt in DTYPES:
        u = U[np.dtype(dt)]
        B, c, Hs, y, ref = inputs(n, dt, True, K, D)
        batch = B.size // (n * n)
        out, info = gpu(n, B, c, Hs, y, K=K, D=D)
        assert not info.any()
        k = 1
        Bm = np.asarray(B).reshape(batch, n, n)[k]  # column-major, lower triangle significant
        Bl = np.tril(Bm.T)
        Bs = Bl + np.tril(Bl, -1).T
        ck, H, Y = np.asarray(c).reshape(batch, n)[k], np.asarray(Hs).reshape(batch, K, n)[k], y.reshape(batch, D, n)[k]
        subB, subc, subH, subY, As, Gs, Es = [], [], [], [], [], [], []
        for i in range(n):
            keep = np.array([j for j in range(n) if j != i])
            subB.append(Bs[np.ix_(keep, keep)].T.reshape(-1))
            subc.append(ck[keep])
            subH.append(H[:, keep].reshape(-1))
            subY.append(Y[:, keep].reshape(-1))
            As.append(Bs[keep, i])
            Gs.append(H[:, i])
            Es.append(Bs[i, i] + ck[i])  # the held-out observation's own variance, noise included
        cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x).reshape(-1) for x in xs]).astype(dt))  # noqa: E731
        sB, sc, sH, sY, sA, sG, sE = (cat(x) for x in (subB, subc, subH, subY, As, Gs, Es))
        held, hinfo = T.run(api, torch, n - 1, sB, sc, sH, sY, sA, sG, sE, want=("mean", "var"), K=K, D=D, Q=1)
        assert not hinfo.any()
        hb = T.bounds(T.reference(T.basis_model(T.model(sB, sc, n - 1), sH, n - 1, K), sY, sA, sG, sE, n - 1, K, D, 1), n - 1, u)
        b = TL.bounds(ref, n, u)
        dm = np.abs(held["mean"].reshape(n, D).T.astype(np.float64) - out["mean"].reshape(batch, D, n)[k])
        dv = np.abs(held["var"].reshape(n).astype(np.float64) - out["var"].reshape(batch, n)[k])
        rm = dm / (hb["mean"][:, :, 0].T + b["mean"][k])
        rv = dv / (hb["var"][:, 0] + b["var"][k])
        print(f"  held-out fits n={n} {np.dtype(dt).name}: worst diff / (sum of bounds) mean {rm.max():.4f} var {rv.max():.4f}")
        assert (rm <= 1).all() and (rv <= 1).all()


@pytest.mark.parametrize("n", [33, 96, 130])
def test_optional_outputs_and_target_locality(n):
    K, D = 4, 33
    for dt in DTYPES:
        B, c, Hs, y, _ = inputs(n, dt, True, K, D)
        batch = B.size // (n * n)
        out, info = gpu(n, B, c, Hs, y, K=K, D=D)
        assert not info.any()
        # every non-empty subset of the outputs: the bits of the all-outputs call
        for r in (1, 2):
            for want in itertools.combinations(TL.OUTPUTS, r):
                o, i = gpu(n, B, c, Hs, y if want != ("var",) else None, want=want, K=K, D=D if want != ("var",) else 0)
                TL.same_bits(o, {k: out[k] for k in want}, (n, dt, want))
                assert not i.any()
        # var is the same for D = 0, 1 and 33
        for Dv in (1,):
            o, _ = gpu(n, B, c, Hs, T.first(y, n, D, Dv), K=K, D=Dv)
            assert np.array_equal(o["var"], out["var"]), (n, dt, Dv)
        # target t alone: the bits it has among 33 (first, the last of a group, the first of the next, the ragged last)
        for t in (0, 15, 16, 32):
            o, _ = gpu(n, B, c, Hs, T.first(y, n, D, [t]), K=K, D=1)
            assert np.array_equal(o["mean"].reshape(batch, n), out["mean"].reshape(batch, D, n)[:, t]), (n, dt, t)
            assert np.array_equal(o["logpl"], out["logpl"].reshape(batch, D)[:, t]), (n, dt, t)
        # matrix k alone, and the batch in two calls
        k1 = batch - 2
        row = lambda x: x.reshape(batch, -1)[k1]  # noqa: E731
        ok, ik = gpu(n, row(B), row(c), row(Hs), row(y), K=K, D=D)
        TL.same_bits(ok, {k: row(v) for k, v in out.items()}, (n, dt, "matrix alone"))
        assert ik[0] == 0
        part = lambda x, lo, hi: x.reshape(batch, -1)[lo:hi].reshape(-1)  # noqa: E731
        for lo, hi in ((0, 3), (3, batch)):
            o, _ = gpu(n, *(part(x, lo, hi) for x in (B, c, Hs, y)), K=K, D=D)
            TL.same_bits(o, {k: part(v, lo, hi) for k, v in out.items()}, (n, dt, lo))
        # the raw C entry point on tensors larger than the call: the tails and the info tail stay as they were
        sizes = dict(mean=batch * D * n, var=batch * n, logpl=batch * D)
        t_ = lambda x: torch.tensor(np.ascontiguousarray(x)).cuda()  # noqa: E731
        ins = [t_(B), t_(c), t_(Hs), t_(y)]
        outs = {k: torch.full((sizes[k] + 7,), -7.5, dtype=ins[0].dtype, device="cuda") for k in TL.OUTPUTS}
        dinfo = torch.full((batch + 3,), -7, dtype=torch.int32, device="cuda")
        ptr = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
        torch.cuda.synchronize()
        rc = lib.lib().matinv_trend_loo_batched(api.F64 if dt is np.float64 else api.F32, n, K, D, *[ptr(x) for x in ins],
                                                *[ptr(outs[k]) for k in TL.OUTPUTS], batch, ptr(dinfo), None)
        torch.cuda.synchronize()
        assert rc == lib.OK
        for k in TL.OUTPUTS:
            got = outs[k].cpu().numpy()
            assert np.array_equal(got[:sizes[k]], out[k]) and (got[sizes[k]:] == -7.5).all(), (n, dt, k)
        got = dinfo.cpu().numpy()
        assert not got[:batch].any() and (got[batch:] == -7).all()


@pytest.mark.parametrize("n", [40, 100])
def test_host_form_equals_device_form(n):
    K, D = 3, 17
    for dt in DTYPES:
        B, c, Hs, y, _ = inputs(n, dt, True, K, D)
        out, _ = gpu(n, B, c, Hs, y, K=K, D=D)
        res = api.trend_loo_batched_host(n, B, c, Hs, y, nbasis=K)
        assert not res[3].any()
        TL.same_bits(dict(zip(TL.OUTPUTS, res[:3])), out, (n, dt, "host"))
        res = api.trend_loo_batched_host(n, B, c, Hs, None, nbasis=K)  # var alone, no targets
        assert res[0] is None and res[2] is None and not res[3].any() and np.array_equal(res[1], out["var"])


@pytest.mark.parametrize("n", [16, 64, 96, 130])
def test_not_positive_definite_and_rank_deficient(n):
    """_loo_worker.break_three on M gives info n, 2, 1; matrix 2 has h_2 = h_1 bit for bit (K = 3), so pivot 2 of A is exactly 0 and info is
    n + 2 (tests/test_gpu_trend.py). Both are the codes of trend_batched on the same inputs."""
    K, D = 3, 17
    for dt in DTYPES:
        for with_c in (True, False):
            B, c, Hs, y, _ = inputs(n, dt, with_c, K, D)
            out, _ = gpu(n, B, c, Hs, y, K=K, D=D)
            Bb, cb, Hb = np.array(B), (None if c is None else np.array(c)), np.array(Hs)
            want_info = dict(TL.break_three(Bb, cb, n, (1, 3, 4)))
            assert want_info == {1: n, 3: 2, 4: 1}
            batch = B.size // (n * n)
            Hb.reshape(batch, K, n)[2, 1] = Hb.reshape(batch, K, n)[2, 0]
            want_info[2] = n + 2
            ob, info = gpu(n, Bb, cb, Hb, y, K=K, D=D)
            TL.check_with_rejects(ob, info, Bb, cb, Hb, y, n, K, D, dt, want_info, name_of(dt, n) + " rejects")
            _, tinfo = T.run(api, torch, n, Bb, cb, Hb, y, None, None, None, want=("logml",), K=K, D=D)
            assert np.array_equal(info, tinfo), (n, dt, info, tinfo)
            ok = [k for k in range(batch) if k not in want_info]
            for k in TL.OUTPUTS:  # the neighbours keep their bits
                assert np.array_equal(ob[k].reshape(batch, -1)[ok], out[k].reshape(batch, -1)[ok]), (n, dt, k)
            o1, i1 = gpu(n, Bb, cb, Hb, None, want=("var",), K=K, D=0)
            assert np.array_equal(i1, info) and np.array_equal(o1["var"], ob["var"], equal_nan=True), (n, dt)


@pytest.mark.parametrize("n", [2, 17, 64, 96, 97])
def test_exact_degenerate_hold_out(n):
    """B = I, c = NULL, H = unit vectors: every operation is exact, P_jj = 1 - 1 = 0 at the points of the basis, and info is exactly
    n + K + i for the FIRST such point i (1-based); every output NaN"""
    D = 2
    for dt in DTYPES:
        sets = TL.degenerate_columns(n)
        for K in (1, 2):
            cols = [s for s in sets if len(s) == K]
            if not cols:
                continue
            pairs = [TL.unit_basis(n, s, dt) for s in cols]
            B = np.concatenate([p[0] for p in pairs])
            Hs = np.concatenate([p[1] for p in pairs])
            y = np.random.default_rng(n).standard_normal(len(cols) * D * n).astype(dt)
            out, info = gpu(n, B, None, Hs, y, K=K, D=D)
            assert np.array_equal(info, [n + K + min(s) + 1 for s in cols]), (n, dt, K, cols, info)
            assert all(np.isnan(v).all() for v in out.values()), (n, dt, K)
            o, i = gpu(n, B, None, Hs, None, want=("var",), K=K, D=0)
            assert np.array_equal(i, info) and np.isnan(o["var"]).all()


@pytest.mark.parametrize("n", [17, 64, 97])
def test_near_degenerate_hold_out(n):
    """H[:, 1] = e_5 + 1e-3 N(0, 1) in one matrix: either info = n + K + 6 (point 5, 1-based) with NaN outputs, or info = 0 and
    var_5 >= 1 / b, b the bound on the error of P_55; the other matrices stay within their bounds"""
    K, D = 3, 2
    for dt in DTYPES:
        u = U[np.dtype(dt)]
        B, c, Hs, y, _ = inputs(n, dt, True, K, D)
        batch = B.size // (n * n)
        Hn = np.array(Hs)
        k = 2
        e5 = np.zeros(n)
        e5[5] = 1
        Hn.reshape(batch, K, n)[k, 1] = (e5 + 1e-3 * np.random.default_rng(50 + n).standard_normal(n)).astype(dt)
        out, info = gpu(n, B, c, Hn, y, K=K, D=D)
        ok = np.array([j for j in range(batch) if j != k])
        assert not info[ok].any()
        TL.check({k_: v for k_, v in out.items()}, TL.reference_of(B, c, Hn, y, n, K, D, idx=ok), n, u, idx=ok, what=name_of(dt, n) + " near")
        # the bound of P_55 of the near-degenerate matrix, without the conditions on the inputs (it breaks them on purpose)
        mdl = T.model(B, c, n, idx=np.array([k]))
        H = Hn.astype(np.float64).reshape(batch, K, n)[k].T[None]
        KH = mdl["Kinv"] @ H
        A = H.transpose(0, 2, 1) @ KH
        sa = np.linalg.svd(A, compute_uv=False)
        bm = dict(mdl, K=K, H=H, KH=KH, Ainv=np.linalg.inv(A), condA=sa[:, 0] / sa[:, -1], hnorm=np.linalg.norm(H, 2, axis=(1, 2)),
                  khnorm=np.linalg.norm(KH, 2, axis=(1, 2)))
        bm.update(TL.loo_terms(bm))
        b = TL.p_bound(bm, n, u)[0, 5]
        v5 = out["var"].reshape(batch, n)[k, 5]
        print(f"  near-degenerate n={n} {np.dtype(dt).name}: info {info[k]} P_55 {bm['pd'][0, 5]:.3e} bound {b:.3e} var_5 {v5:.3e}")
        if info[k]:
            assert info[k] == n + K + 6 and all(np.isnan(v.reshape(batch, -1)[k]).all() for v in out.values())
        else:
            # the computed P_55 is at most P_55 + b: var_5 >= 1 / (P_55 + b), which is 1 / b where P_55 drowns in its bound; where it does
            # not (b < P_55), var_5 is also within the bound of the worker
            p5 = bm["pd"][0, 5]
            assert np.isfinite(v5) and v5 >= 1 / (p5 + b) and all(np.isfinite(v.reshape(batch, -1)[k]).all() for v in out.values())
            if b < p5:
                assert abs(v5 - 1 / p5) <= b / (p5 * (p5 - b)) + 2 * u / p5, (n, dt, v5, p5, b)


def test_grid_stride_and_chunking(tmp_path):
    """the calls of _trend_loo_worker.STRIDE_CASES under the default switches, saved; then one process with the grid held to one round of
    resident workgroups and the workspace cap at 1 MiB must give the same bits"""
    saved = {}
    for i, (n, batch, K, D, dt, with_c, rejects_at, singular_at) in enumerate(TL.STRIDE_CASES):
        B, c, Hs, Ys, want_info = TL.stride_inputs(n, batch, K, D, dt, with_c, rejects_at, singular_at)
        out, info = gpu(n, B, c, Hs, Ys, K=K, D=D)
        expect = np.zeros(batch, dtype=np.int64)
        for k, v in want_info.items():
            expect[k] = v
        assert np.array_equal(info, expect), (n, dt, np.flatnonzero(info != expect)[:10], info[info != expect][:10])
        bad = sorted(want_info)
        for k, v in out.items():
            o = v.reshape(batch, -1)
            assert np.isnan(o[bad]).all() and np.isfinite(np.delete(o, bad, axis=0)).all(), (n, dt, k)
        saved[TL.stride_key(i, "info")] = info
        for k, v in out.items():
            saved[TL.stride_key(i, k)] = v
    path = os.path.join(tmp_path, "default_call.npz")
    np.savez(path, **saved)
    e = dict(os.environ)
    e.update({"MATINV_TILE_GRID_MULT": "1", "MATINV_BLOCKED_WS_MB": "1"})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_trend_loo_worker.py"), path], capture_output=True, text=True, env=e,
                       timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "trend-loo-worker ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])


def test_argument_refusals_launch_nothing():
    """n <= nbasis, nbasis outside 1 .. 16, every output NULL, mean or logpl without targets: refused, and the outputs keep their fill"""
    n, K, D, batch = 8, 2, 2, 2
    B = torch.eye(n, dtype=torch.float64, device="cuda").reshape(-1).repeat(batch)
    H = torch.ones(batch * 16 * n, dtype=torch.float64, device="cuda")
    Y = torch.ones(batch * D * n, dtype=torch.float64, device="cuda")
    outs = [torch.full((batch * D * n,), -7.5, dtype=torch.float64, device="cuda") for _ in range(3)]
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    ptr = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())  # noqa: E731
    L = lib.lib()

    def call(n_=n, K_=K, D_=D, y=Y, o=outs):
        return L.matinv_trend_loo_batched(api.F64, n_, K_, D_, ptr(B), None, ptr(H), ptr(y), *[ptr(x) for x in o], batch, ptr(info), None)

    for rc in (call(K_=8), call(K_=9), call(n_=1, K_=1), call(K_=0), call(K_=17), call(o=[None, None, None]), call(D_=0), call(y=None),
               call(D_=0, o=[outs[0], None, None]), call(y=None, o=[None, None, outs[2]])):
        assert rc == lib.ERR_ARG, (rc, L.matinv_last_error())
    torch.cuda.synchronize()
    assert all((x == -7.5).all().item() for x in outs) and (info == -7).all().item()
    assert call() == lib.OK
