"""GPU tests of the gradients of the multi-output GP log marginal likelihood (matinv_multi_target_grad_batched): all four outputs against
float64 / longdouble numpy (bounds derived in tests/_multi_target_grad_worker.py, not fitted), which outputs are requested (the workspace
against the dAlpha read-back of the target groups), the ties to multi_target_batched (bit for bit) and logml_grad_batched, bit locality,
structured derivatives, the not-positive-definite contract, the host form, and grid rounds and workspace chunks.

Worst err / bound seen on an MI355X (printed by every run; DESIGN.md, "Gradients of the multi-output log marginal likelihood", Accuracy):
tile fp64 grad 0.062, gradc 0.077, logml 0.45, alpha 0.055 (the first three at n = 1); tile fp32 0.096, 0.083, 0.37, 0.31, all at n = 1;
from n = 15 on grad stays below 0.004, gradc below 0.03 and logml and alpha below 0.08; the global forms below 0.015 everywhere."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _multi_target_grad_worker as MG
import _multi_target_worker as MT
from conftest import pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
api = pkg("api")
lib = pkg("_lib")
U = MG.U
DTYPES = (np.float64, np.float32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu(n, B, c, Ys, dMs, want=MG.OUTPUTS, **kw):
    """(dict of numpy outputs, info)"""
    return MG.run(api, torch, n, B, c, Ys, dMs, want=want, **kw)


def name_of(dt, n):
    name = api.multi_target_grad_kernel_name(dt, n)
    assert name.startswith("matinv_spd_tile_f" if n <= 96 else "matinv_chol_global<")
    assert name.endswith(", true, true, true, true, true, true, true, true, true>")
    return name


def inputs(n, dt, with_c, D, P):
    """(B, c, y, dM, reference) of the first D targets and P derivative matrices of the shared case"""
    B, c, Ys, dMs, full = MG.case(n, np.dtype(dt).name, with_c)
    return B, c, MG.first(Ys, n, MG.DMAX, D), (MG.first_derivs(dMs, n, MG.PMAX, P) if P else None), MG.take(full, dMs, n, D, P)


def accuracy(n, dt, with_c, dps):
    for D, P in dps:
        B, c, y, dm, ref = inputs(n, dt, with_c, D, P)
        out, info = gpu(n, B, c, y, dm)
        assert not info.any(), (n, dt, info)
        assert all(v.dtype == np.dtype(dt) for v in out.values())
        MG.check(out, ref, n, U[np.dtype(dt)], what=name_of(dt, n) + (" c" if with_c else ""))


@pytest.mark.parametrize("n", MG.TILE_SIZES + MG.GLOBAL_SIZES)
def test_accuracy(n):
    for dt in DTYPES:
        for with_c in (True, False):
            accuracy(n, dt, with_c, MG.DP)


@pytest.mark.parametrize("dt", DTYPES)
def test_accuracy_1024(dt):
    accuracy(1024, dt, True, (MG.DP_1024,))


@pytest.mark.parametrize("n", [33, 96, 130])
@pytest.mark.parametrize("D", [17, 33])
def test_optional_outputs(n, D):
    P = 2
    for dt in DTYPES:
        B, c, y, dm, _ = inputs(n, dt, True, D, P)
        out, info = gpu(n, B, c, y, dm)
        assert not info.any()
        # each output alone, grad + alpha and grad: the bits of the all-outputs call. Without alpha the groups of targets come back from
        # the library's workspace, with it from dAlpha
        for want in [(k,) for k in MG.OUTPUTS] + [("grad", "alpha"), ("grad", "gradc")]:
            o, i = gpu(n, B, c, y, dm if "grad" in want else None, want=want)
            MG.same_bits(o, {k: out[k] for k in want}, (n, dt, want))
            assert not i.any()
        # gradc alone with P = 0 and dDMs = NULL
        o, _ = gpu(n, B, c, y, None, want=("gradc",), P=0)
        assert np.array_equal(o["gradc"], out["gradc"])
        # the raw C entry point on tensors larger than the call: the tails and the info tail stay as they were
        batch = B.size // (n * n)
        sizes = dict(grad=batch * P, gradc=batch * n, logml=batch * D, alpha=batch * D * n)
        t = lambda x: torch.tensor(np.ascontiguousarray(x)).cuda()  # noqa: E731
        ins = [t(B), t(c), t(y), t(dm)]
        outs = {k: torch.full((sizes[k] + 7,), -7.5, dtype=ins[0].dtype, device="cuda") for k in MG.OUTPUTS}
        info = torch.full((batch + 3,), -7, dtype=torch.int32, device="cuda")
        ptr = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
        torch.cuda.synchronize()
        rc = lib.lib().matinv_multi_target_grad_batched(api.F64 if dt is np.float64 else api.F32, n, D, P, *[ptr(x) for x in ins],
                                                        *[ptr(outs[k]) for k in MG.OUTPUTS], batch, ptr(info), None)
        torch.cuda.synchronize()
        assert rc == lib.OK
        for k in MG.OUTPUTS:
            got = outs[k].cpu().numpy()
            assert np.array_equal(got[:sizes[k]], out[k]) and (got[sizes[k]:] == -7.5).all(), (n, dt, k)
        got = info.cpu().numpy()
        assert not got[:batch].any() and (got[batch:] == -7).all()


@pytest.mark.parametrize("n", [33, 64, 95, 130])
def test_logml_and_alpha_are_the_bits_of_multi_target_batched(n):
    D = 33
    for dt in DTYPES:
        for with_c in (True, False):
            B, c, y, dm, _ = inputs(n, dt, with_c, D, 1)
            out, info = gpu(n, B, c, y, dm)
            parent, pinfo = MT.run(api, torch, n, B, c, y, None, want=("alpha", "logml"))
            assert np.array_equal(info, pinfo)
            MG.same_bits({k: out[k] for k in ("alpha", "logml")}, parent, (n, dt, with_c))


@pytest.mark.parametrize("n", [16, 64, 96, 130])
def test_one_target_agrees_with_logml_grad_batched(n):
    """D = 1 against logml_grad_batched: each side is within one bound of the reference, so they are within two of each other"""
    P = 2
    for dt in DTYPES:
        B, c, y, dm, ref = inputs(n, dt, True, 1, P)
        out, info = gpu(n, B, c, y, dm)
        assert not info.any()
        t = lambda x: torch.tensor(np.ascontiguousarray(x)).cuda()  # noqa: E731
        grad, gradc, alpha = api.logml_grad_batched(n, t(B), t(c), t(y), t(dm), want=("grad", "gradc", "alpha"))
        torch.cuda.synchronize()
        single = dict(grad=grad.cpu().numpy(), gradc=gradc.cpu().numpy(), alpha=alpha.cpu().numpy())
        u = U[np.dtype(dt)]
        MG.check(single, ref, n, u, what=f"logml_grad_batched n={n}")
        b = MG.bounds(ref, n, u)
        shp = MG.shapes(ref, n)
        for k, v in single.items():
            diff = np.abs(out[k].reshape(shp[k]).astype(np.float64) - v.reshape(shp[k]).astype(np.float64))
            assert (diff <= 2 * b[k]).all(), (n, dt, k, float((diff / b[k]).max()))


@pytest.mark.parametrize("n", [33, 95, 130])
@pytest.mark.parametrize("D", [17, 33])
def test_locality(n, D):
    P = 3
    for dt in DTYPES:
        u = U[np.dtype(dt)]
        B, c, y, dm, ref = inputs(n, dt, True, D, P)
        batch = B.size // (n * n)
        out, info = gpu(n, B, c, y, dm)
        assert not info.any()
        # matrix k alone
        k1 = batch - 2
        row = lambda x: x.reshape(batch, -1)[k1]  # noqa: E731
        ok, ik = gpu(n, row(B), row(c), row(y), row(dm))
        MG.same_bits(ok, {k: row(v) for k, v in out.items()}, (n, dt, "matrix alone"))
        assert ik[0] == 0
        # grad[k, p] depends on dM_p alone: p alone, and P = 3 in the other order against its positions
        g3 = out["grad"].reshape(batch, P)
        for p in range(P):
            o1, _ = gpu(n, B, c, y, MG.first_derivs(dm, n, P, [p]), want=("grad",))
            assert np.array_equal(o1["grad"], g3[:, p]), (n, dt, p)
        o3, _ = gpu(n, B, c, y, MG.first_derivs(dm, n, P, [2, 0, 1]), want=("grad",))
        assert np.array_equal(o3["grad"].reshape(batch, P), g3[:, [2, 0, 1]]), (n, dt)
        # an all-zero target appended: alpha = 0 adds nothing to sum alpha alpha^T, but D counts it, so grad and gradc move by the
        # K term of one target: against the reference of the D + 1 targets, within the bounds
        y1 = np.concatenate([y.reshape(batch, D, n), np.zeros((batch, 1, n), dtype=y.dtype)], axis=1).reshape(-1)
        o1, _ = gpu(n, B, c, y1, dm, want=("grad", "gradc"))
        mdl = MT.model(B, c, n)
        MG.check(o1, MG.reference(MT.reference(mdl, y1, None, n, D + 1, 0), dm, n, P), n, u, what=f"{name_of(dt, n)} zero target appended")
        # targets permuted: the same sums in another order, within two bounds
        perm = np.random.default_rng(5).permutation(D)
        op, _ = gpu(n, B, c, MG.first(y, n, D, list(perm)), dm, want=("grad", "gradc"))
        b = MG.bounds(ref, n, u)
        shp = MG.shapes(ref, n)
        for k in ("grad", "gradc"):
            diff = np.abs(op[k].reshape(shp[k]).astype(np.float64) - out[k].reshape(shp[k]).astype(np.float64))
            assert (diff <= 2 * b[k]).all(), (n, dt, k, float((diff / b[k]).max()))


def edge_pairs(n):
    """(i, j), i >= j, on both sides of every 16-wide tile edge, the corners and the last row"""
    pairs = [(0, 0), (n - 1, 0), (n - 1, n - 1)]
    for e in range(16, n, 16):
        pairs += [(e - 1, e - 1), (e, e - 1), (e, e), (e, 0), (n - 1, e), (n - 1, e - 1)]
    return sorted(set(pairs))


@pytest.mark.parametrize("n", [33, 96])
def test_structured_derivatives(n):
    D = 17
    for dt in DTYPES:
        u = U[np.dtype(dt)]
        B, c, y, _, _ = inputs(n, dt, True, D, 0)
        batch = B.size // (n * n)
        mt = MT.reference(MT.model(B, c, n), y, None, n, D, 0)
        pairs = edge_pairs(n)
        mats = [np.eye(n)]
        for i, j in pairs:  # dM = e_i e_j^T + e_j e_i^T
            m = np.zeros((n, n))
            m[i, j] += 1
            m[j, i] += 1
            mats.append(m)
        P = len(mats)
        dm = np.ascontiguousarray(np.broadcast_to(np.stack(mats)[None], (batch, P, n, n))).astype(dt).reshape(-1)
        ref = MG.reference(mt, dm, n, P)
        out, info = gpu(n, B, c, y, dm)
        assert not info.any()
        MG.check(out, ref, n, u, what=f"{name_of(dt, n)} structured dM")
        b = MG.bounds(ref, n, u)
        g = out["grad"].reshape(batch, P).astype(np.float64)
        gc = out["gradc"].reshape(batch, n).astype(np.float64)
        # dM = I: grad = sum_i gradc_i, each side within its bound
        assert (np.abs(g[:, 0] - gc.sum(axis=1)) <= b["grad"][:, 0] + b["gradc"].sum(axis=1)).all(), (n, dt)
        # dM = e_i e_j^T + e_j e_i^T: grad = G_ij
        for p, (i, j) in enumerate(pairs, start=1):
            assert (np.abs(g[:, p] - ref["G"][:, i, j]) <= b["grad"][:, p]).all(), (n, dt, i, j)
        # an upper triangle filled with NaN, in B and in every dM, changes no bit (column-major: element (r, c) at c n + r, so the
        # strictly upper part r < c is the strictly lower part of the flat matrix read row by row)
        upper = np.tril(np.ones((n, n), dtype=bool), -1).reshape(-1)
        poison = lambda flat: np.where(upper[None], np.nan, flat.reshape(-1, n * n)).astype(dt).reshape(-1)  # noqa: E731
        on, i_n = gpu(n, poison(B), c, y, poison(dm))
        MG.same_bits(on, out, (n, dt, "NaN above the diagonal"))
        assert not i_n.any()


@pytest.mark.parametrize("n", [17, 64, 100])
def test_not_positive_definite(n):
    D, P = 17, 2
    for dt in DTYPES:
        for with_c in (True, False):
            B, c, y, dm, _ = inputs(n, dt, with_c, D, P)
            out, _ = gpu(n, B, c, y, dm)
            Bb, cb = np.array(B), (None if c is None else np.array(c))
            want_info = MG.break_three(Bb, cb, n, (1, 3, 4))
            assert want_info == {1: n, 3: 2, 4: 1}
            ob, info = gpu(n, Bb, cb, y, dm)
            MG.check_with_rejects(ob, info, Bb, cb, y, dm, n, D, P, dt, want_info, name_of(dt, n) + " rejects")
            # the neighbours keep their bits
            batch = info.size
            ok = [k for k in range(batch) if k not in want_info]
            for k in MG.OUTPUTS:
                assert np.array_equal(ob[k].reshape(batch, -1)[ok], out[k].reshape(batch, -1)[ok]), (n, dt, k)
            # each output alone is NaN there as well
            for k in MG.OUTPUTS:
                o1, i1 = gpu(n, Bb, cb, y, dm if k == "grad" else None, want=(k,))
                assert np.array_equal(i1, info) and np.array_equal(o1[k], ob[k], equal_nan=True), (n, dt, k)


@pytest.mark.parametrize("n", [40, 100])
def test_host_form_equals_device_form(n):
    for dt in DTYPES:
        B, c, y, dm, _ = inputs(n, dt, True, 17, 2)
        out, _ = gpu(n, B, c, y, dm)
        g, gc, lm, al, info = api.multi_target_grad_batched_host(n, B, c, y, dm)
        assert not info.any()
        MG.same_bits(dict(grad=g, gradc=gc, logml=lm, alpha=al), out, (n, dt, "host"))
        g, gc, lm, al, info = api.multi_target_grad_batched_host(n, B, c, y, None, want=("gradc",))
        assert g is None and lm is None and al is None and not info.any() and np.array_equal(gc, out["gradc"])


def test_grid_stride_and_chunking(tmp_path):
    """the calls of _multi_target_grad_worker.STRIDE_CASES under the default switches, checked against the reference and saved; then one
    process with the grid held to one round of resident workgroups and the workspace cap at 1 MiB must give the same bits"""
    saved = {}
    for i, (n, batch, D, P, dt, with_c, rejects_at) in enumerate(MG.STRIDE_CASES):
        B, c, Ys, dMs, want_info = MG.stride_inputs(n, batch, D, P, dt, with_c, rejects_at)
        out, info = gpu(n, B, c, Ys, dMs)
        MG.check_with_rejects(out, info, B, c, Ys, dMs, n, D, P, dt, want_info, f"{name_of(dt, n)} batch={batch}")
        saved[MG.stride_key(i, "info")] = info
        for k, v in out.items():
            saved[MG.stride_key(i, k)] = v
    path = os.path.join(tmp_path, "default_call.npz")
    np.savez(path, **saved)
    e = dict(os.environ)
    e.update({"MATINV_TILE_GRID_MULT": "1", "MATINV_BLOCKED_WS_MB": "1"})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_multi_target_grad_worker.py"), path], capture_output=True, text=True,
                       env=e, timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "multi-target-grad-worker ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
