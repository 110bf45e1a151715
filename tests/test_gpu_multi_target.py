"""GPU tests of the multi-output GP solves (matinv_multi_target_batched): all five outputs against float64 / longdouble numpy (bounds
derived in tests/_multi_target_worker.py, not fitted), which outputs are requested, bit locality (target and query position, D, Q, batch,
grid rounds, workspace chunks), the not-positive-definite contract, the agreement with the single-target entry points and the host form.

Worst err / bound seen on an MI355X (printed by every run; DESIGN.md, "Multi-output solves", Accuracy): tile fp64 alpha 0.055, quad 0.031,
logdet 0.33, logml 0.45, mean 0.041 (logdet and logml at n = 1); tile fp32 0.31, 0.25, 0.24, 0.37, 0.40, all at n = 1; from n = 15 on
every output of the tile forms stays below 0.08 and of the global forms below 0.015."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _multi_target_worker as MT
from conftest import pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
api = pkg("api")
lib = pkg("_lib")
U = MT.U
DTYPES = (np.float64, np.float32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_TARGET = ("alpha", "quad", "logml", "mean")


def gpu(n, B, c, Ys, As, want=MT.OUTPUTS, **kw):
    """(dict of numpy outputs, info)"""
    return MT.run(api, torch, n, B, c, Ys, As, want=want, **kw)


def name_of(dt, n):
    name = api.multi_target_kernel_name(dt, n)
    assert name.startswith("matinv_spd_tile_f" if n <= 96 else "matinv_chol_global<")
    assert name.endswith(", true, true, true, true, true, true, true, true>")
    return name


def accuracy(n, dt, with_c, dqs):
    B, c, Ys, As, full = MT.case(n, np.dtype(dt).name, with_c)
    first = None
    for D, Q in dqs:
        y, a = MT.first(Ys, n, MT.DMAX, D), (MT.first(As, n, MT.QMAX, Q) if Q else None)
        want = MT.OUTPUTS if Q else MT.OUTPUTS[:-1]
        out, info = gpu(n, B, c, y, a, want=want)
        assert not info.any(), (n, dt, info)
        assert all(v.dtype == np.dtype(dt) for v in out.values())
        MT.check(out, MT.take(full, D, Q), n, U[np.dtype(dt)], what=name_of(dt, n) + (" c" if with_c else ""))
        if first is None:
            first = out["logdet"]
        assert np.array_equal(out["logdet"], first), (n, dt, D, Q)  # logdet depends on neither D nor Q


@pytest.mark.parametrize("n", MT.TILE_SIZES + MT.GLOBAL_SIZES)
def test_accuracy(n):
    for dt in DTYPES:
        for with_c in (True, False):
            accuracy(n, dt, with_c, MT.DQ + ((33, 0),))


@pytest.mark.parametrize("dt", DTYPES)
def test_accuracy_1024(dt):
    accuracy(1024, dt, True, (MT.DQ_1024,))


@pytest.mark.parametrize("n", [33, 64, 96, 130])
def test_optional_outputs(n):
    for dt in DTYPES:
        B, c, Ys, As, _ = MT.case(n, np.dtype(dt).name, True)
        D, Q = 17, 16
        y, a = MT.first(Ys, n, MT.DMAX, D), MT.first(As, n, MT.QMAX, Q)
        out, info = gpu(n, B, c, y, a)
        assert not info.any()
        # each output alone, and alpha + mean: the bits of the all-outputs call
        for want in [(k,) for k in MT.OUTPUTS] + [("alpha", "mean")]:
            o, i = gpu(n, B, c, y, a if "mean" in want else None, want=want)
            MT.same_bits(o, {k: out[k] for k in want}, (n, dt, want))
            assert not i.any()
        # logdet alone reads neither Y nor A: dYs = NULL, ntarget = 0
        o, _ = gpu(n, B, c, None, None, want=("logdet",))
        assert np.array_equal(o["logdet"], out["logdet"])
        # the raw C entry point on tensors larger than the call: the tails and the info tail stay as they were
        batch = B.size // (n * n)
        sizes = dict(alpha=batch * D * n, quad=batch * D, logdet=batch, logml=batch * D, mean=batch * D * Q)
        t = lambda x: torch.tensor(np.ascontiguousarray(x)).cuda()  # noqa: E731
        ins = [t(B), t(c), t(y), t(a)]
        outs = {k: torch.full((sizes[k] + 7,), -7.5, dtype=ins[0].dtype, device="cuda") for k in MT.OUTPUTS}
        info = torch.full((batch + 3,), -7, dtype=torch.int32, device="cuda")
        ptr = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
        torch.cuda.synchronize()
        rc = lib.lib().matinv_multi_target_batched(api.F64 if dt is np.float64 else api.F32, n, D, Q, *[ptr(x) for x in ins],
                                                   *[ptr(outs[k]) for k in MT.OUTPUTS], batch, ptr(info), None)
        torch.cuda.synchronize()
        assert rc == lib.OK
        for k in MT.OUTPUTS:
            got = outs[k].cpu().numpy()
            assert np.array_equal(got[:sizes[k]], out[k]) and (got[sizes[k]:] == -7.5).all(), (n, dt, k)
        got = info.cpu().numpy()
        assert not got[:batch].any() and (got[batch:] == -7).all()


@pytest.mark.parametrize("n", [33, 64, 95, 130])
def test_locality(n):
    for dt in DTYPES:
        B, c, Ys, As, _ = MT.case(n, np.dtype(dt).name, True)
        batch = B.size // (n * n)
        out, info = gpu(n, B, c, Ys, As)  # D = 33, Q = 33
        assert not info.any()
        per = dict(alpha=n, quad=1, logml=1, mean=MT.QMAX)
        o33 = {k: out[k].reshape(batch, MT.DMAX, per[k]) for k in per}
        # a target alone gives the bits it has as target 0, 15, 16 and 32 of D = 33
        for t in (0, 15, 16, 32):
            o1, _ = gpu(n, B, c, MT.first(Ys, n, MT.DMAX, [t]), As)
            for k in per:
                assert np.array_equal(o1[k].reshape(batch, per[k]), o33[k][:, t]), (n, dt, t, k)
            assert np.array_equal(o1["logdet"], out["logdet"])
        # ... and targets 16 .. 32 as a call of their own, in other lanes and another group
        o17, _ = gpu(n, B, c, MT.first(Ys, n, MT.DMAX, slice(16, 33)), As)
        for k in per:
            assert np.array_equal(o17[k].reshape(batch, 17, per[k]), o33[k][:, 16:]), (n, dt, k)
        # the same for the queries in mean
        m33 = o33["mean"]
        for j in (0, 15, 16, 32):
            o1, _ = gpu(n, B, c, Ys, MT.first(As, n, MT.QMAX, [j]), want=("mean",))
            assert np.array_equal(o1["mean"].reshape(batch, MT.DMAX), m33[:, :, j]), (n, dt, j)
        o17, _ = gpu(n, B, c, Ys, MT.first(As, n, MT.QMAX, slice(16, 33)), want=("mean",))
        assert np.array_equal(o17["mean"].reshape(batch, MT.DMAX, 17), m33[:, :, 16:]), (n, dt)
        # matrix k alone
        k1 = batch - 2
        row = lambda x: x.reshape(batch, -1)[k1]  # noqa: E731
        ok, ik = gpu(n, row(B), row(c), row(Ys), row(As))
        MT.same_bits(ok, {k: row(v) for k, v in out.items()}, (n, dt, "matrix alone"))
        assert ik[0] == 0


@pytest.mark.parametrize("n", [17, 64, 100])
def test_not_positive_definite(n):
    for dt in DTYPES:
        for with_c in (True, False):
            B, c, Ys, As, _ = MT.case(n, np.dtype(dt).name, with_c)
            D, Q = 17, 16
            y, a = MT.first(Ys, n, MT.DMAX, D), MT.first(As, n, MT.QMAX, Q)
            out, _ = gpu(n, B, c, y, a)
            Bb, cb = np.array(B), (None if c is None else np.array(c))
            want_info = MT.break_three(Bb, cb, n, (1, 3, 4))
            assert want_info == {1: n, 3: 2, 4: 1}
            ob, info = gpu(n, Bb, cb, y, a)
            MT.check_with_rejects(ob, info, Bb, cb, y, a, n, D, Q, dt, want_info, name_of(dt, n) + " rejects")
            # the neighbours keep their bits
            batch = info.size
            ok = [k for k in range(batch) if k not in want_info]
            for k in MT.OUTPUTS:
                assert np.array_equal(ob[k].reshape(batch, -1)[ok], out[k].reshape(batch, -1)[ok]), (n, dt, k)
            # each output alone is NaN there as well
            for k in MT.OUTPUTS:
                o1, i1 = gpu(n, Bb, cb, None if k == "logdet" else y, a if k == "mean" else None, want=(k,))
                assert np.array_equal(i1, info) and np.array_equal(o1[k], ob[k], equal_nan=True), (n, dt, k)


@pytest.mark.parametrize("n", [16, 64, 96, 130])
def test_agreement_with_the_single_target_entry_points(n):
    """D = 1 against logml_batched, logml_grad_batched(want=("alpha",)) and predict_batched(want=("mean",)): each side is within one bound
    of the reference, so they are within two of each other"""
    for dt in DTYPES:
        B, c, Ys, As, full = MT.case(n, np.dtype(dt).name, True)
        y = MT.first(Ys, n, MT.DMAX, 1)
        out, info = gpu(n, B, c, y, As)
        assert not info.any()
        t = lambda x: torch.tensor(np.ascontiguousarray(x)).cuda()  # noqa: E731
        tb, tc, ty, ta = t(B), t(c), t(y), t(As)
        logml = api.logml_batched(n, tb, tc, ty)
        _, _, alpha = api.logml_grad_batched(n, tb, tc, ty, None, want=("alpha",))
        mean, _ = api.predict_batched(n, tb, tc, ty, ta, None, want=("mean",))
        torch.cuda.synchronize()
        single = dict(logml=logml.cpu().numpy(), alpha=alpha.cpu().numpy(), mean=mean.cpu().numpy())
        ref = MT.take(full, 1, MT.QMAX)
        u = U[np.dtype(dt)]
        MT.check(single, ref, n, u, what=f"single-target entry points n={n}")
        b = MT.bounds(ref, n, u)
        shp = MT.shapes(ref, n)
        for k, v in single.items():
            diff = np.abs(out[k].reshape(shp[k]).astype(np.float64) - v.reshape(shp[k]).astype(np.float64))
            assert (diff <= 2 * b[k]).all(), (n, dt, k, float((diff / b[k]).max()))


@pytest.mark.parametrize("n", [40, 100])
def test_host_form_equals_device_form(n):
    for dt in DTYPES:
        B, c, Ys, As, _ = MT.case(n, np.dtype(dt).name, True)
        y, a = MT.first(Ys, n, MT.DMAX, 17), MT.first(As, n, MT.QMAX, 16)
        out, _ = gpu(n, B, c, y, a)
        al, qd, ld, lm, mn, info = api.multi_target_batched_host(n, B, c, y, a)
        assert not info.any()
        MT.same_bits(dict(alpha=al, quad=qd, logdet=ld, logml=lm, mean=mn), out, (n, dt, "host"))
        al, qd, ld, lm, mn, info = api.multi_target_batched_host(n, B, c, None, None, want=("logdet",))
        assert al is None and qd is None and lm is None and mn is None and not info.any() and np.array_equal(ld, out["logdet"])


def test_grid_stride_and_chunking():
    """one process with the grid held to one round of resident workgroups and the workspace cap at 1 MiB: tests/_multi_target_worker.py"""
    e = dict(os.environ)
    e.update({"MATINV_TILE_GRID_MULT": "1", "MATINV_BLOCKED_WS_MB": "1"})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_multi_target_worker.py")], capture_output=True, text=True, env=e,
                       timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "multi-target-worker ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
