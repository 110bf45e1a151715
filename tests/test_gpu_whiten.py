"""GPU tests of the batched whitening W = chol(C)^-1 (X - m), the squared Mahalanobis distances, the log-determinant and the Gaussian
log-density (matinv_whiten_batched): every output against float64 / longdouble numpy (bounds (3) - (5) derived in
tests/_whiten_worker.py, not fitted), the round trip through matinv_colour_batched, bit locality (point position, batch, requested
outputs, m = None, X = m, grid rounds, workspace chunks), strided C, the not-positive-definite contract and the host form.

Worst err / bound seen on an MI355X (printed by every run; DESIGN.md, "Whitening", Accuracy), all at q = 1: W 0.059 (tile fp64), 0.077 (tile
fp32); maha 0.065, 0.072; logdet 0.64, 0.45; logpdf 0.47, 0.41. From q = 15 on W stays below 0.004 and logdet below 0.02; the global form
below 0.003 everywhere; 0.048 (logdet) on the set scaled by 1e-30; the round trip 0.004."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _colour_worker as CW
import _whiten_worker as W
from conftest import pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
api = pkg("api")
lib = pkg("_lib")
U = W.U
DTYPES = (np.float64, np.float32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu_whiten(q, C, m, X, want=W.OUTPUTS, **kw):
    """(dict of numpy outputs, info)"""
    return W.run(api, torch, q, C, m, X, want=want, **kw)


def name_of(dt, q):
    name = api.whiten_kernel_name(dt, q)
    assert name.startswith("matinv_spd_tile_f" if q <= 96 else "matinv_chol_global<")
    assert name.endswith(", true, true, true, true, true, true, true>")
    return name


@pytest.mark.parametrize("q", W.QSIZES)
def test_accuracy(q):
    for dt in DTYPES:
        C, m, X = W.case(q, np.dtype(dt).name)
        first = None
        for S in W.SS:
            x = W.samples(X, q, slice(0, S))
            out, info = gpu_whiten(q, C, m, x)
            assert not info.any(), (q, dt, info)
            assert all(v.dtype == np.dtype(dt) for v in out.values())
            W.check(out, W.take(W.case_reference(q, np.dtype(dt).name), slice(0, S)), q, U[np.dtype(dt)], what=name_of(dt, q))
            if first is None:
                first = out["logdet"]
            assert np.array_equal(out["logdet"], first), (q, dt, S)  # logdet does not depend on S


@pytest.mark.parametrize("q", [17, 96, 130])
def test_nothing_is_squared_out_of_range(q):
    """C scaled by 1e-30 (fp64): its factor is of order 1e-15, W of order 1e15, maha of order 1e30 and det C far below the smallest
    float64; the same relative bounds, and a finite logdet"""
    C, m, X = W.case(q, "float64", 50, 1e-30)
    x = W.samples(X, q, slice(0, 17))
    out, info = gpu_whiten(q, C, m, x)
    assert not info.any()
    assert np.isfinite(out["logdet"]).all() and (out["logdet"] < -60 * q).all()
    ref = W.take(W.case_reference(q, "float64", 50, 1e-30), slice(0, 17))
    W.check(out, ref, q, U[np.dtype(np.float64)], what=name_of(np.float64, q) + " 1e-30")


@pytest.mark.parametrize("dt", DTYPES)
def test_accuracy_1024(dt):
    q = 1024
    C, m, X = W.case(q, np.dtype(dt).name, 2)
    x = W.samples(X, q, slice(0, 1))
    out, info = gpu_whiten(q, C, m, x)
    assert not info.any()
    W.check(out, W.whiten_reference(C, m, x, q), q, U[np.dtype(dt)], what=name_of(dt, q))


@pytest.mark.parametrize("q", [15, 33, 96, 97])
def test_round_trip_through_colour(q):
    """whiten(C, m, colour(C, m, Z).Y) returns Z within bound (3) plus |Lh^-1| times the bound (2) of _colour_worker on Y, which is one
    more perturbation of the right-hand side"""
    for dt in DTYPES:
        C, m, Z = W.case(q, np.dtype(dt).name)
        z = W.samples(Z, q, slice(0, 17))
        t = lambda a: torch.tensor(np.ascontiguousarray(a)).cuda()  # noqa: E731
        Y, _ = api.colour_batched(q, t(C), t(m), t(z), want=("Y",))
        torch.cuda.synchronize()
        Y = Y.cpu().numpy()
        out, info = gpu_whiten(q, C, m, Y, want=("W",))
        assert not info.any()
        u = U[np.dtype(dt)]
        yb = CW.y_bound(CW.reference(C, m, z, q), q, u)
        # the reference of the exact pair: x = Yh = m + Lh z, whose W is z itself
        ref = W.whiten_reference(C, m, Y, q)
        ref["W"] = np.asarray(z, dtype=np.float64).reshape(ref["z"].shape)
        got = {"W": out["W"]}
        W.check(got, ref, q, u, what=name_of(dt, q) + " round trip", extra_r=yb)


@pytest.mark.parametrize("q", [15, 33, 96, 97])
def test_locality(q):
    for dt in DTYPES:
        C, m, X = W.case(q, np.dtype(dt).name)
        batch = W.BATCH
        out, info = gpu_whiten(q, C, m, X)  # S = 33
        assert not info.any()
        per = dict(W=q, maha=1, logpdf=1)
        o33 = {k: out[k].reshape(batch, CW.SMAX, per[k]) for k in per}
        # a point alone gives the bits it has as column 0, 15, 16 and 32 of S = 33
        for s in (0, 15, 16, 32):
            o1, _ = gpu_whiten(q, C, m, W.samples(X, q, [s]))
            for k in per:
                assert np.array_equal(o1[k].reshape(batch, per[k]), o33[k][:, s]), (q, dt, s, k)
            assert np.array_equal(o1["logdet"], out["logdet"])
        # ... and among 17, in another lane
        o17, _ = gpu_whiten(q, C, m, W.samples(X, q, [16, 3] + list(range(17, 32))))
        for k in per:
            assert np.array_equal(o17[k].reshape(batch, 17, per[k])[:, :2], o33[k][:, [16, 3]]), (q, dt, k)
        # matrix k alone
        k1 = 101
        ok, ik = gpu_whiten(q, C.reshape(batch, -1)[k1], m.reshape(batch, -1)[k1], X.reshape(batch, -1)[k1])
        W.same_bits(ok, {k: v.reshape(batch, -1)[k1] for k, v in out.items()}, (q, dt, "matrix alone"))
        assert ik[0] == 0
        # which outputs are requested changes no bit of the others: each alone, each left out, and a pair
        subsets = [(k,) for k in W.OUTPUTS] + [tuple(k for k in W.OUTPUTS if k != o) for o in W.OUTPUTS] + [("maha", "logdet")]
        for want in subsets:
            o2, i2 = gpu_whiten(q, C, m, X, want=want)
            W.same_bits(o2, {k: out[k] for k in want}, (q, dt, want))
            assert not i2.any()
        # logdet alone does not read X
        o3, _ = gpu_whiten(q, C, None, None, want=("logdet",))
        assert np.array_equal(o3["logdet"], out["logdet"])
        # m = None is m = 0
        o4, _ = gpu_whiten(q, C, None, X)
        o5, _ = gpu_whiten(q, C, np.zeros_like(m), X)
        W.same_bits(o4, o5, (q, dt, "m = None"))
        # X = m: W compares equal to zero, as +0.0 (include/matinv.h), and maha is +0.0
        xm = np.ascontiguousarray(np.broadcast_to(m.reshape(batch, 1, q), (batch, 17, q))).reshape(-1)
        o6, _ = gpu_whiten(q, C, m, xm)
        assert (o6["W"] == 0).all() and (o6["maha"] == 0).all()
        assert not np.signbit(o6["W"]).any() and not np.signbit(o6["maha"]).any()
        assert np.array_equal(o6["logpdf"].reshape(batch, 17), np.broadcast_to(o6["logpdf"].reshape(batch, 17)[:, :1], (batch, 17)))
        W.check(o6, W.whiten_reference(C, m, xm, q), q, U[np.dtype(dt)], what=name_of(dt, q) + " X = m")


def test_strided_input():
    """matrix k at k * strideC with strideC > q * q and NaN in the gap: the bits of the packed call"""
    q, batch = 33, 50
    C, m, X = W.case(q, "float64", batch)
    stride = q * q + 7
    padded = np.full((batch, stride), np.nan)
    padded[:, :q * q] = C.reshape(batch, -1)
    out, _ = gpu_whiten(q, C, m, X)
    o, info = gpu_whiten(q, padded.reshape(-1), m, X, stride=stride, batch=batch)
    assert not info.any()
    W.same_bits(o, out, "strided")


@pytest.mark.parametrize("q", [33, 97])
def test_not_positive_definite(q):
    for dt in DTYPES:
        C, m, X = W.case(q, np.dtype(dt).name)
        batch = W.BATCH
        x = W.samples(X, q, slice(0, 17))
        out, _ = gpu_whiten(q, C, m, x)
        cols = {10: 1, 11: 16, 57: 17, 199: q}
        broken = W.break_many(C, q, cols)
        ob, info = gpu_whiten(q, broken, m, x)
        expect = np.zeros(batch, dtype=np.int64)
        for k, j in cols.items():
            expect[k] = j
        assert np.array_equal(info, expect), (q, dt, info[sorted(cols)], cols)
        bad = sorted(cols)
        ok = [k for k in range(batch) if k not in cols]
        for k in W.OUTPUTS:
            assert np.isnan(ob[k].reshape(batch, -1)[bad]).all(), (q, dt, k)
            # the neighbours keep their bits
            assert np.array_equal(ob[k].reshape(batch, -1)[ok], out[k].reshape(batch, -1)[ok]), (q, dt, k)
        # each output alone is NaN as well
        for k in W.OUTPUTS:
            o1, i1 = gpu_whiten(q, broken, m, None if k == "logdet" else x, want=(k,))
            assert np.array_equal(i1, expect) and np.array_equal(o1[k], ob[k], equal_nan=True), (q, dt, k)


@pytest.mark.parametrize("q", [17, 97])
def test_host_form_equals_device_form(q):
    for dt in DTYPES:
        C, m, X = W.case(q, np.dtype(dt).name, 20)
        x = W.samples(X, q, slice(0, 17))
        out, _ = gpu_whiten(q, C, m, x)
        w, mh, ld, lp, info = api.whiten_batched_host(q, C, m, x)
        assert not info.any()
        W.same_bits(dict(W=w, maha=mh, logdet=ld, logpdf=lp), out, (q, dt, "host"))
        w, mh, ld, lp, info = api.whiten_batched_host(q, C, None, None, want=("logdet",))
        assert w is None and mh is None and lp is None and not info.any() and np.array_equal(ld, out["logdet"])


def test_grid_stride_and_chunking():
    """one process with the grid held to one round of resident workgroups and the workspace cap at 1 MiB: tests/_whiten_worker.py"""
    e = dict(os.environ)
    e.update({"MATINV_TILE_GRID_MULT": "1", "MATINV_BLOCKED_WS_MB": "1"})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_whiten_worker.py")], capture_output=True, text=True, env=e,
                       timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "whiten-worker ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
