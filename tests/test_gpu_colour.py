"""GPU tests of the batched Cholesky factor and the coloured samples Y = m + chol(C) Z (matinv_colour_batched): structure, the backward
error of the factor and the forward error of Y against float64 numpy (bounds derived in tests/_colour_worker.py, not fitted), bit locality
(sample position, batch, requested outputs, Z = 0, grid rounds, workspace chunks) and the not-positive-definite contract.

Worst err / bound seen on an MI355X (printed by every run; DESIGN.md, "Posterior samples", Accuracy): factor 0.19 (tile fp64), 0.17 (tile fp32),
0.14 (global form); Y 0.40 (fp64), 0.41 (fp32), 0.35 on the set scaled by 1e-30."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _colour_worker as W
from conftest import pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
api = pkg("api")
lib = pkg("_lib")
U = W.U
DTYPES = (np.float64, np.float32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(x):
    return None if x is None else torch.tensor(np.ascontiguousarray(x)).cuda()  # a copy: the shared cases are read-only arrays


def gpu_colour(q, C, m, Z, want=("Y", "L")):
    """(Y, L, info) as numpy (None for what was not asked for); checks that the inputs are bitwise unchanged"""
    tc, tm, tz = dev(C), dev(m), dev(Z)
    batch = C.size // (q * q)
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    Y, L = api.colour_batched(q, tc, tm, tz, info=info, want=want)
    torch.cuda.synchronize()
    for t, x in ((tc, C), (tm, m), (tz, Z)):
        assert x is None or np.array_equal(t.cpu().numpy(), x, equal_nan=True), "an input was modified"
    Y, L = (None if o is None else o.cpu().numpy() for o in (Y, L))
    return Y, L, info.cpu().numpy()


def name_of(dt, q):
    name = api.colour_kernel_name(dt, q)
    assert name.startswith("matinv_spd_tile_f" if q <= 96 else "matinv_chol_global<") and name.endswith(", true, true, true, true, true, true>")
    return name


@pytest.mark.parametrize("q", W.QSIZES)
def test_structure_and_accuracy(q):
    for dt in DTYPES:
        C, m, Z = W.case(q, np.dtype(dt).name)
        first = None
        for S in W.SS:
            z = W.samples(Z, q, slice(0, S))
            Y, L, info = gpu_colour(q, C, m, z)
            assert not info.any(), (q, dt, info)
            ref = W.reference(C, m, z, q)
            if first is None:  # L does not depend on S: checked once, compared bit for bit afterwards
                first = L
                W.check_factor(L, ref, q, U[np.dtype(dt)], what=name_of(dt, q))
            assert np.array_equal(L, first), (q, dt, S)
            W.check_y(Y, ref, q, U[np.dtype(dt)], what=name_of(dt, q))


@pytest.mark.parametrize("q", [17, 96, 130])
def test_nothing_is_squared_out_of_range(q):
    """C scaled by 1e-30 (fp64): its factor is of order 1e-15 and its pivots of order 1e-30; the same relative bounds"""
    C, m, Z = W.case(q, "float64", 50, 1e-30)
    z = W.samples(Z, q, slice(0, 17))
    Y, L, info = gpu_colour(q, C, m, z)
    assert not info.any()
    ref = W.reference(C, m, z, q)
    W.check_factor(L, ref, q, U[np.dtype(np.float64)], what=name_of(np.float64, q) + " 1e-30")
    W.check_y(Y, ref, q, U[np.dtype(np.float64)], what=name_of(np.float64, q) + " 1e-30")


@pytest.mark.parametrize("dt", DTYPES)
def test_accuracy_1024(dt):
    q = 1024
    C, m, Z = W.case(q, np.dtype(dt).name, 2)
    z = W.samples(Z, q, slice(0, 1))
    Y, L, info = gpu_colour(q, C, m, z)
    assert not info.any()
    ref = W.reference(C, m, z, q)
    W.check_factor(L, ref, q, U[np.dtype(dt)], what=name_of(dt, q))
    W.check_y(Y, ref, q, U[np.dtype(dt)], what=name_of(dt, q))


@pytest.mark.parametrize("q", [15, 33, 96, 97])
def test_locality(q):
    for dt in DTYPES:
        C, m, Z = W.case(q, np.dtype(dt).name)
        batch = W.BATCH
        Y, L, info = gpu_colour(q, C, m, Z)  # S = 33
        y33 = Y.reshape(batch, W.SMAX, q)
        # a sample alone gives the bits it has as column 0, 15, 16 and 32 of S = 33
        for s in (0, 15, 16, 32):
            y1, l1, _ = gpu_colour(q, C, m, W.samples(Z, q, [s]))
            assert np.array_equal(y1.reshape(batch, q), y33[:, s]), (q, dt, s)
            assert np.array_equal(l1, L)
        # ... and among 17, in another lane
        y17, _, _ = gpu_colour(q, C, m, W.samples(Z, q, [16, 3] + list(range(17, 32))))
        assert np.array_equal(y17.reshape(batch, 17, q)[:, :2], y33[:, [16, 3]])
        # matrix k alone
        k = 101
        yk, lk, ik = gpu_colour(q, C.reshape(batch, -1)[k], m.reshape(batch, -1)[k], Z.reshape(batch, -1)[k])
        assert np.array_equal(yk, Y.reshape(batch, -1)[k]) and np.array_equal(lk, L.reshape(batch, -1)[k]) and ik[0] == 0
        # which outputs are requested changes no bit of the others; m = None is m = 0; Z is not read without Y
        y2, l2, _ = gpu_colour(q, C, m, Z, want=("Y",))
        assert l2 is None and np.array_equal(y2, Y)
        y3, l3, _ = gpu_colour(q, C, None, None, want=("L",))
        assert y3 is None and np.array_equal(l3, L)
        y4, _, _ = gpu_colour(q, C, None, Z, want=("Y",))
        y5, _, _ = gpu_colour(q, C, np.zeros_like(m), Z, want=("Y",))
        assert np.array_equal(y4, y5)
        # Z = 0 returns the bits of m
        z0 = np.zeros(batch * 17 * q, dtype=dt)
        y0, _, _ = gpu_colour(q, C, m, z0)
        assert np.array_equal(y0.reshape(batch, 17, q), np.broadcast_to(m.reshape(batch, 1, q), (batch, 17, q)))


def test_strided_input():
    """matrix k at k * strideC with strideC > q * q: the bits of the packed call"""
    q, batch, dt = 33, 50, np.float64
    C, m, Z = W.case(q, "float64", batch)
    stride = q * q + 7
    padded = np.full((batch, stride), np.nan)
    padded[:, :q * q] = C.reshape(batch, -1)
    Y, L, _ = gpu_colour(q, C, m, Z)
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    y, l = api.colour_batched(q, dev(padded.reshape(-1)), dev(m), dev(Z), info=info, strideC=stride, batchSize=batch)
    torch.cuda.synchronize()
    assert not info.cpu().numpy().any()
    assert np.array_equal(y.cpu().numpy(), Y) and np.array_equal(l.cpu().numpy(), L)


@pytest.mark.parametrize("q", [33, 97])
def test_not_positive_definite(q):
    for dt in DTYPES:
        C, m, Z = W.case(q, np.dtype(dt).name)
        batch = W.BATCH
        z = W.samples(Z, q, slice(0, 17))
        Y, L, _ = gpu_colour(q, C, m, z)
        cols = {10: 1, 11: 16, 57: 17, 199: q}
        broken = C
        for k, j in cols.items():
            broken = W.break_at(broken, q, k, j)
        yb, lb, info = gpu_colour(q, broken, m, z)
        expect = np.zeros(batch, dtype=np.int64)
        for k, j in cols.items():
            expect[k] = j
        assert np.array_equal(info, expect), (q, dt, info[sorted(cols)], cols)
        bad = sorted(cols)
        ok = [k for k in range(batch) if k not in cols]
        assert np.isnan(yb.reshape(batch, -1)[bad]).all() and np.isnan(lb.reshape(batch, -1)[bad]).all()
        # the neighbours keep their bits
        assert np.array_equal(yb.reshape(batch, -1)[ok], Y.reshape(batch, -1)[ok])
        assert np.array_equal(lb.reshape(batch, -1)[ok], L.reshape(batch, -1)[ok])
        # each output alone is NaN as well
        y1, _, i1 = gpu_colour(q, broken, m, z, want=("Y",))
        _, l1, i2 = gpu_colour(q, broken, None, None, want=("L",))
        assert np.array_equal(i1, expect) and np.array_equal(i2, expect)
        assert np.array_equal(y1, yb, equal_nan=True) and np.array_equal(l1, lb, equal_nan=True)


@pytest.mark.parametrize("q", [17, 97])
def test_host_form_equals_device_form(q):
    for dt in DTYPES:
        C, m, Z = W.case(q, np.dtype(dt).name, 20)
        z = W.samples(Z, q, slice(0, 17))
        Y, L, _ = gpu_colour(q, C, m, z)
        y, l, info = api.colour_batched_host(q, C, m, z)
        assert not info.any() and np.array_equal(y, Y) and np.array_equal(l, L)
        y, l, info = api.colour_batched_host(q, C, None, None, want=("L",))
        assert y is None and not info.any() and np.array_equal(l, L)


def test_grid_stride_and_chunking():
    """one process with the grid held to one round of resident workgroups and the workspace cap at 1 MiB: tests/_colour_worker.py"""
    e = dict(os.environ)
    e.update({"MATINV_TILE_GRID_MULT": "1", "MATINV_BLOCKED_WS_MB": "1"})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_colour_worker.py")], capture_output=True, text=True, env=e,
                       timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "colour-worker ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
