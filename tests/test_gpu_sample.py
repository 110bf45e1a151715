"""GPU tests of the joint posterior samples of a GP at its query points (matinv_sample_batched): mean and cov carry the bits of
predict_cov_batched, Y the bits of colour_batched on them, whatever is requested; the zero-mean form; the info codes of the two stages;
and one end-to-end check against float64 numpy (bounds derived in tests/_colour_worker.py and tests/_predict_cov_worker.py)."""
import numpy as np
import pytest

import _colour_worker as W
import _predict_cov_worker as PC
from conftest import pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
api = pkg("api")
lib = pkg("_lib")
DTYPES = (np.float64, np.float32)
SHAPES = [(n, nquery) for n in (1, 16, 17, 96, 97) for nquery in (1, 16, 17, 33)] + [(33, 97)]
BATCH = W.SAMPLE_BATCH


def dev(x):
    return None if x is None else torch.tensor(np.ascontiguousarray(x)).cuda()  # a copy: the shared cases are read-only arrays


def gpu_sample(n, B, c, d, As, Es, Z, want=("Y", "mean", "cov")):
    """(Y, mean, cov, info) as numpy (None for what was not asked for); checks that the inputs are bitwise unchanged"""
    ts = [dev(x) for x in (B, c, d, As, Es, Z)]
    info = torch.full((B.size // (n * n),), -7, dtype=torch.int32, device="cuda")
    out = api.sample_batched(n, *ts, info=info, want=want)
    torch.cuda.synchronize()
    for t, x in zip(ts, (B, c, d, As, Es, Z)):
        assert x is None or np.array_equal(t.cpu().numpy(), x, equal_nan=True), "an input was modified"
    return tuple(None if o is None else o.cpu().numpy() for o in out) + (info.cpu().numpy(),)


def gpu_cov(n, B, c, d, As, Es, want=("mean", "cov")):
    info = torch.full((B.size // (n * n),), -7, dtype=torch.int32, device="cuda")
    mean, cov = api.predict_cov_batched(n, dev(B), dev(c), dev(d), dev(As), dev(Es), info=info, want=want)
    torch.cuda.synchronize()
    return (None if mean is None else mean.cpu().numpy()), cov.cpu().numpy(), info.cpu().numpy()


def gpu_colour_y(q, C, m, Z):
    info = torch.full((C.size // (q * q),), -7, dtype=torch.int32, device="cuda")
    Y, _ = api.colour_batched(q, dev(C), dev(m), dev(Z), info=info, want=("Y",))
    torch.cuda.synchronize()
    return Y.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("n,nquery", SHAPES)
def test_two_stages_bit_for_bit(n, nquery):
    for dt in DTYPES:
        B, c, d, As, Es, Z = W.sample_case(n, nquery, np.dtype(dt).name)
        for S in (1, 17):
            z = W.samples(Z, nquery, slice(0, S))
            Y, mean, cov, info = gpu_sample(n, B, c, d, As, Es, z)
            assert not info.any(), (n, nquery, dt, info)
            m0, c0, _ = gpu_cov(n, B, c, d, As, Es)
            assert np.array_equal(mean, m0) and np.array_equal(cov, c0)
            y0, i0 = gpu_colour_y(nquery, c0, m0, z)
            assert not i0.any() and np.array_equal(Y, y0)
            # the same bits whether or not mean / cov are requested
            for want in (("Y",), ("Y", "mean"), ("Y", "cov")):
                y1, m1, c1, i1 = gpu_sample(n, B, c, d, As, Es, z, want=want)
                assert np.array_equal(y1, Y) and not i1.any(), want
                assert (m1 is None) == ("mean" not in want) and (c1 is None) == ("cov" not in want)
                assert (m1 is None or np.array_equal(m1, mean)) and (c1 is None or np.array_equal(c1, cov))
            # d = None: the zero-mean posterior
            y2, m2, c2, i2 = gpu_sample(n, B, c, None, As, Es, z, want=("Y", "cov"))
            yz, _ = gpu_colour_y(nquery, c0, None, z)
            assert m2 is None and not i2.any() and np.array_equal(c2, cov) and np.array_equal(y2, yz)


@pytest.mark.parametrize("n,nquery", [(17, 17), (97, 16), (33, 97)])
def test_info_of_the_two_stages(n, nquery):
    for dt in DTYPES:
        B, c, d, As, Es, Z = W.sample_case(n, nquery, np.dtype(dt).name)
        z = W.samples(Z, nquery, slice(0, 17))
        # E = 0: cov = -a K a^T, whose first pivot is negative: info = n + 1, Y NaN, cov finite and the covariance route's
        e0 = np.zeros_like(Es)
        Y, mean, cov, info = gpu_sample(n, B, c, d, As, e0, z)
        m0, c0, _ = gpu_cov(n, B, c, d, As, e0)
        assert (info == n + 1).all(), (n, nquery, dt, info)
        assert np.isnan(Y).all() and np.isfinite(cov).all() and np.array_equal(cov, c0) and np.array_equal(mean, m0)
        y1, _, _, i1 = gpu_sample(n, B, c, d, As, e0, z, want=("Y",))
        assert (i1 == n + 1).all() and np.isnan(y1).all()
        # M not positive definite in two matrices, first bad pivot at column 1 and at column n; the others keep their bits
        Yg, meang, covg, _ = gpu_sample(n, B, c, d, As, Es, z)
        Bb, cb = np.array(B), np.array(c)
        cb.reshape(BATCH, n)[[1, 4]] = 0
        mb = Bb.reshape(BATCH, n, n)
        mb[1, 0, 0] = -1.0
        mb[4, n - 1, n - 1] = -1e6
        expect = np.zeros(BATCH, dtype=np.int64)
        expect[1], expect[4] = 1, n
        for want in (("Y", "mean", "cov"), ("Y",)):
            Y, mean, cov, info = gpu_sample(n, Bb, cb, d, As, Es, z, want=want)
            assert np.array_equal(info, expect), (n, nquery, dt, info)
            ok = [0, 2, 3, 5]
            for got, good in ((Y, Yg), (mean, meang), (cov, covg)):
                if got is not None:
                    assert np.isnan(got.reshape(BATCH, -1)[[1, 4]]).all()
                    assert np.array_equal(got.reshape(BATCH, -1)[ok], good.reshape(BATCH, -1)[ok])


@pytest.mark.parametrize("n,nquery", [(16, 17), (96, 33), (97, 16), (33, 97)])
def test_end_to_end_accuracy(n, nquery):
    for dt in DTYPES:
        u = W.U[np.dtype(dt)]
        B, c, d, As, Es, Z = W.sample_case(n, nquery, np.dtype(dt).name)
        z = W.samples(Z, nquery, slice(0, 17))
        Y, mean, cov, info = gpu_sample(n, B, c, d, As, Es, z)
        assert not info.any()
        cref, ref = W.sample_reference(B, c, d, As, Es, z, n, nquery)
        PC.check(mean, cov, cref, n, u, what=f"sample n={n}")
        b_mean, b_cov = PC.bounds(cref, n, u)
        W.check_y(Y, ref, nquery, u, what=f"sample n={n} {api.colour_kernel_name(dt, nquery)}", dcov=b_cov, dmean=b_mean)


@pytest.mark.parametrize("n,nquery", [(17, 16), (97, 97)])
def test_host_form_equals_device_form(n, nquery):
    for dt in DTYPES:
        B, c, d, As, Es, Z = W.sample_case(n, nquery, np.dtype(dt).name)
        z = W.samples(Z, nquery, slice(0, 17))
        Y, mean, cov, _ = gpu_sample(n, B, c, d, As, Es, z)
        y, m, v, info = api.sample_batched_host(n, B, c, d, As, Es, z, want=("Y", "mean", "cov"))
        assert not info.any() and np.array_equal(y, Y) and np.array_equal(m, mean) and np.array_equal(v, cov)
        y, m, v, info = api.sample_batched_host(n, B, c, d, As, Es, z)
        assert m is None and v is None and not info.any() and np.array_equal(y, Y)
