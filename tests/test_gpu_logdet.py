"""Batched log-determinant (matinv_logdet_batched) and GP log marginal likelihood (matinv_logml_batched) on the GPU against numpy
in float64 (np.linalg.slogdet, np.linalg.solve) on the float64 image of exactly the input the kernel was given (for the Cholesky
contract and logml: of the lower triangle it reads).

Bound per matrix, first order and not tuned (u = 2^-53 in fp64, 2^-24 in fp32):

    |logabsdet - want| <= n^2 * u * cond2(A_k) + n * u * max(1, |want|)

A backward error of n*u relative to A moves log det by at most n * ||A^-1|| * ||dA||, and n additions of logarithms each round by
at most u times the partial sum. logml: half of that, plus for q = d^T M^-1 d the relative tolerance test_gpu_solve.py applies to a
solve: 0.5*|q|*max(1e-10, 1e-15*cond*n) in fp64, 0.5*|q|*1e-5*cond in fp32.
"""
import ctypes
import math

import numpy as np
import pytest

from conftest import as_mats, general_batch, pkg, read_ref, spd_batch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
api = pkg("api")
GJ, CH = api.ALGO_GAUSS_JORDAN, api.ALGO_CHOLESKY
AUTO, TILE, ROW, GLOBAL = api.KERNEL_AUTO, api.KERNEL_TILE, api.KERNEL_ROW, api.KERNEL_GLOBAL
U = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}
DTYPES = (np.float64, np.float32)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def lower_image(a, n):
    """(batch, n, n) float64 matrices built from the lower triangles of a flat column-major batch: what ALGO_CHOLESKY reads"""
    m = as_mats(a, n).astype(np.float64)
    lo = np.tril(m)
    return lo + np.tril(m, -1).transpose(0, 2, 1)


def full_image(a, n):
    return as_mats(a, n).astype(np.float64)


def bound(mat, want, n, u):
    return n * n * u * np.linalg.cond(mat) + n * u * max(1.0, abs(want))


def families(algo, n):
    fam = [AUTO, GLOBAL]
    if algo == CH and n <= 96:
        fam.append(TILE)
    if algo == GJ and n <= 64:
        fam.append(ROW)
    return fam


def gpu_logdet(a, n, algo, kernel=AUTO):
    ta = dev(a)
    batch = a.size // (n * n)
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    sign, ld = api.logdet_batched(ta, n, algo, info=info, kernel=kernel)
    torch.cuda.synchronize()
    assert np.array_equal(ta.cpu().numpy(), a, equal_nan=True), "A was modified"
    return sign.cpu().numpy(), ld.cpu().numpy(), info.cpu().numpy()


def check_logdet(sign, ld, mats, n, u, idx=None, what=""):
    idx = range(len(mats)) if idx is None else idx
    wsign, wld = np.linalg.slogdet(mats)
    for k in idx:
        b = bound(mats[k], wld[k], n, u)
        err = abs(float(ld[k]) - wld[k])
        print(f"  {what} k={k} n={n} err={err:.3e} bound={b:.3e} ratio={err / b:.3f}")
        assert sign[k] == wsign[k], (what, k, sign[k], wsign[k])
        assert err <= b, (what, k, err, b)


SIZES = [1, 2, 5, 8, 16, 17, 24, 32, 33, 48, 63, 64, 65, 80, 96, 97, 100, 128, 200]


@pytest.mark.parametrize("n", SIZES)
def test_accuracy(n):
    batch = 5 if n > 64 else 9
    for dt in DTYPES:
        u = U[np.dtype(dt)]
        spd = spd_batch(n, batch, seed=n, dtype=dt)
        gen = general_batch(n, batch, seed=100 + n, dtype=dt)
        for a, algo, image in ((spd, CH, lower_image), (spd, GJ, full_image), (gen, GJ, full_image)):
            mats = image(a, n)
            for kernel in families(algo, n):
                sign, ld, info = gpu_logdet(a, n, algo, kernel)
                assert not info.any(), (n, dt, algo, kernel, info)
                check_logdet(sign, ld, mats, n, u, what=f"{np.dtype(dt).name} algo={algo} kernel={kernel}")


def test_range_large_determinant_overflows_fp64():
    n = 1024
    a = spd_batch(n, 2, seed=7)
    mats = lower_image(a, n)
    want = np.linalg.slogdet(mats)[1]
    assert (want > 7.0e3).all() and np.isinf(np.linalg.det(mats)).all()  # the determinant itself overflows
    for algo in (CH, GJ):
        sign, ld, info = gpu_logdet(a, n, algo)
        assert not info.any()
        assert np.isfinite(ld).all()
        check_logdet(sign, ld, mats, n, U[np.dtype(np.float64)], what=f"n=1024 algo={algo}")


@pytest.mark.parametrize("dt,s", [(np.float64, 1e-30), (np.float32, 1e-3)])
def test_range_scaled_until_the_determinant_underflows(dt, s):
    n = 64
    u = U[np.dtype(dt)]
    a = spd_batch(n, 6, seed=8, dtype=dt)
    scaled = (a * dt(s)).astype(dt)
    for algo, image in ((CH, lower_image), (GJ, full_image)):
        for kernel in families(algo, n):
            _, base, i0 = gpu_logdet(a, n, algo, kernel)
            sign, ld, info = gpu_logdet(scaled, n, algo, kernel)
            assert not i0.any() and not info.any()
            assert np.isfinite(ld).all()
            mats = image(scaled, n)
            if dt == np.float64:
                assert (np.linalg.det(mats) == 0).all()  # 1e-30^64 underflows
            check_logdet(sign, ld, mats, n, u, what=f"scaled {np.dtype(dt).name} algo={algo} kernel={kernel}")
            # ... and equals the unscaled result plus n log s within the bound (s as rounded to the dtype; cond is unchanged)
            for k in range(6):
                want = float(base[k]) + n * math.log(float(dt(s)))
                b = bound(mats[k], want, n, u)
                assert abs(float(ld[k]) - want) <= b, (k, float(ld[k]), want, b)


@pytest.mark.parametrize("n", [5, 33, 64, 100])
def test_sign(n):
    for dt in DTYPES:
        u = U[np.dtype(dt)]
        m = as_mats(spd_batch(n, 8, seed=11, dtype=dt), n).copy()
        m[1::2, [0, n - 1], :] = m[1::2, [n - 1, 0], :]  # two rows exchanged in every second matrix
        a = np.ascontiguousarray(m.transpose(0, 2, 1)).reshape(-1)
        diag = np.zeros((4, n, n), dtype=dt)
        rng = np.random.default_rng(n)
        for k in range(4):
            d = rng.uniform(0.5, 2.0, n)
            d[rng.choice(n, size=min(2 * k + 1, n if n % 2 else n - 1), replace=False)] *= -1  # an odd number of negative entries
            diag[k] = np.diag(d)
        dflat = np.ascontiguousarray(diag.transpose(0, 2, 1)).reshape(-1)
        for kernel in families(GJ, n):
            sign, ld, info = gpu_logdet(a, n, GJ, kernel)
            assert not info.any()
            assert (sign[0::2] == 1).all() and (sign[1::2] == -1).all()
            check_logdet(sign, ld, full_image(a, n), n, u, what=f"exchange {np.dtype(dt).name} kernel={kernel}")
            sign, ld, info = gpu_logdet(dflat, n, GJ, kernel)
            assert not info.any()
            assert (sign == -1).all()
            check_logdet(sign, ld, full_image(dflat, n), n, u, what=f"diag {np.dtype(dt).name} kernel={kernel}")


@pytest.mark.parametrize("n", [17, 32, 64, 128])
def test_singular_and_not_spd_report_info(n):
    """the cases of test_gpu_solve.test_singular_and_not_spd_report_info: in fp64 info equals the inverse's, outputs NaN exactly there"""
    a = spd_batch(n, 8, seed=3).reshape(8, n, n)
    a[2, 1, :] = 0.0  # column 1 of matrix 2 (memory is [k, col, row])
    a[5] = 0.0
    c = spd_batch(n, 8, seed=4).reshape(8, n, n)
    c[1, n - 1, n - 1] = -1.0
    c[3, 1, :] = 0.0
    c[6] = 0.0
    for algo, m, bad, image in ((GJ, a, [2, 5], full_image), (CH, c, [1, 3, 6], lower_image)):
        ok = [k for k in range(8) if k not in bad]
        for dt in DTYPES:
            flat = m.reshape(-1).astype(dt)
            for kernel in families(algo, n):
                sign, ld, info = gpu_logdet(flat, n, algo, kernel)
                if dt == np.float64:
                    iinfo = torch.full((8,), -7, dtype=torch.int32, device="cuda")
                    api.inverse_batched(dev(flat), n, algo, info=iinfo)
                    torch.cuda.synchronize()
                    assert info.tolist() == iinfo.cpu().tolist(), (algo, kernel, info, iinfo)
                assert all(info[k] != 0 for k in bad), (algo, dt, kernel, info)
                assert not info[ok].any(), (algo, dt, kernel, info)
                assert np.isnan(ld[bad]).all() and np.isnan(sign[bad]).all()
                assert not np.isnan(ld[ok]).any() and not np.isnan(sign[ok]).any()
                check_logdet(sign, ld, image(flat, n), n, U[np.dtype(dt)], idx=ok, what=f"info algo={algo} kernel={kernel}")
                if algo == CH and dt == np.float64:
                    assert info[1] == n  # the negative last diagonal fails at the last pivot
    # logml reports the same not-SPD matrices and leaves NaN exactly there
    for dt in DTYPES:
        flat = c.reshape(-1).astype(dt)
        d = np.random.default_rng(5).standard_normal(8 * n).astype(dt)
        info = torch.full((8,), -7, dtype=torch.int32, device="cuda")
        out = api.logml_batched(n, dev(flat), None, dev(d), info=info)
        torch.cuda.synchronize()
        info, out = info.cpu().numpy(), out.cpu().numpy()
        assert all(info[k] != 0 for k in (1, 3, 6)) and not info[[0, 2, 4, 5, 7]].any(), info
        assert np.isnan(out[[1, 3, 6]]).all() and not np.isnan(out[[0, 2, 4, 5, 7]]).any()


def nan_above_diagonal(a, n):
    dirty = as_mats(a, n).copy()
    iu = np.triu_indices(n, 1)
    dirty[:, iu[0], iu[1]] = np.nan
    return np.ascontiguousarray(dirty.transpose(0, 2, 1)).reshape(-1)


@pytest.mark.parametrize("n", [8, 32, 50, 64, 96, 100])
def test_reads_lower_triangle_only(n):
    for dt in DTYPES:
        a = spd_batch(n, 6, seed=21, dtype=dt)
        dirty = nan_above_diagonal(a, n)
        for kernel in families(CH, n):
            s0, l0, i0 = gpu_logdet(a, n, CH, kernel)
            s1, l1, i1 = gpu_logdet(dirty, n, CH, kernel)
            assert not i0.any() and not i1.any()
            assert np.array_equal(l0, l1) and np.array_equal(s0, s1) and (s0 == 1).all()
        rng = np.random.default_rng(22)
        c, d = rng.random(6 * n).astype(dt), rng.standard_normal(6 * n).astype(dt)
        clean = api.logml_batched(n, dev(a), dev(c), dev(d)).cpu().numpy()
        got = api.logml_batched(n, dev(dirty), dev(c), dev(d)).cpu().numpy()
        assert np.isfinite(clean).all() and np.array_equal(clean, got)


@pytest.mark.parametrize("n,algo,kernel", [(32, CH, AUTO), (64, CH, AUTO), (40, GJ, AUTO), (12, GJ, AUTO), (100, CH, AUTO), (100, GJ, AUTO),
                                           (48, CH, GLOBAL)])
def test_padded_strides_and_purity(n, algo, kernel):
    batch, extra = 7, 4
    sa = n * n + 13
    for dt in DTYPES:
        base = spd_batch(n, batch, seed=31, dtype=dt)
        A = np.full(batch * sa, np.nan, dtype=dt)
        for k in range(batch):
            A[k * sa:k * sa + n * n] = base[k * n * n:(k + 1) * n * n]
        ta = dev(A)
        sign = torch.full((batch + extra,), 123.0, dtype=ta.dtype, device="cuda")
        out = torch.full((batch + extra,), 321.0, dtype=ta.dtype, device="cuda")
        info = torch.full((batch + extra,), -7, dtype=torch.int32, device="cuda")
        s, o = api.logdet_batched(ta, n, algo, sign=sign, out=out, info=info, kernel=kernel, batch=batch, stride=sa)
        torch.cuda.synchronize()
        assert s is sign and o is out
        assert np.array_equal(ta.cpu().numpy(), A, equal_nan=True), "A was modified"
        assert (sign[batch:] == 123.0).all() and (out[batch:] == 321.0).all() and (info[batch:] == -7).all()
        assert not info[:batch].any()
        image = lower_image if algo == CH else full_image
        check_logdet(sign[:batch].cpu().numpy(), out[:batch].cpu().numpy(), image(base, n), n, U[np.dtype(dt)], what="strided")
        # the packed call gives the same bits; a NULL sign is accepted at the C level
        s2, o2, _ = gpu_logdet(base, n, algo, kernel)
        assert np.array_equal(o2, out[:batch].cpu().numpy()) and np.array_equal(s2, sign[:batch].cpu().numpy())
        lib = pkg("_lib")
        o3 = torch.full((batch,), 5.0, dtype=ta.dtype, device="cuda")
        lib.check(lib.lib().matinv_logdet_batched_ex(algo, api.F64 if dt == np.float64 else api.F32, n, ctypes.c_void_p(ta.data_ptr()), sa,
                                                     ctypes.c_void_p(o3.data_ptr()), None, batch, None,
                                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), kernel))
        torch.cuda.synchronize()
        assert np.array_equal(o3.cpu().numpy(), o2)
    # logml: inputs bitwise unchanged, elements of the output beyond the batch untouched
    rng = np.random.default_rng(33)
    B = spd_batch(n, batch, seed=32)
    c, d = rng.random(batch * n), rng.standard_normal(batch * n)
    tb, tc, td = dev(B), dev(c), dev(d)
    out = torch.full((batch + extra,), 321.0, dtype=torch.float64, device="cuda")
    api.logml_batched(n, tb, tc, td, out=out, batchSize=batch)
    torch.cuda.synchronize()
    assert np.array_equal(tb.cpu().numpy(), B) and np.array_equal(tc.cpu().numpy(), c) and np.array_equal(td.cpu().numpy(), d)
    assert (out[batch:] == 321.0).all() and torch.isfinite(out[:batch]).all()


@pytest.mark.parametrize("n", [20, 48, 64, 100])
def test_per_matrix_determinism(n):
    """the result for matrix k depends on matrix k alone: a mixed SPD / general batch, whole and as three subsets, gives the same bits"""
    dom = spd_batch(n, 12, seed=41).reshape(12, n * n)
    gen = general_batch(n, 12, seed=42).reshape(12, n * n)
    a = np.empty((24, n * n))
    a[0::2], a[1::2] = dom, gen
    for dt in DTYPES:
        aa = a.astype(dt)
        for algo, rows in ((GJ, aa), (CH, aa[0::2])):
            sign, ld, info = gpu_logdet(rows.reshape(-1), n, algo)
            assert not info.any()
            for sel in (slice(0, None, 2), slice(1, None, 2), [3, 4, 11]):
                s, l, _ = gpu_logdet(rows[sel].reshape(-1), n, algo)
                assert np.array_equal(l, ld[sel]) and np.array_equal(s, sign[sel])
        rng = np.random.default_rng(44)
        B = aa[0::2]
        c, d = rng.random((12, n)).astype(dt), rng.standard_normal((12, n)).astype(dt)
        whole = api.logml_batched(n, dev(B.reshape(-1)), dev(c.reshape(-1)), dev(d.reshape(-1))).cpu().numpy()
        for sel in (slice(0, None, 2), slice(1, None, 2), [3, 4, 11]):
            part = api.logml_batched(n, dev(B[sel].reshape(-1)), dev(c[sel].reshape(-1)), dev(d[sel].reshape(-1))).cpu().numpy()
            assert np.array_equal(part, whole[sel])


@pytest.mark.parametrize("n", [32, 64])
def test_families_agree(n):
    for dt in DTYPES:
        u = U[np.dtype(dt)]
        a = spd_batch(n, 16, seed=51, dtype=dt)
        g = general_batch(n, 16, seed=52, dtype=dt)
        assert api.logdet_kernel_name(CH, dt, n).startswith("matinv_logdet_tile_")
        assert api.logdet_kernel_name(GJ, dt, n).startswith("matinv_logdet_row<")
        for m, algo, fast, image in ((a, CH, TILE, lower_image), (a, GJ, ROW, full_image), (g, GJ, ROW, full_image)):
            s1, l1, i1 = gpu_logdet(m, n, algo, fast)
            s2, l2, i2 = gpu_logdet(m, n, algo, GLOBAL)
            assert not i1.any() and not i2.any() and np.array_equal(s1, s2)
            mats = image(m, n)
            check_logdet(s1, l1, mats, n, u, what="fast")
            check_logdet(s2, l2, mats, n, u, what="global")
            for k in range(16):
                b = bound(mats[k], float(l2[k]), n, u)
                assert abs(float(l1[k]) - float(l2[k])) <= 2 * b


def logml_reference(B, c, d, n):
    """(want, q, logdet, M) in float64 from the lower triangle of B"""
    M = lower_image(B, n)
    if c is not None:
        M = M + np.stack([np.diag(v) for v in np.asarray(c, dtype=np.float64).reshape(-1, n)])
    dd = np.asarray(d, dtype=np.float64).reshape(-1, n)
    q = np.einsum("ki,ki->k", dd, np.linalg.solve(M, dd[:, :, None])[:, :, 0])
    sign, ld = np.linalg.slogdet(M)
    assert (sign == 1).all()
    return -0.5 * q - 0.5 * ld - 0.5 * n * math.log(2 * math.pi), q, ld, M


def q_tol(q, cond, n, f64):
    return 0.5 * abs(q) * (max(1e-10, 1e-15 * cond * n) if f64 else 1e-5 * cond)


def check_logml(got, B, c, d, n, dt, what=""):
    want, q, ld, M = logml_reference(B, c, d, n)
    u, f64 = U[np.dtype(dt)], np.dtype(dt) == np.float64
    for k in range(len(want)):
        cond = np.linalg.cond(M[k])
        tol = 0.5 * (n * n * u * cond + n * u * max(1.0, abs(ld[k]))) + q_tol(q[k], cond, n, f64)
        err = abs(float(got[k]) - want[k])
        print(f"  logml {what} k={k} n={n} err={err:.3e} tol={tol:.3e}")
        assert err <= tol, (what, k, err, tol)


@pytest.mark.parametrize("d,n", [("gaussian_100_8x8", 8), ("gaussian_100_16x16", 16), ("gaussian_32_32x32", 32),
                                 ("gaussian_12_64x64", 64)])
def test_logml_reference_fixtures(d, n):
    for dt in DTYPES:
        r = {f: read_ref(f"{d}/{f}.mats", dtype=dt)[0] for f in ("b", "c", "d")}
        info = torch.full((r["b"].size // (n * n),), -7, dtype=torch.int32, device="cuda")
        got = api.logml_batched(n, dev(r["b"]), dev(r["c"]), dev(r["d"]), info=info)
        torch.cuda.synchronize()
        assert not info.cpu().numpy().any()
        check_logml(got.cpu().numpy(), r["b"], r["c"], r["d"], n, dt, what=d)


@pytest.mark.parametrize("n", [5, 16, 17, 40, 64, 80, 96, 97, 128, 200])
def test_logml_synthetic(n):
    batch = 7
    for dt in DTYPES:
        rng = np.random.default_rng(n)
        B = spd_batch(n, batch, seed=n, dtype=dt)
        c = rng.uniform(0.1, 2.0, batch * n).astype(dt)
        d = rng.standard_normal(batch * n).astype(dt)
        for cc in (c, None):
            info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
            got = api.logml_batched(n, dev(B), dev(cc) if cc is not None else None, dev(d), info=info)
            torch.cuda.synchronize()
            assert not info.cpu().numpy().any()
            got = got.cpu().numpy()
            check_logml(got, B, cc, d, n, dt, what=f"{np.dtype(dt).name} c={'yes' if cc is not None else 'no'}")
            # consistency inside the library: logml + logabsdet(CHOLESKY, M)/2 + n/2 log(2 pi) = variance(a = d, e = 0)/2
            Mflat = B.copy()
            if cc is not None:
                Mflat.reshape(batch, n * n)[:, ::n + 1] += cc.reshape(batch, n)
            _, ld, i2 = gpu_logdet(Mflat, n, CH)
            assert not i2.any()
            zc = cc if cc is not None else np.zeros(batch * n, dtype=dt)
            var = api.variance_batched(n, dev(d), dev(B), dev(zc), dev(np.zeros(batch, dtype=dt))).cpu().numpy()
            _, q, wld, M = logml_reference(B, cc, d, n)
            u, f64 = U[np.dtype(dt)], dt == np.float64
            for k in range(batch):
                cond = np.linalg.cond(M[k])
                tol = (n * n * u * cond + n * u * max(1.0, abs(wld[k]))) + 2 * q_tol(q[k], cond, n, f64)
                lhs = float(got[k]) + 0.5 * float(ld[k]) + 0.5 * n * math.log(2 * math.pi)
                assert abs(lhs - 0.5 * float(var[k])) <= tol, (k, lhs, 0.5 * float(var[k]), tol)


def test_offsets_beyond_2_pow_32_elements():
    """1.1 M x 64^2 fp32 = 4.5e9 elements: matrix offsets past 2^32, six matrices spot-checked against numpy"""
    n, batch = 64, 1_100_000
    free, _ = torch.cuda.mem_get_info()
    need = batch * n * n * 4 + 4 * batch * 4
    assert free > need + (4 << 30), f"needs {need >> 30} GiB of device memory"
    g = torch.Generator(device="cuda").manual_seed(5)
    a = torch.rand(batch * n * n, dtype=torch.float32, device="cuda", generator=g)
    a.view(batch, n * n)[:, :: n + 1] += float(n)  # dominant diagonal
    u = U[np.dtype(np.float32)]
    first_high = (1 << 32) // (n * n)
    for algo, image in ((CH, lower_image), (GJ, full_image)):
        info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
        sign, ld = api.logdet_batched(a, n, algo, info=info)
        torch.cuda.synchronize()
        assert int(info.abs().sum()) == 0
        for k in (0, 12345, first_high - 1, first_high, first_high + 1, batch - 1):
            ak = a[k * n * n:(k + 1) * n * n].cpu().numpy()
            check_logdet(sign[k:k + 1].cpu().numpy(), ld[k:k + 1].cpu().numpy(), image(ak, n), n, u, what=f"offset k={k} algo={algo}")
        del sign, ld, info
    del a


def test_host_form_equals_device_form():
    n = 40
    for dt in DTYPES:
        a = spd_batch(n, 11, seed=61, dtype=dt)
        for algo, image in ((GJ, full_image), (CH, lower_image)):
            sign, ld, info = api.logdet_batched_host(a, n, algo)
            assert not info.any()
            check_logdet(sign, ld, image(a, n), n, U[np.dtype(dt)], what="host")
            s, l, _ = gpu_logdet(a, n, algo)
            assert np.array_equal(ld, l) and np.array_equal(sign, s)
        rng = np.random.default_rng(62)
        c, d = rng.random(11 * n).astype(dt), rng.standard_normal(11 * n).astype(dt)
        for cc in (c, None):
            out, info = api.logml_batched_host(n, a, cc, d)
            assert not info.any()
            check_logml(out, a, cc, d, n, dt, what="host")
            od = api.logml_batched(n, dev(a), dev(cc) if cc is not None else None, dev(d)).cpu().numpy()
            assert np.array_equal(out, od)
