"""Every kernel instantiation a request can reach, run at the first and the last size it serves (tests/_instantiations.py makes the
list from the library's own route names; tests/test_instantiations_cpu.py checks it against the compiled kernels).

Shape of a case: batch 13 up to n = 64, 5 up to 256, 2 beyond; blocks at a stride of width + 3 elements inside a larger allocation whose
gaps hold NaN (inputs) or a sentinel (outputs) -- tests/_instantiation_runner.py. Every case asserts that no input changed, that no
output gap was written, and that no NaN reached a healthy result.

References and tolerances are the ones of the hand-written tests:
  inverse fp64 : CPU oracle, max |x-y| / max(|y|, 1e-3 max|Y|) < max(1e-10, 1e-15 cond n)            (test_gpu_parity.py)
  inverse fp32 : fp64 oracle on the fp32-rounded input, ||X-Y||_F / ||Y||_F < 1e-5 cond per matrix      (test_fp32_vs_fp64_oracle)
  solve        : check_close of test_gpu_solve.py;  logdet, logml: check_logdet / check_logml of test_gpu_logdet.py
  mean, variance : oracle on the float64 inputs, 1e-10 / 2e-5 absolute                                  (test_pipeline_synthetic)
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from conftest import ROOT, pkg, rel_err

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import _instantiations as inst  # noqa: E402
from _instantiation_runner import (LEAD, Blocks, bits, info_buffer, read_info, run_inverse, run_screened_cases,  # noqa: E402
                                   screened_cases)
from test_gpu_logdet import U, check_logdet, check_logml, full_image, lower_image  # noqa: E402
from test_gpu_solve import check_close  # noqa: E402

api = inst.api
lib = pkg("_lib")
GJ, CH = inst.GJ, inst.CH
CASES = inst.cases()


def of(entry, algo=None):
    return [c for c in CASES if c.route.entry == entry and (algo is None or c.route.algo == algo)]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def f64_of(case):
    return case.route.dtype == "f64"


def resolved_family(case):
    r = case.route
    k = inst.FAMILIES[r.family]
    return api.select_kernel(inst.ALGOS[r.algo], inst.DTYPES[r.dtype], case.n) if k == api.KERNEL_AUTO else k


def check_inverse(got, want, n, f64, cond, what):
    """got, want: (k, n*n) healthy matrices"""
    assert np.isfinite(got).all(), f"{what}: NaN or Inf in a healthy result"
    if f64:
        err, tol = rel_err(got, want, n), max(1e-10, 1e-15 * cond * n)
    else:
        g, w = got.astype(np.float64), want
        err, tol = (np.linalg.norm(g - w, axis=1) / np.linalg.norm(w, axis=1)).max(), 1e-5 * cond
    print(f"  {what}: err={err:.3e} tol={tol:.3e} cond={cond:.3e}")
    assert err < tol, (what, err, tol)


# ---- references: once per (n, dtype, kind), shared by every case of that size ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gj_reference(n, dtype, mixed):
    a, ok = inst.gj_batch(n, dtype, mixed)
    want, winfo = oracle.inverse_batched(a.astype(np.float64).reshape(-1), n, oracle.ALGO_GJ_PIVOT)
    assert np.array_equal(np.flatnonzero(winfo == 0), ok), "the oracle disagrees about which matrices are healthy"
    return want.reshape(len(a), n * n), winfo


@functools.lru_cache(maxsize=None)
def chol_reference(n, dtype):
    clean, _, ok = inst.chol_batch(n, dtype)
    want, winfo = oracle.inverse_batched(clean.astype(np.float64).reshape(-1), n, oracle.ALGO_CHOLESKY)
    assert winfo.tolist() == [0] * len(ok) + [n // 3 + 1]
    return want.reshape(len(clean), n * n), winfo


@functools.lru_cache(maxsize=None)
def pipeline_reference(n):
    a, B, c, d, e = inst.pipeline_batch(n)
    return oracle.mean_batched(a, B, c, d, n), oracle.variance_batched(a, B, c, e, n)


# ---- inverse ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", of("inverse", "gj"), ids=inst.case_id)
def test_gauss_jordan_inverse(case):
    r, n = case.route, case.n
    family = resolved_family(case)
    # AUTO / TILE / ROWLANE: natural-order kernels with a pivoting second pass -> the mixed batch; the pivoting families: a general one
    mixed = family in (api.KERNEL_TILE, api.KERNEL_ROWLANE)
    a, ok = inst.gj_batch(n, r.dtype, mixed)
    want, winfo = gj_reference(n, r.dtype, mixed)
    got, info = run_inverse(a, n, GJ, inst.FAMILIES[r.family])
    bad = winfo != 0
    assert np.array_equal(info != 0, bad), (info, winfo)
    if family == api.KERNEL_TILE and 17 <= n <= 32:  # where test_natural_pass_two_rows_per_lane compares the values
        assert np.array_equal(info[bad], winfo[bad]), (info, winfo)
    assert np.isnan(got[bad]).all(), "a flagged result is not all NaN"
    check_inverse(got[ok], want[ok], n, f64_of(case), inst.max_cond("gj", n, r.dtype, mixed), inst.case_id(case))


@pytest.mark.parametrize("case", of("inverse", "chol"), ids=inst.case_id)
def test_cholesky_inverse(case):
    r, n = case.route, case.n
    _, dirty, ok = inst.chol_batch(n, r.dtype)
    want, winfo = chol_reference(n, r.dtype)
    got, info = run_inverse(dirty, n, CH, inst.FAMILIES[r.family])
    assert info.tolist() == winfo.tolist()
    assert np.isnan(got[winfo != 0]).all(), "a flagged result is not all NaN"
    check_inverse(got[ok], want[ok], n, f64_of(case), inst.max_cond("chol", n, r.dtype), inst.case_id(case))


def refusals():
    out = []
    for r in inst.routes():
        out += [(r, n) for n in inst.refused(r)]
    return out


@pytest.mark.parametrize("route,n", refusals(), ids=lambda v: "-".join(x for x in map(str, v) if x) if isinstance(v, tuple) else str(v))
def test_forced_family_refuses_the_size_after_its_last(route, n):
    """the name is "" there (test_instantiations_cpu.py) and the call is refused: an argument check, nothing is launched"""
    assert inst.route_name(route, n) == ""
    t = torch.zeros(n * n + 3, dtype=torch.float64 if route.dtype == "f64" else torch.float32, device="cuda")
    algo, kernel = inst.ALGOS[route.algo], inst.FAMILIES[route.family]
    with pytest.raises(lib.MatinvError) as e:
        if route.entry == "inverse":
            api.inverse_batched(t, n, algo, out=torch.empty_like(t), kernel=kernel, batch=1)
        elif route.entry == "solve":
            api.solve_batched(t, t[: n * route.nrhs], n, route.nrhs, algo, out=torch.empty_like(t), kernel=kernel, batch=1)
        else:
            assert route.entry == "logdet"
            api.logdet_batched(t, n, algo, kernel=kernel, batch=1)
    assert e.value.code == lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()


# ---- solve --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", of("solve"), ids=inst.case_id)
def test_solve(case):
    r, n, nrhs = case.route, case.n, case.route.nrhs
    clean, a = inst.solve_batch(n, r.dtype, r.algo)
    b = inst.rhs_batch(n, nrhs, r.dtype)
    la, lb = Blocks(len(a), n * n, n), Blocks(len(a), n * nrhs, n)
    ha, hb = la.host_input(a), lb.host_input(b)
    da, db = dev(ha), dev(hb)
    dx = lb.device_output(da.dtype)
    info = info_buffer(la.batch)
    with inst.gj_policy(api.GJ_PIVOT if r.family == "pivot" else None):
        assert api.solve_kernel_name(inst.ALGOS[r.algo], inst.DTYPES[r.dtype], n, nrhs, inst.FAMILIES.get(r.family, api.KERNEL_AUTO)) == case.name
        api.solve_batched(da[LEAD:], db[LEAD:], n, nrhs, inst.ALGOS[r.algo], info=info, out=dx[LEAD:],
                          kernel=inst.FAMILIES.get(r.family, api.KERNEL_AUTO), batch=la.batch, strideA=la.stride, strideB=lb.stride,
                          strideX=lb.stride)
        torch.cuda.synchronize()
    la.check_input_unchanged(da, ha, "A")
    lb.check_input_unchanged(db, hb, "B")
    x = lb.read_output(dx, "solve")
    assert not read_info(info, la.batch).any()
    assert np.isfinite(x).all()
    check_close(x.reshape(-1), clean.reshape(-1), b.reshape(-1), n, nrhs, f64_of(case))


# ---- logdet -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", of("logdet"), ids=inst.case_id)
def test_logdet(case):
    """general matrices (both signs) through Gauss-Jordan, SPD ones with garbage above the diagonal through Cholesky; one item of
    every batch of 5 or more is singular / not positive definite: info as the inverse reports it, both outputs NaN"""
    r, n = case.route, case.n
    if r.algo == "gj":
        a, ok = inst.gj_batch(n, r.dtype, False)
        mats, winfo = full_image(a.reshape(-1), n), gj_reference(n, r.dtype, False)[1]
    else:
        clean, a, ok = inst.chol_batch(n, r.dtype)
        mats, winfo = lower_image(clean.reshape(-1), n), chol_reference(n, r.dtype)[1]
    lay = Blocks(len(a), n * n, n)
    ha = lay.host_input(a)
    da = dev(ha)
    sign, ld = (torch.full((lay.batch + 3,), -5.0, dtype=da.dtype, device="cuda") for _ in range(2))
    info = info_buffer(lay.batch)
    api.logdet_batched(da[LEAD:], n, inst.ALGOS[r.algo], sign=sign, out=ld, info=info, kernel=inst.FAMILIES[r.family],
                       batch=lay.batch, stride=lay.stride)
    torch.cuda.synchronize()
    lay.check_input_unchanged(da, ha, "A")
    sign, ld, info = sign.cpu().numpy(), ld.cpu().numpy(), read_info(info, lay.batch)
    assert (sign[lay.batch:] == -5.0).all() and (ld[lay.batch:] == -5.0).all(), "outputs were written beyond the batch"
    bad = winfo != 0
    assert np.array_equal(info != 0, bad), (info, winfo)
    if r.algo == "chol":
        assert info.tolist() == winfo.tolist()
    assert np.isnan(ld[:lay.batch][bad]).all() and np.isnan(sign[:lay.batch][bad]).all()
    assert np.isfinite(ld[ok]).all()
    check_logdet(sign, ld, mats, n, U[np.dtype(inst.NP_DTYPES[r.dtype])], idx=ok, what=inst.case_id(case))


# ---- fused pipeline, logml: packed batches (these entry points take no stride), NaN behind every input, sentinel behind the output ----
def padded(x, n):
    return dev(np.concatenate([x, np.full((n + 16) ** 2, np.nan, dtype=x.dtype)]))


@pytest.mark.parametrize("case", of("mean") + of("variance"), ids=inst.case_id)
def test_mean_variance(case):
    r, n = case.route, case.n
    dt = inst.NP_DTYPES[r.dtype]
    variance = r.entry == "variance"
    assert api.gp_kernel_name(inst.DTYPES[r.dtype], n, variance) == case.name
    host = [x.astype(dt) for x in inst.pipeline_batch(n)]
    a, B, c, d, e = (padded(x, n) for x in host)
    batch = inst.batch_of(n)
    out = torch.full((batch + 3,), -5.0, dtype=B.dtype, device="cuda")
    info = info_buffer(batch)
    if variance:
        api.calcluateVariance(n, a, B, c, e, Variances=out, batchSize=batch, info=info)
    else:
        api.calcluateMean(n, a, B, c, d, Means=out, batchSize=batch, info=info)
    torch.cuda.synchronize()
    for t, h in zip((a, B, c, d, e), host):
        assert np.array_equal(bits(t.cpu().numpy()[: h.size]), bits(h)) and torch.isnan(t[h.size:]).all(), "an input was modified"
    got = out.cpu().numpy()
    assert (got[batch:] == -5.0).all(), "the output was written beyond the batch"
    assert not read_info(info, batch).any()
    want = pipeline_reference(n)[1 if variance else 0]
    err, tol = np.abs(got[:batch].astype(np.float64) - want).max(), 1e-10 if f64_of(case) else 2e-5
    print(f"  {inst.case_id(case)}: err={err:.3e} tol={tol:.1e}")
    assert err < tol


@pytest.mark.parametrize("case", of("logml"), ids=inst.case_id)
def test_logml(case):
    r, n = case.route, case.n
    dt = inst.NP_DTYPES[r.dtype]
    assert api.logml_kernel_name(inst.DTYPES[r.dtype], n) == case.name
    clean, dirty, _ = inst.chol_batch(n, r.dtype, False)  # only the lower triangle may be read
    _, _, c, d, _ = (x.astype(dt) for x in inst.pipeline_batch(n))
    batch = inst.batch_of(n)
    tB, tc, td = padded(dirty.reshape(-1), n), padded(c, n), padded(d, n)
    out = torch.full((batch + 3,), -5.0, dtype=tB.dtype, device="cuda")
    info = info_buffer(batch)
    api.logml_batched(n, tB, tc, td, out=out, batchSize=batch, info=info)
    torch.cuda.synchronize()
    for t, h in ((tB, dirty.reshape(-1)), (tc, c), (td, d)):
        assert np.array_equal(bits(t.cpu().numpy()[: h.size]), bits(h)), "an input was modified"
    got = out.cpu().numpy()
    assert (got[batch:] == -5.0).all(), "the output was written beyond the batch"
    assert not read_info(info, batch).any()
    check_logml(got[:batch], clean.reshape(-1), c, d, n, dt, what=inst.case_id(case))


# ---- kernels no route names -----------------------------------------------------------------------------------------------------
def test_screened_launches_give_the_same_bits(tmp_path):
    """MATINV_TILE_SCREEN=1 puts the screening kernel (and, for 3 and 4 tiles, the early-exit form of the natural-order kernel) in front
    of every natural-order launch of the tile family. It may change what a launch costs, never a bit of what it computes: the Gauss-Jordan
    TILE cases above (compared with the oracle there) are run again in one fresh process with the switch set."""
    path = str(tmp_path / "screened.npz")
    env = dict(os.environ, MATINV_TILE_SCREEN="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_instantiation_runner.py"), path], capture_output=True, text=True,
                       env=env, timeout=300)
    assert p.returncode == 0 and "screen-worker ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    screened = np.load(path)
    here = run_screened_cases()
    assert sorted(screened.files) == sorted(here) and len(here) == 2 * len(screened_cases())
    for i, c in enumerate(screened_cases()):
        assert np.array_equal(screened[f"{i}i"], here[f"{i}i"]), (inst.case_id(c), "info")
        assert np.array_equal(screened[str(i)], here[str(i)]), (inst.case_id(c), "result bits")

