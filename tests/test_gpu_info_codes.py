"""The VALUE of info on every kernel route: include/matinv.h promises the 1-based column of the first non-positive leading minor
(Cholesky contract) or of the elimination step without a usable pivot (Gauss-Jordan contract), not merely "non-zero".

Cases: the audited list of tests/_instantiations.py (every kernel name of every route at the first and the last size it serves) for
inverse, solve, logdet, mean, variance and logml; leave-one-out and the gradients grouped here the same way from the library's
matinv_loo_kernel_name / matinv_logml_grad_kernel_name. Inputs: tests/_info_cases.py (checked against the CPU oracle by
tests/test_info_cases_cpu.py) -- C1, C2, C3 on the Cholesky-contract routes, G1, G2 on the Gauss-Jordan ones; the routes that take
M = B + diag c get the edit in B.

Per batch: info equals the expected vector exactly (G2: one of the two zero columns), every output of a flagged matrix is NaN, the
three healthy matrices report 0, are finite and are bit-identical to a second call on those three alone (matinv.h: the result
"depends on matrix k alone"); no input changes, nothing is written past the batch. The accuracy of the healthy results is pinned by
test_gpu_instantiations.py.

The fp32 one-wave-per-tile-column SPD sweep (SAME_TILE_KERNELS below: Cholesky inverse and the solve composed from it, 160 < n <= 256)
eliminates the columns of a 16-column tile in a permuted order and reports the first failure in that order; for it matinv.h promises
the 16-column tile of the first non-positive leading minor, and C2 / C3 assert exactly that: the same tile, and never past n. C1 is
exact everywhere.
"""
import functools
import re

import numpy as np
import pytest

import _info_cases as ic
from conftest import pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import _instantiations as inst  # noqa: E402
from _instantiation_runner import LEAD, Blocks, bits, info_buffer, read_info, run_inverse  # noqa: E402

api = inst.api
SENTINEL = -5.0
LOCAL_ENTRIES = {"loo": api.loo_kernel_name, "grad": api.logml_grad_kernel_name}


def local_cases():
    """leave-one-out and gradients: the first and the last n of each run of a kernel name, as _instantiations.cases() does it"""
    out = []
    for entry, name_of in LOCAL_ENTRIES.items():
        for dt in inst.DTYPES:
            r = inst.Route(entry, "", dt, "", 0)
            table = {}
            for n in inst.sizes():
                name = name_of(inst.DTYPES[dt], n)
                if name:
                    table.setdefault(name, []).append(n)
            for name, ns in sorted(table.items()):
                picked = set()
                for first, last in inst.runs(ns):
                    picked.update((first, last))
                out += [inst.Case(r, name, n) for n in sorted(picked)]
    return out


def name_of(case):
    r = case.route
    if r.entry in LOCAL_ENTRIES:
        return LOCAL_ENTRIES[r.entry](inst.DTYPES[r.dtype], case.n)
    return inst.route_name(r, case.n)


ENTRIES = ("inverse", "solve", "logdet", "mean", "variance", "logml")
# sorted by size: the batches of one size are built once and shared by the cases of that size that follow each other
CASES = sorted([c for c in inst.cases() if c.route.entry in ENTRIES] + local_cases(), key=lambda c: (c.n, inst.case_id(c)))


def gauss_jordan(case):
    return case.route.algo == "gj"


# The fp32 one-wave-per-tile-column SPD sweep (160 < n <= 256) writes info itself from the permuted elimination order of its 16-column
# tiles (PanelSolve::binfo with TileGeo<float>::pcol); the other fp32 tile kernels that report for themselves resolve the column in
# natural order on their error path (spd_natural_first_failure, tile_common.hpp)
SAME_TILE_KERNELS = (r"matinv_gj_tile4_f32<(\d+), false, \1, true>",)


def same_tile_only(case):
    """routes on which C2 / C3 are promised (matinv.h) and asserted to name the right 16-column tile only: see the module docstring"""
    return case.route.dtype == "f32" and not gauss_jordan(case) and any(re.fullmatch(p, case.name) for p in SAME_TILE_KERNELS)


@functools.lru_cache(maxsize=5)
def batch_of(family, n):
    b = ic.build(family, n)
    b.a.setflags(write=False)
    return b


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def padded(x, n):
    """a packed input with NaN behind it: a kernel that reads past the batch computes NaN and stays inside the allocation"""
    x = np.ascontiguousarray(x).reshape(-1)
    return dev(np.concatenate([x, np.full((n + 16) ** 2, np.nan, dtype=x.dtype)]))


def unchanged(t, h):
    h = np.ascontiguousarray(h).reshape(-1)
    return np.array_equal(bits(t.cpu().numpy()[: h.size]), bits(h))


def out_buffer(count, dtype):
    return torch.full((count + 3,), SENTINEL, dtype=dtype, device="cuda")


def read_out(t, count, width, what):
    h = t.cpu().numpy()
    assert (h[count:] == SENTINEL).all(), f"{what} was written beyond the batch"
    return h[:count].reshape(-1, width).copy()


# ---- inputs of a case: a dict of arrays with the batch as leading dimension, so that a subset of the matrices is a plain index ----------
def inputs_of(case, mats):
    r, n = case.route, case.n
    dt = inst.NP_DTYPES[r.dtype]
    batch = len(mats)
    rng = np.random.default_rng(31 * n + batch)
    if r.entry in ("inverse", "logdet"):
        return {"A": mats.reshape(batch, n * n).astype(dt)}
    if r.entry == "solve":
        return {"A": mats.reshape(batch, n * n).astype(dt), "B": rng.standard_normal((batch, n * r.nrhs)).astype(dt)}
    B, c = ic.split_diagonal(mats, dt, seed=n)
    x = {"B": B.reshape(batch, n * n), "c": c, "d": rng.random((batch, n)).astype(dt)}
    if r.entry in ("mean", "variance"):
        x["a"] = rng.random((batch, n)).astype(dt)
        x["e"] = rng.random((batch, 1)).astype(dt)
    return x


def subset(x, idx):
    return {k: np.ascontiguousarray(v[list(idx)]) for k, v in x.items()}


def launch(case, x):
    """runs the route on the inputs x; returns ({output name: (batch, width) array}, info) after checking that no input changed and
    that nothing was written outside the outputs"""
    r, n = case.route, case.n
    batch = len(next(iter(x.values())))
    algo = inst.ALGOS.get(r.algo)
    kernel = inst.FAMILIES.get(r.family, api.KERNEL_AUTO)
    if r.entry == "inverse":
        got, info = run_inverse(x["A"], n, algo, kernel)
        return {"inverse": got}, info
    info = info_buffer(batch)
    if r.entry == "solve":
        la, lb = Blocks(batch, n * n, n), Blocks(batch, n * r.nrhs, n)
        ha, hb = la.host_input(x["A"]), lb.host_input(x["B"])
        da, db = dev(ha), dev(hb)
        dx = lb.device_output(da.dtype)
        with inst.gj_policy(api.GJ_PIVOT if r.family == "pivot" else None):
            api.solve_batched(da[LEAD:], db[LEAD:], n, r.nrhs, algo, info=info, out=dx[LEAD:], kernel=kernel, batch=batch,
                              strideA=la.stride, strideB=lb.stride, strideX=lb.stride)
            torch.cuda.synchronize()
        la.check_input_unchanged(da, ha, "A")
        lb.check_input_unchanged(db, hb, "B")
        return {"X": lb.read_output(dx, "solve")}, read_info(info, batch)
    if r.entry == "logdet":
        lay = Blocks(batch, n * n, n)
        ha = lay.host_input(x["A"])
        da = dev(ha)
        sign, ld = out_buffer(batch, da.dtype), out_buffer(batch, da.dtype)
        api.logdet_batched(da[LEAD:], n, algo, sign=sign, out=ld, info=info, kernel=kernel, batch=batch, stride=lay.stride)
        torch.cuda.synchronize()
        lay.check_input_unchanged(da, ha, "A")
        return {"logabsdet": read_out(ld, batch, 1, "logabsdet"), "sign": read_out(sign, batch, 1, "sign")}, read_info(info, batch)
    t = {k: padded(v, n) for k, v in x.items()}
    dtype = t["B"].dtype
    if r.entry in ("mean", "variance"):
        o = out_buffer(batch, dtype)
        if r.entry == "variance":
            api.calcluateVariance(n, t["a"], t["B"], t["c"], t["e"], Variances=o, batchSize=batch, info=info)
        else:
            api.calcluateMean(n, t["a"], t["B"], t["c"], t["d"], Means=o, batchSize=batch, info=info)
        outs = {r.entry: (o, 1)}
    elif r.entry == "logml":
        o = out_buffer(batch, dtype)
        api.logml_batched(n, t["B"], t["c"], t["d"], out=o, batchSize=batch, info=info)
        outs = {"logml": (o, 1)}
    elif r.entry == "loo":
        mean, var, logpl = out_buffer(batch * n, dtype), out_buffer(batch * n, dtype), out_buffer(batch, dtype)
        api.loo_batched(n, t["B"], t["c"], t["d"], mean=mean, var=var, logpl=logpl, batchSize=batch, info=info)
        outs = {"mean": (mean, n), "var": (var, n), "logpl": (logpl, 1)}
    else:
        assert r.entry == "grad"
        grad, gradc, alpha = out_buffer(batch, dtype), out_buffer(batch * n, dtype), out_buffer(batch * n, dtype)
        # one derivative matrix per item: B itself (inputs may alias each other; its NaN tail is not part of it)
        api.logml_grad_batched(n, t["B"], t["c"], t["d"], t["B"][: batch * n * n], grad=grad, gradc=gradc, alpha=alpha, batchSize=batch,
                               info=info)
        outs = {"grad": (grad, 1), "gradc": (gradc, n), "alpha": (alpha, n)}
    torch.cuda.synchronize()
    for k, v in x.items():
        assert unchanged(t[k], v) and torch.isnan(t[k][v.size:]).all(), f"input {k} was modified"
    return {k: read_out(o, batch * w, w, k) for k, (o, w) in outs.items()}, read_info(info, batch)


def mismatches(info, want):
    return [(int(k), int(info[k]), int(want[k])) for k in np.flatnonzero(info != want)[:10]]


def check_family(case, family):
    n = case.n
    b = batch_of(family, n)
    x = inputs_of(case, b.a)
    out, info = launch(case, x)
    what = f"{inst.case_id(case)} {family}"
    healthy = list(b.healthy)
    bad = b.expect != 0
    if family == "G2":
        first = int((info[bad] == b.expect[bad]).sum())
        print(f"  {what}: {first} of {int(bad.sum())} name the first of the two zero columns")
        ok = (info == b.expect) | (info == b.alt)
        assert ok.all(), (what, [(int(k), int(info[k]), int(b.expect[k]), int(b.alt[k])) for k in np.flatnonzero(~ok)[:10]])
    elif family in ("C2", "C3") and same_tile_only(case):
        exact = int((info[bad] == b.expect[bad]).sum())
        print(f"  {what}: {exact} of {int(bad.sum())} name the column itself")
        assert not info[healthy].any(), (what, info[healthy])
        ok = ((info[bad] - 1) // ic.TILE == (b.expect[bad] - 1) // ic.TILE) & (info[bad] >= 1) & (info[bad] <= n)
        assert ok.all(), (what, [(int(k), int(info[bad][k]), int(b.expect[bad][k])) for k in np.flatnonzero(~ok)[:10]])
    else:
        assert np.array_equal(info, b.expect), (what, mismatches(info, b.expect))
    for name, v in out.items():
        assert np.isnan(v[bad]).all(), f"{what}: {name} of a flagged matrix is not all NaN"
        assert np.isfinite(v[healthy]).all(), f"{what}: {name} of a healthy matrix is not finite"
    alone, info_alone = launch(case, subset(x, healthy))
    assert not info_alone.any(), (what, info_alone)
    for name, v in out.items():
        assert np.array_equal(bits(v[healthy]), bits(alone[name])), f"{what}: {name} of a healthy matrix depends on its neighbours"


@pytest.mark.parametrize("case", CASES, ids=inst.case_id)
def test_info_names_the_first_failing_column(case):
    assert name_of(case) == case.name
    for family in (ic.GJ_FAMILIES if gauss_jordan(case) else ic.CHOL_FAMILIES):
        check_family(case, family)
