"""Every kernel instantiation the host can route a request to, and the sizes at the edges of each one's range. No GPU needed.

The library names the __global__ function a request launches (matinv_kernel_name, matinv_solve_kernel_name,
matinv_logdet_kernel_name, matinv_gp_kernel_name, matinv_logml_kernel_name: pure host logic, "" for a request that would be
refused). This module asks for every n in 1 .. 1024 on every route and groups the sizes by the name that came back:

  inverse   algorithm x dtype x every KERNEL_* family (AUTO included)
  solve     the fused route with nrhs 1 and 16 (AUTO and TILE; for Gauss-Jordan also AUTO under the PIVOT policy, which takes the
            row solve instead), the composed route with nrhs 17 (AUTO)
  logdet    algorithm x dtype x (AUTO, TILE, ROW, GLOBAL)
  mean, variance, logml   dtype

A Case is one (route, name, n). cases() holds, for every name of every route, the first and the last n of each run of consecutive
sizes that name serves -- for a partial-tile instantiation n % 16 == 1 and 15, for a FULL one its single n -- and, for names whose
run is longer than a tile (LDS, GLOBAL, the blocked paths: no n in the name), the sizes inside the run at which the host code
branches: the two-level threshold of the blocked Gauss-Jordan. The mean / variance routes also keep the fp32 sizes 137 and 138: no
host branch, but the sizes either side of where the LDS fallback kernel (the pipeline kernels' rejects) drops to one workgroup per
CU. tests/test_instantiations_cpu.py checks the list against the kernels compiled into the library,
tests/test_gpu_instantiations.py runs it.
"""
import contextlib
import functools
from collections import namedtuple

import numpy as np

from conftest import as_mats, general_batch, pkg, spd_batch

api = pkg("api")
GJ, CH = api.ALGO_GAUSS_JORDAN, api.ALGO_CHOLESKY
F64, F32 = api.F64, api.F32
N_MAX = 1024

FAMILIES = {"auto": api.KERNEL_AUTO, "lds": api.KERNEL_LDS, "rowlane": api.KERNEL_ROWLANE, "tile": api.KERNEL_TILE,
            "row": api.KERNEL_ROW, "global": api.KERNEL_GLOBAL, "blocked": api.KERNEL_BLOCKED, "tilep": api.KERNEL_TILEP}
ALGOS = {"gj": GJ, "chol": CH}
DTYPES = {"f64": F64, "f32": F32}
LOGDET_FAMILIES = ("auto", "tile", "row", "global")
SOLVE_FUSED_NRHS, SOLVE_COMPOSED_NRHS = (1, 16), 17
PIPELINE_F32_LDS_MAX = 137  # last fp32 size at which two workgroups of the LDS fallback kernel (matinv_gp_lds_worklist) fit a CU

# entry: inverse / solve / logdet / mean / variance / logml; algo, dtype, family: keys of the tables above (algo and family "" where
# the entry point has none; for solve also "pivot": AUTO while matinv_set_gj_policy(PIVOT) holds); nrhs: 0 except for solve
Route = namedtuple("Route", "entry algo dtype family nrhs")
Case = namedtuple("Case", "route name n")


def routes():
    out = []
    for dt in DTYPES:
        for algo in ALGOS:
            out += [Route("inverse", algo, dt, fam, 0) for fam in FAMILIES]
            out += [Route("solve", algo, dt, fam, nrhs) for fam in ("auto", "tile") for nrhs in SOLVE_FUSED_NRHS]
            out.append(Route("solve", algo, dt, "auto", SOLVE_COMPOSED_NRHS))
            if algo == "gj":
                out += [Route("solve", algo, dt, "pivot", nrhs) for nrhs in SOLVE_FUSED_NRHS]
            out += [Route("logdet", algo, dt, fam, 0) for fam in LOGDET_FAMILIES]
        out += [Route(entry, "", dt, "", 0) for entry in ("mean", "variance", "logml")]
    return out


@contextlib.contextmanager
def gj_policy(policy):
    """the Gauss-Jordan policy of the process for the length of a with block (None: left alone)"""
    old = api.set_gj_policy(policy) if policy is not None else None
    try:
        yield
    finally:
        if old is not None:
            api.set_gj_policy(old)


def route_name(r, n):
    """the name the library gives for size n on route r ("" where the request would be refused)"""
    dt = DTYPES[r.dtype]
    if r.entry == "inverse":
        return api.kernel_name(ALGOS[r.algo], dt, n, FAMILIES[r.family])
    if r.entry == "solve":
        with gj_policy(api.GJ_PIVOT if r.family == "pivot" else None):
            name = api.solve_kernel_name(ALGOS[r.algo], dt, n, r.nrhs, FAMILIES.get(r.family, api.KERNEL_AUTO))
        # nrhs 1 and 16 are there for the fused kernels; where such a request takes the composed route, nrhs 17 covers it
        return name if r.nrhs == SOLVE_COMPOSED_NRHS or name.startswith("matinv_solve_") else ""
    if r.entry == "logdet":
        return api.logdet_kernel_name(ALGOS[r.algo], dt, n, FAMILIES[r.family])
    if r.entry in ("mean", "variance"):
        return api.gp_kernel_name(dt, n, r.entry == "variance")
    if r.entry == "logml":
        return api.logml_kernel_name(dt, n)
    raise ValueError(r.entry)


def sizes():
    return range(1, N_MAX + 1)


@functools.lru_cache(maxsize=None)
def served():
    """{(route, name): sorted list of the n that route serves with that kernel}"""
    table = {}
    for r in routes():
        for n in sizes():
            name = route_name(r, n)
            if name:
                table.setdefault((r, name), []).append(n)
    return table


def runs(ns):
    """maximal runs of consecutive integers in a sorted list, as (first, last)"""
    out, first = [], ns[0]
    for prev, cur in zip(ns, ns[1:]):
        if cur != prev + 1:
            out.append((first, prev))
            first = cur
    out.append((first, ns[-1]))
    return out


@functools.lru_cache(maxsize=None)
def blocked_gj_two_level_min():
    """smallest n at which the blocked Gauss-Jordan takes its two-level scheme: where the name of its dominant kernel changes"""
    return min(n for n in sizes() if "update_mfma" in api.kernel_name(GJ, F64, n, api.KERNEL_BLOCKED))


def internal_boundaries():
    t = blocked_gj_two_level_min()
    return (t - 1, t, PIPELINE_F32_LDS_MAX, PIPELINE_F32_LDS_MAX + 1)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for (r, name), ns in sorted(served().items()):
        picked = set()
        for first, last in runs(ns):
            picked.update((first, last))
            if last - first > 16 or r.entry in ("mean", "variance"):  # no n in the name: where the host branches; mean / variance: PIPELINE_F32_LDS_MAX
                picked.update(n for n in internal_boundaries() if first < n < last)
        out += [Case(r, name, n) for n in sorted(picked)]
    return tuple(out)


def case_id(c):
    r = c.route
    where = "-".join(x for x in (r.entry, r.algo, r.dtype, r.family, f"nrhs{r.nrhs}" if r.nrhs else "") if x)
    return f"{where}-{c.name}-n{c.n}".replace(" ", "")


def batch_of(n):
    """13 up to n = 64 (ragged against the 4 or 8 matrices per wavefront of the rowlane kernels), 5 up to 256, 2 beyond"""
    return 13 if n <= 64 else (5 if n <= 256 else 2)


def refused(r):
    """for a forced family: the sizes just past the end of each run it serves, where the request must be refused"""
    ns = sorted({n for (rr, _), v in served().items() if rr == r for n in v})
    if not ns or r.family in ("", "auto", "pivot"):
        return []
    return [last + 1 for _, last in runs(ns) if not route_name(r, last + 1)]


# ---- the inputs of a case (numpy only): built once per (kind, n, dtype) and shared, never modified -------------------------------------
NP_DTYPES = {"f64": np.float64, "f32": np.float32}
SINGULAR, WITH_NAN = 2, 3  # where a batch of at least 5 carries its singular matrix and its matrix with a NaN


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def gj_batch(n, dtype, mixed):
    """(batch, n*n) matrices in memory order [k, col, row] and the indices of the healthy ones.
    mixed: the batch of test_natural_pass_two_rows_per_lane -- SPD matrices, every third one general U(0,1) (the natural-order pass
    rejects it, the pivoting / worklist kernel runs), one singular (a zero row), one holding a NaN. Otherwise: all general, one
    singular. Batches of 2 have room for neither the singular matrix nor the NaN."""
    batch = batch_of(n)
    g = general_batch(n, batch, seed=1000 + n).reshape(batch, n, n)
    if mixed:
        a = spd_batch(n, batch, seed=900 + n).reshape(batch, n, n).copy()
        a[1::3] = g[1::3]
    else:
        a = g.copy()
    bad = []
    if batch >= 5:
        a[SINGULAR, :, n // 2] = 0.0  # memory [k, col, row]: row n/2 is zero
        bad.append(SINGULAR)
        if mixed:
            a[WITH_NAN, min(3, n - 1), min(3, n - 1)] = np.nan
            bad.append(WITH_NAN)
    ok = np.array([k for k in range(batch) if k not in bad])
    return _frozen(a.reshape(batch, n * n).astype(NP_DTYPES[dtype]), ok)


@functools.lru_cache(maxsize=None)
def chol_batch(n, dtype, with_bad=True):
    """(clean, dirty, ok): SPD matrices, the last one with pivot n/3 turned negative (not positive definite) when with_bad;
    dirty = the same with 1e30 in the strict upper triangle, which ALGO_CHOLESKY must not read"""
    batch = batch_of(n)
    clean = spd_batch(n, batch, seed=50 + n).reshape(batch, n, n).copy()
    if with_bad:
        clean[batch - 1, n // 3, n // 3] = -1.0
    dirty = clean.copy()
    iu = np.triu_indices(n, 1)
    dirty[:, iu[1], iu[0]] = 1e30  # element (row, col) with row < col (memory is [k, col, row])
    dt = NP_DTYPES[dtype]
    ok = np.arange(batch - 1 if with_bad else batch)
    return _frozen(clean.reshape(batch, n * n).astype(dt), dirty.reshape(batch, n * n).astype(dt), ok)


@functools.lru_cache(maxsize=None)
def solve_batch(n, dtype, algo):
    """healthy matrices only. gj: SPD, every third one general; chol: (clean, dirty) as above without the bad item"""
    if algo == "chol":
        clean, dirty, _ = chol_batch(n, dtype, with_bad=False)
        return clean, dirty
    batch = batch_of(n)
    a = spd_batch(n, batch, seed=900 + n).reshape(batch, n, n).copy()
    a[1::3] = general_batch(n, batch, seed=1000 + n).reshape(batch, n, n)[1::3]
    a, = _frozen(a.reshape(batch, n * n).astype(NP_DTYPES[dtype]))
    return a, a


@functools.lru_cache(maxsize=None)
def rhs_batch(n, nrhs, dtype):
    b, = _frozen(np.random.default_rng(n * nrhs).standard_normal((batch_of(n), n * nrhs)).astype(NP_DTYPES[dtype]))
    return b


@functools.lru_cache(maxsize=None)
def pipeline_batch(n):
    """the inputs of test_pipeline_synthetic in float64: (a, B, c, d, e)"""
    batch = batch_of(n)
    rng = np.random.default_rng(n)
    B = spd_batch(n, batch, seed=n)
    a, c, d = (rng.random(batch * n) for _ in range(3))
    return _frozen(a, B, c, d, rng.random(batch))


@functools.lru_cache(maxsize=None)
def max_cond(kind, n, dtype, mixed=False):
    """largest 2-norm condition number among the healthy matrices of a batch, in float64 on the rounded input"""
    if kind == "gj":
        a, ok = gj_batch(n, dtype, mixed)
    else:
        a, _, ok = chol_batch(n, dtype)
    return max(np.linalg.cond(m) for m in as_mats(a[ok].astype(np.float64), n))
