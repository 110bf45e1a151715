"""CPU half of the several-rounds coverage (tests/test_gpu_grid_stride.py, tests/_stride_worker.py): the pools are what the GPU test
takes them for -- checked with the CPU oracle and numpy alone --, the case table names the kernels the library launches, and the batch
sizes still wrap every grid the launch sites ask for."""
import os
import re

import numpy as np
import pytest

import _stride_worker as W
import oracle
from conftest import as_mats, pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-matrix-inversion_amd", "csrc")
ALL_CASES = W.cases() + W.screen_cases()


def pool_key(c):
    return ("gp" if c.op in ("mean", "variance", "logml") else c.algo, c.dtype, c.n)


def one_case_per_pool():
    """one case per pool and kind of check: the pipeline pools per entry point (their vectors differ), the logdet cases on their own
    (signs, and a bound of their own), the singular variant"""
    seen = {}
    for c in ALL_CASES:
        seen.setdefault(pool_key(c) + ((c.op,) if pool_key(c)[0] == "gp" or c.op == "logdet" else ()) + (c.variant == "singular",), c)
    return list(seen.values())


POOL_CASES = one_case_per_pool()


def tolerance_of(case, cond):
    """the looser end of the existing bound of the case's entry point at condition number cond, as a relative error"""
    n, f64 = case.n, case.dtype == "f64"
    if case.op == "inverse":
        return 1e-15 * cond * n * 8 if f64 else 2e-6 * max(cond, 10.0)
    if case.op in ("solve", "logml"):
        return 1e-15 * cond * n if f64 else 1e-5 * cond
    return n * n * W.U[case.dtype] * cond  # logdet; mean and variance have an absolute bound, their matrices are those of logml


@pytest.mark.parametrize("case", POOL_CASES, ids=W.case_id)
def test_pool_members_are_flagged_exactly_as_intended(case):
    n = case.n
    inputs, M, kinds = W.pool_of(case)
    intended = np.array([W.intended_info(k, n) for k in kinds])
    _, info = W.oracle_info(case)
    # the singular / not-SPD / NaN members are exactly the ones the oracle flags, with the columns they were built for
    assert info.tolist() == intended.tolist()
    singular = case.variant == "singular"
    assert sorted(kinds) == sorted(W.GJ_KINDS_SINGULAR if singular else (W.GJ_KINDS if pool_key(case)[0] == "gj" else W.CHOL_KINDS))
    ok = intended == 0
    # every other member is healthy. COND_CAP and the 0.1 below are limits of the pool's construction (draws beyond the cap are
    # drawn again), not bounds on anything the GPU computes: below them the existing bounds of the anchor leave at least one digit
    cond = np.linalg.cond(M[ok])
    assert np.isfinite(cond).all() and cond.max() <= W.COND_CAP, (W.case_id(case), float(cond.max()))
    if case.op != "logdet":
        assert max(tolerance_of(case, c) for c in cond) <= 0.1, (W.case_id(case), float(cond.max()))
    # 47 distinct items, and the same bits on every build
    main = inputs["B" if "B" in inputs and "A" not in inputs else "A"]
    assert len({m.tobytes() for m in main}) == W.P
    if pool_key(case)[0] == "gj":
        assert np.array_equal(W.gj_pool.__wrapped__(n, case.dtype, singular)[0], W.gj_pool(n, case.dtype, singular)[0], equal_nan=True)
    else:
        assert np.array_equal(W.chol_pool.__wrapped__(n, case.dtype)[0], W.chol_pool(n, case.dtype)[0], equal_nan=True)
    if pool_key(case)[0] == "gj":
        a = as_mats(main, n)
        sym = np.array([np.array_equal(m, m.T) for m in a])
        for k, kind in enumerate(kinds):
            if kind == "spd":
                assert sym[k], "an SPD member is not bitwise symmetric"
            if kind == "dominant":
                assert not sym[k]
        general = [k for k, kind in enumerate(kinds) if kind == "general"]
        assert 0.55 < (len(general) + (kinds.count("zero_row") if singular else 0)) / W.P < 0.65
        if n == 64:
            assert sum(sym[general]) == len(general) // 2, "half of the general members are symmetric (indefinite) at n = 64"
            assert all(np.linalg.eigvalsh(a[k].astype(np.float64)).min() < 0 for k in general if sym[k])
            # the second grid of the 64 x 64 fp64 front route (256 * 8 workgroups over the not-symmetric list, csrc/tile_impl.hpp:1057)
            # and the screening pass (256 * 16 over the batch, :1071) wrap as well
            assert (W.BATCH_ONE_WAVE // W.P) * int((~sym).sum()) > 256 * 8 and W.BATCH_ONE_WAVE > 2 * 256 * 16
        else:
            assert not sym[general].any()
        if case.op == "logdet":
            assert set(np.linalg.slogdet(M[ok])[0]) == {-1.0, 1.0}, "the healthy members carry both signs"
    else:
        a = as_mats(main, n)
        iu = np.triu_indices(n, 1)
        assert (a[:, iu[0], iu[1]] == np.float64(1e30).astype(a.dtype)).all(), "garbage above the diagonal of every member"
        assert 0.55 < (~ok).sum() / W.P < 0.65
        assert (np.linalg.eigvalsh(M[ok]).min(axis=1) > 0).all()


@pytest.mark.parametrize("case", [c for c in POOL_CASES if c.op in ("mean", "variance")], ids=W.case_id)
def test_pipeline_oracle_flags_the_same_members(case):
    """oracle.mean_batched / variance_batched refuse exactly the flagged members and serve the others"""
    n = case.n
    inputs, M, kinds = W.pool_of(case)
    ok = np.array([W.intended_info(k, n) == 0 for k in kinds])
    f = {k: v.astype(np.float64) for k, v in inputs.items()}
    # what the pipeline reads of B is its lower triangle: the oracle gets the mirrored image
    low = np.ascontiguousarray(W.lower_image(inputs["B"], n).transpose(0, 2, 1)).reshape(W.P, -1)
    run = (lambda s: oracle.mean_batched(f["a"][s], low[s], f["c"][s], f["d"][s], n)) if case.op == "mean" else \
        (lambda s: oracle.variance_batched(f["a"][s], low[s], f["c"][s], f["e"][s], n))
    assert np.isfinite(run(ok)).all()
    with pytest.raises(ArithmeticError, match=f"^{int((~ok).sum())} matrices"):
        run(slice(None))
    for k in np.flatnonzero(~ok):
        with pytest.raises(ArithmeticError):
            run(slice(k, k + 1))


def test_case_table_names_the_kernels_the_library_launches():
    """the family each case expects is the one the route functions name, on both sides of every boundary the table was cut at; and every
    batch wraps the grid of its kernel at least twice with a ragged tail"""
    api = pkg("api")
    algo = {"gj": api.ALGO_GAUSS_JORDAN, "chol": api.ALGO_CHOLESKY}
    kern = {"auto": api.KERNEL_AUTO, "tilep": api.KERNEL_TILEP, "row": api.KERNEL_ROW}
    for c in ALL_CASES:
        code = api.F64 if c.dtype == "f64" else api.F32
        if c.policy == "pivot":
            continue  # the name follows the process-wide policy: the worker checks it where it sets the policy
        name = {"inverse": lambda: api.kernel_name(algo[c.algo], code, c.n, kern[c.kernel]),
                "solve": lambda: api.solve_kernel_name(algo[c.algo], code, c.n, c.nrhs, kern[c.kernel]),
                "logdet": lambda: api.logdet_kernel_name(algo[c.algo], code, c.n, kern[c.kernel]),
                "logml": lambda: api.logml_kernel_name(code, c.n),
                "mean": lambda: api.gp_kernel_name(code, c.n, False),
                "variance": lambda: api.gp_kernel_name(code, c.n, True)}[c.op]()
        assert c.expect in name, (W.case_id(c), c.expect, name)
        batch = W.batch_of(name)
        assert batch % W.P != 0 and batch % 256 != 0
        grid = W.fallback_grid(c, name)
        if grid is not None:
            assert 0.55 * batch > grid[1], (W.case_id(c), batch, grid)
        grid2 = W.second_grid(c, name)
        assert (grid2 is not None) == (c.variant == "singular")
        if grid2 is not None:
            assert (batch // W.P) * W.GJ_KINDS_SINGULAR.count("zero_row") > grid2[1], (W.case_id(c), batch, grid2)
    ids = [(c.group, W.case_id(c)) for c in ALL_CASES]
    assert len(set(ids)) == len(ids)


def sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".inc"))}


# launch sites of workgroups of several wavefronts: the files whose tile_grid() calls size a grid of 128 .. 1024 threads per workgroup
MULTI_WAVE_FILES = {"tile4_impl.hpp", "tilep4_impl.hpp", "tileq_impl.hpp", "spd_tile2_kernels.hip"}
ONE_WAVE_FILES = {"tile_impl.hpp", "tile_kernels.hip", "tile_f32_kernels.hip", "tilep_impl.hpp", "gp_tile_impl.hpp", "solve_tile_impl.hpp",
                  "logdet_tile_impl.hpp", "loo_tile_impl.hpp", "logml_grad_tile_impl.hpp", "predict_tile_impl.hpp"}


def call_args(line, start):
    """the top-level arguments of the call whose opening parenthesis ends at line[start - 1]"""
    args, depth, cur = [], 0, ""
    for ch in line[start:]:
        if ch == ")" and depth == 0:
            return args + [cur.strip()]
        depth += (ch == "(") - (ch == ")")
        if ch == "," and depth == 0:
            args, cur = args + [cur.strip()], ""
        else:
            cur += ch
    raise AssertionError(f"call continues on the next line: {line}")


def test_batches_still_wrap_every_launch_site():
    """scan csrc/ for the grids: a per-CU figure above what the batch constants of tests/_stride_worker.py assume, or a launch site in a
    file nobody classified, fails here -- otherwise the GPU test would quietly stop striding"""
    src = sources()
    sites = {}
    for f, text in src.items():
        for ln, line in enumerate(text.splitlines(), 1):
            if line.lstrip().startswith(("//", "inline unsigned tile_grid", "unsigned tile_grid")):
                continue
            for m in re.finditer(r"\btile_grid\(", line):
                sites[(f, ln, m.start())] = (line, [int(v) for v in re.findall(r"(\d+)u", call_args(line, m.end())[1])])
    assert {f for f, _, _ in sites} == MULTI_WAVE_FILES | ONE_WAVE_FILES, sorted({f for f, _, _ in sites})
    assert len(sites) >= 20
    for (f, ln, _), (line, per_cu) in sites.items():
        assert per_cu, (f, ln, line)
        one_wave = f in ONE_WAVE_FILES or "sgrid" in line  # the screening pass of the tile4 family is a one-wavefront kernel
        limit = W.ONE_WAVE_PER_CU if one_wave else W.MULTI_WAVE_PER_CU
        assert max(per_cu) <= limit, f"{f}:{ln} asks for {max(per_cu)} workgroups per CU, the batches assume {limit}: {line.strip()}"
    # whole-batch ROW kernels
    row_caps = [(f, int(v)) for f, text in src.items() for v in re.findall(r"cap = 256u \* (\d+)u \* tile_grid_rounds\(\)", text)]
    assert sorted(f for f, _ in row_caps) == ["logdet_row_kernels.hip", "row_kernels.hip", "solve_row_kernels.hip"]
    assert all(v <= W.ROW_BLOCKS_PER_CU for _, v in row_caps), row_caps
    # persistent grids
    for f, fn in (("rowlane_kernels.hip", "rowlane_occupancy"), ("rowlane2_kernels.hip", "rl2_occupancy")):
        body = re.search(r"constexpr int " + fn + r"\([^)]*\)\s*\{?\s*return ([^;]*);", src[f])
        assert body, fn
        values = [int(v) for v in re.findall(r"[?:]\s*\(?\s*(\d+)\b", body.group(1))]
        assert values and max(values) <= W.MAX_OCCUPANCY, (fn, values)
        assert re.search(r"resident = 256u \* \(unsigned\)" + fn, src[f]), f"the grid of {f} is no longer 256 * occupancy blocks"
    # the fixed grids of the fallback kernels, as fallback_grid() states them
    assert len(re.findall(r"_lds_worklist<T>, dim3\(1024\)", src["lds_kernels.hip"])) == 3
    assert "dim3(512 * wl_rounds), dim3(256)" in src["solve_row_kernels.hip"]
    assert src["row_kernels.hip"].count("dim3(512 * wl_rounds), dim3(256)") == 2
    assert "tile_grid(batch, 12u, 1u)" in src["tilep_impl.hpp"] and "tile_grid(batch, 4u, 1u)" in src["tilep4_impl.hpp"]
    assert "tile_grid(batch, 1u, 1u)" in src["tileq_impl.hpp"]
    assert "tile_grid(batch, 8u, 1u)" in src["tile_impl.hpp"] and "tile_grid(batch, 16u, 1u)" in src["tile_impl.hpp"]


def test_every_case_of_the_table_belongs_to_a_group_the_gpu_test_runs():
    """the GPU test names its groups literally: a group added to the table and not to the test would never run"""
    import test_gpu_grid_stride as G
    assert sorted(G.GROUPS) == sorted(W.groups()) and sorted(G.SCREEN_GROUPS) == sorted(W.groups(screen=True))
    assert len(set(G.GROUPS)) == len(G.GROUPS)
