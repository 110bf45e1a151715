"""Pools, case table and worker of tests/test_gpu_grid_stride.py (tests/test_grid_stride_cpu.py checks the pools and the launch sites
on the CPU): every batch-striding kernel run for several rounds of its grid, rejects included.

ONE process per group under MATINV_TILE_GRID_MULT=1 MATINV_DEBUG_REJECTS=1 (the library reads its switches once per process): every
grid is one round of resident workgroups, so a batch of a few thousand matrices makes each workgroup take a second and a third matrix.

A case is (entry point, algorithm, dtype, n, forced family). Its inputs are a POOL of P = 47 distinct items; the batch is built on the
device as pool[i % 47]. 47 is prime and every grid is a multiple of 256, so the item a workgroup meets in its next round is always
another pool member. Per case:

  1. anchor: the pool alone (47 items, nothing strides). Against float64 numpy / the CPU oracle on the float64 image of exactly the
     input, with the bounds the project already uses (cited at each check below); info equals the oracle's; every output of a flagged
     member is NaN; inputs bitwise unchanged.
  2. head: the first batch % 47 members alone: bit-equal to the anchor.
  3. the strided call, outputs and info pre-filled with sentinels: every output of a healthy item is bit-identical to the anchor's
     output for that member (integer views, torch.equal, on the device); info equals the anchor's; outputs of flagged items are NaN
     and their number is the multiplicity of the flagged members; inputs bitwise unchanged; the MATINV_DEBUG_REJECTS counter grew by
     (batch // 47) * r_pool + r_head, the growth measured on calls 1 and 2 (an entry lost from, or written twice to, a work list
     filled in a second round shows here), and exceeds the fixed grid of the fallback kernel behind the list.
  4. the strided call again: same bits, same count. Before the first strided call of a Gauss-Jordan case the reject hint of the launch
     history is reset by an all-SPD call, so the first strided call runs unscreened and the second one behind the screening pass --
     unless MATINV_TILE_SCREEN pins the choice; under MATINV_TILE_SCREEN=1 every batch is at least 8229, two rounds of the screening
     kernels' 4096 workgroups. In the main worker the second launch of a case beyond n = 64 is screened too, but its batch of 2085
     does not wrap the tile4 screening kernel: those are covered by the screened worker alone.

Two variants. "front": 64 x 64 fp64 in a process of its own with the strided call FIRST, because the front route (the symmetric-only
kernel over the batch, then the two-arm kernel on 256 * 8 workgroups over the not-symmetric list) is taken only until a front launch
has found a quarter of its batch not symmetric, which the pool does; matinv_sym_front_stats must show the front launch, the batch and
more than 2048 not-symmetric items, and no front launch for the screened second call. The anchor follows and is compared afterwards.
In every other process the 64 x 64 fp64 launches take the direct route (the two-arm kernel alone). "singular": 26 of the 47 members
have a zero row, so the kernel that takes the singular matrices from the pivoting work-list kernel (ROW work list, 512 blocks of four
matrices; LDS work list, 1024 workgroups) wraps as well. Behind the wide pivoting kernel (n > 128) that second level is not wrapped.

Prints one line per case (kernel, batch, rejects, ok) and `stride-worker ok`; exits non-zero at the first failure or HIP error and
starts nothing after it. No tolerance is new: every numeric bound is one of another test module, every new comparison is bitwise."""
import collections
import functools
import importlib
import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import oracle  # noqa: E402
from conftest import as_mats, rel_err  # noqa: E402

P = 47
NP_DTYPES = {"f64": np.float64, "f32": np.float32}
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}

# ---- batch sizes: two full rounds of the largest grid of the class at MATINV_TILE_GRID_MULT=1, plus a ragged tail of 37 ---------------
# grid = tile_grid(batch, per_cu) = 256 * per_cu workgroups (csrc/common.hpp:169). tests/test_grid_stride_cpu.py fails when a launch
# site asks for more per CU than assumed here.
ONE_WAVE_PER_CU = 16   # largest per-CU figure of a 64-thread launch: csrc/tile_impl.hpp:1070 (fp32), :1071 (screening pass),
#                        csrc/tile_f32_kernels.hip:17, csrc/solve_tile_impl.hpp:285; 12 at csrc/tile_impl.hpp:1055, csrc/tile_kernels.hip:250,
#                        csrc/tilep_impl.hpp:464; 8 at csrc/tile_impl.hpp:1134, csrc/gp_tile_impl.hpp:185, csrc/logdet_tile_impl.hpp:201
MULTI_WAVE_PER_CU = 4  # workgroups of several wavefronts: csrc/spd_tile2_kernels.hip:20, csrc/tilep4_impl.hpp:404; 3 / 1 at
#                        csrc/tile4_impl.hpp:314, 1 at csrc/tileq_impl.hpp:509
ROW_BLOCKS_PER_CU = 2  # whole-batch ROW kernels, four matrices per 256-thread block: csrc/row_kernels.hip:131,
#                        csrc/solve_row_kernels.hip:125, csrc/logdet_row_kernels.hip:88
MAX_OCCUPANCY = 6      # persistent grids, 256 * occupancy blocks of four waves: rowlane_occupancy (csrc/rowlane_kernels.hip:206, grid
#                        at :394), rl2_occupancy (csrc/rowlane2_kernels.hip:140, grid at :294)
BATCH_ONE_WAVE = 2 * 256 * ONE_WAVE_PER_CU + 37           # 8229
BATCH_MULTI_WAVE = 2 * 256 * MULTI_WAVE_PER_CU + 37       # 2085
BATCH_ROW = 4 * 256 * ROW_BLOCKS_PER_CU * 4 + 37          # 8229: four rounds of 2048 matrices
BATCH_ROWLANE8 = 2 * 256 * MAX_OCCUPANCY * 4 * 8 + 37     # 98341: eight matrices per wavefront
BATCH_ROWLANE16 = 2 * 256 * MAX_OCCUPANCY * 4 * 4 + 37    # 49189: four matrices per wavefront (gj_rowlane<16>, gj_rowlane2)
assert (BATCH_ONE_WAVE, BATCH_MULTI_WAVE, BATCH_ROW, BATCH_ROWLANE8, BATCH_ROWLANE16) == (8229, 2085, 8229, 98341, 49189)

MULTI_WAVE_FAMILIES = ("gj_tile4_", "gj_tilep3_", "gj_tilep4_", "gj_tileqw_", "spd_tile2_", "spd_tile2w_", "spd_tile3w_")


def batch_of(name):
    """the batch that wraps the grid of the kernel `name` at least twice"""
    if "gj_rowlane<" in name:
        return BATCH_ROWLANE8 if re.search(r"rowlane<\w+, 8,", name) else BATCH_ROWLANE16
    if "gj_rowlane2<" in name:
        return BATCH_ROWLANE16
    if any(f in name for f in MULTI_WAVE_FAMILIES):
        return BATCH_MULTI_WAVE
    if any(f in name for f in ("gj_row<", "solve_row<", "logdet_row<")):
        return BATCH_ROW
    return BATCH_ONE_WAVE


def fallback_grid(case, name):
    """(what, matrices per round) of the fixed grid of the work-list kernel behind the first kernel, or None where the first kernel
    finishes its matrices itself. Grids in workgroups = matrices, except the ROW solve (four per block)."""
    nt = int(re.search(r"<(\d+)", name).group(1)) if re.search(r"_f(64|32)<\d+", name) else 0
    if case.op in ("mean", "variance", "logml"):
        if any(f in name for f in ("gj_rowlane2<", "gp_tile_", "gp_spd_tile_", "spd_tile2_f64<true>")):
            return "gp_lds_worklist", 1024          # csrc/lds_kernels.hip:487
        return None
    if case.op == "solve" and "solve_tile_" in name:
        return ("solve_row_worklist", 512 * 4) if case.algo == "gj" else None  # csrc/solve_row_kernels.hip:108
    if case.op == "logdet" or case.kernel != "auto" or case.policy == "pivot":
        return None
    if case.algo == "chol":
        if "spd_tile_f" in name or "spd_tile2_f64<" in name:
            return "chol_lds_worklist", 1024        # csrc/lds_kernels.hip:461
        return None
    if "gj_rowlane2<" in name or "gj_tile_f" in name:
        return "gj_tilep on the list", 256 * 12     # csrc/tilep_impl.hpp:464
    if "gj_tile4_" in name:
        return ("gj_tilep3/4 on the list", 256 * 4) if nt <= 8 else ("gj_tileqw on the list", 256)  # csrc/tilep4_impl.hpp:404, csrc/tileq_impl.hpp:509
    return None


def second_grid(case, name):
    """(what, matrices per round) of the fixed grid of the kernel that takes the SINGULAR matrices from the pivoting work-list kernel"""
    if case.variant != "singular":
        return None
    if "gj_tile_f" in name:
        return "gj_row_worklist", 512 * 4           # csrc/row_kernels.hip:119, blocks of four matrices
    assert "gj_tile4_" in name and int(re.search(r"<(\d+)", name).group(1)) <= 8
    return "gj_lds_worklist", 1024                  # csrc/lds_kernels.hip:449


# ---- the pools (numpy only) -----------------------------------------------------------------------------------------------------------
ORDER = (np.arange(P) * 17) % P  # where the j-th entry of a kind list goes: the kinds interleave

GJ_KINDS = ["general"] * 28 + ["spd"] * 7 + ["dominant"] * 7 + ["mild"] * 2 + ["zero_row", "nan", "last_col"]
GJ_KINDS_SINGULAR = ["general"] * 4 + ["zero_row"] * 26 + ["spd"] * 7 + ["dominant"] * 7 + ["mild"] * 2 + ["nan"]
CHOL_KINDS = ["neg_first"] * 9 + ["neg_mid"] * 9 + ["neg_last"] * 9 + ["nan"] + ["spd"] * 19
assert len(GJ_KINDS) == P and len(CHOL_KINDS) == P and len(GJ_KINDS_SINGULAR) == P


# Healthy members stay below this 2-norm condition number, so that the existing bounds of the anchor mean something for each of them:
# at 1e4 the fp32 inverse is held to 2e-6 * cond = 2 % and the fp32 solve to 1e-5 * cond = 10 %, the fp64 ones to 1e-10 .. 2e-8.
COND_CAP = 1e4


def seed_of(n, dtype):
    return 100003 * n + (64 if dtype == "f64" else 32)


def nan_at(n):
    return min(3, n - 1)


def intended_info(kind, n):
    """the info code a pool member is built to have (0: healthy)"""
    return {"zero_row": n,             # partial pivoting never picks the zero row: it is the one left for the last step
            "nan": nan_at(n) + 1, "last_col": n, "neg_first": 1, "neg_mid": n // 2 + 1, "neg_last": n}.get(kind, 0)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def gj_pool(n, dtype, singular=False):
    """(A[P, n*n] in memory order [k, col, row], kinds[P]). About 60 % U(0,1) general matrices as conftest.general_batch (at n = 64 half of
    them symmetrised: symmetric indefinite), bitwise symmetric dominant SPD ones as conftest.spd_batch, R + n I, two mild ones
    R + R^T + 0.35 n I, a zero row, a single NaN, a zero last column (exactly singular as well, but the natural-order sweep runs to its
    last step before it rejects). singular: GJ_KINDS_SINGULAR instead, 26 members with a zero row."""
    rng = np.random.default_rng(seed_of(n, dtype))
    r = rng.random((P, n, n))
    for k in range(P):  # a draw beyond COND_CAP (as rounded to dtype, and symmetrised) is drawn again
        while max(np.linalg.cond(m.astype(NP_DTYPES[dtype]).astype(np.float64)) for m in (r[k], r[k] + r[k].T)) > COND_CAP:
            r[k] = rng.random((n, n))
    s = r + r.transpose(0, 2, 1)
    a = np.empty_like(r)
    kinds = [None] * P
    eye = np.eye(n)
    for j, kind in enumerate(GJ_KINDS_SINGULAR if singular else GJ_KINDS):
        k = int(ORDER[j])
        kinds[k] = kind
        if kind == "general":
            a[k] = s[k] if (n == 64 and j % 2 == 0) else r[k]
        elif kind == "dominant":
            a[k] = r[k] + n * eye
        elif kind == "mild":
            a[k] = s[k] + 0.35 * n * eye
        else:
            a[k] = s[k] + n * eye
        if kind == "zero_row":
            a[k, :, n // 2] = 0.0
        elif kind == "nan":
            a[k, nan_at(n), nan_at(n)] = np.nan
        elif kind == "last_col":
            a[k, n - 1, :] = 0.0
    a, = _frozen(a.reshape(P, n * n).astype(NP_DTYPES[dtype]))
    return a, tuple(kinds)


@functools.lru_cache(maxsize=None)
def chol_pool(n, dtype):
    """(B[P, n*n], kinds[P]). About 60 % not positive definite: diagonal entry -1 at column 1, at the middle column, at column n (the
    construction of _loo_worker.break_three), one NaN on the diagonal; the rest SPD. 1e30 in the strict upper triangle of every matrix,
    which these entry points must not read."""
    rng = np.random.default_rng(seed_of(n, dtype) + 1)
    r = rng.random((P, n, n))
    a = r + r.transpose(0, 2, 1) + n * np.eye(n)
    kinds = [None] * P
    for j, kind in enumerate(CHOL_KINDS):
        k = int(ORDER[j])
        kinds[k] = kind
        if kind == "nan":
            a[k, nan_at(n), nan_at(n)] = np.nan
        elif kind != "spd":
            i = intended_info(kind, n) - 1
            a[k, i, i] = -1.0
    iu = np.triu_indices(n, 1)
    a[:, iu[1], iu[0]] = 1e30  # element (row, col) with row < col (memory is [k, col, row])
    a, = _frozen(a.reshape(P, n * n).astype(NP_DTYPES[dtype]))
    return a, tuple(kinds)


def lower_image(a, n):
    """(P, n, n) float64 [k, row, col] from the lower triangles: what ALGO_CHOLESKY and the pipeline read"""
    m = as_mats(a, n).astype(np.float64)
    return np.tril(m) + np.tril(m, -1).transpose(0, 2, 1)


# variant: "" | "front" (fresh process, the strided call first: the 64 x 64 fp64 front route) | "singular" (more than half of the pool
# exactly singular: the ROW / LDS work-list kernel behind the pivoting kernel wraps its grid as well)
Case = collections.namedtuple("Case", "group op algo dtype n kernel nrhs policy expect variant", defaults=("",))


def case_id(c):
    return f"{c.op}-{c.algo}-{c.dtype}-n{c.n}" + (f"-{c.kernel}" if c.kernel != "auto" else "") + (f"-nrhs{c.nrhs}" if c.nrhs else "") + \
        (f"-{c.policy}" if c.policy else "") + (f"-{c.variant}" if c.variant else "")


@functools.lru_cache(maxsize=None)
def pool_of(case):
    """inputs {name: array[P, width]} in call order, the matrices M[P, n, n] in float64 as the entry point reads them, kinds"""
    n, dt = case.n, NP_DTYPES[case.dtype]
    rng = np.random.default_rng(seed_of(n, case.dtype) + 2)
    if case.op in ("mean", "variance", "logml"):
        B, kinds = chol_pool(n, case.dtype)
        flagged = np.array([intended_info(k, n) != 0 for k in kinds])
        a, c, d = (rng.random((P, n)).astype(dt) for _ in range(3))
        e = rng.random((P, 1)).astype(dt)
        c[flagged] = 0.0  # M = B for the members built to fail: their column is the intended one
        M = lower_image(B, n) + np.stack([np.diag(v) for v in c.astype(np.float64)])
        inputs = {"mean": {"a": a, "B": B, "c": c, "d": d}, "variance": {"a": a, "B": B, "c": c, "e": e},
                  "logml": {"B": B, "c": c, "d": d}}[case.op]
    else:
        A, kinds = gj_pool(n, case.dtype, case.variant == "singular") if case.algo == "gj" else chol_pool(n, case.dtype)
        M = as_mats(A, n).astype(np.float64) if case.algo == "gj" else lower_image(A, n)
        inputs = {"A": A}
        if case.op == "solve":
            inputs["B"] = rng.standard_normal((P, n * case.nrhs)).astype(dt)
    _frozen(*inputs.values())
    return inputs, M, kinds


def oracle_info(case):
    """info[P] of the CPU oracle on the float64 image of the matrices the entry point reads"""
    _, M, _ = pool_of(case)
    flat = np.ascontiguousarray(M.transpose(0, 2, 1)).reshape(-1)
    algo = oracle.ALGO_GJ_PIVOT if (case.algo == "gj" and case.op in ("inverse", "solve", "logdet")) else oracle.ALGO_CHOLESKY
    want, info = oracle.inverse_batched(flat, case.n, algo)
    return want.reshape(P, -1), info


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
GJ_AUTO = {5: "gj_rowlane<{T}, 8, false, false", 8: "gj_rowlane<{T}, 8, true, false", 12: "gj_rowlane<{T}, 16, false, false",
           16: "gj_rowlane<{T}, 16, true, false", 20: "gj_rowlane2<{T}, 24, false, 0>", 24: "gj_rowlane2<{T}, 24, true, 0>",
           33: "gj_tile_{F}<3, false", 48: "gj_tile_{F}<3, true", 50: "gj_tile_{F}<4, false", 64: "gj_tile_{F}<4, true",
           72: "gj_tile4_{F}<5, false", 96: "gj_tile4_{F}<6, true", 100: "gj_tile4_{F}<7, false", 128: "gj_tile4_{F}<8, true",
           130: "gj_tile4_{F}<9, false, 9", 160: "gj_tile4_{F}<10, false, 10", 192: "gj_tile4_{F}<12, false, 12"}
GJ_TILEP = {33: "gj_tilep_{F}<3, false>", 64: "gj_tilep_{F}<4, true>", 96: "gj_tilep3_{F}<6, true>", 128: "gj_tilep4_{F}<8, true>",
            192: "gj_tileqw_{F}<12, false>"}
CHOL_F64 = {5: "gj_rowlane<double, 8, false, true, false>", 16: "gj_rowlane<double, 16, true, true, false>", 17: "spd_tile_f64<2, false>",
            96: "spd_tile_f64<6, true>", 100: "spd_tile_f64<7, false>", 112: "spd_tile_f64<7, true>", 120: "spd_tile2_f64<false>",
            128: "spd_tile2_f64<false>", 130: "spd_tile2w_f64<9, false>", 176: "spd_tile2w_f64<11, false>", 177: "spd_tile3w_f64<12, false>",
            192: "spd_tile3w_f64<12, false>"}
CHOL_F32 = {5: "gj_rowlane<float, 8, false, true, false>", 16: "gj_rowlane<float, 16, true, true, false>", 17: "spd_tile_f32<2, false>",
            96: "spd_tile_f32<6, true>", 100: "spd_tile_f32<7, false>", 112: "spd_tile_f32<7, true>", 120: "spd_tile_f32<8, false>",
            128: "spd_tile_f32<8, false>", 130: "spd_tile_f32<9, false>", 144: "spd_tile_f32<9, false>", 160: "spd_tile_f32<10, false>",
            161: "gj_tile4_f32<11, false, 11, true>", 176: "gj_tile4_f32<11, false, 11, true>", 177: "gj_tile4_f32<12, false, 12, true>",
            192: "gj_tile4_f32<12, false, 12, true>", 256: "gj_tile4_f32<16, false, 16, true>"}
# mean and variance; logml takes the bordered logdet tile kernel up to n = 96 and the variance's kernel beyond
GP_F64 = {5: "gj_rowlane<double, 8, false, true, true>", 16: "gj_rowlane<double, 16, true, true, true>", 20: "gj_rowlane2<double, 24, false, 2>",
          33: "gp_tile_f64<3, false>", 80: "gp_tile_f64<5, true>", 81: "gp_spd_tile_f64<6>", 112: "gp_spd_tile_f64<7>",
          120: "spd_tile2_f64<true>", 130: "spd_tile2w_f64<9, true>", 180: "spd_tile3w_f64<12, true>"}
GP_F32 = {33: "gp_tile_f32<3, false>", 96: "gp_tile_f32<6, true>", 100: "gp_spd_tile_f32<7>", 128: "gp_spd_tile_f32<8>",
          137: "gp_spd_tile_f32<9>", 138: "gp_spd_tile_f32<9>", 160: "gp_spd_tile_f32<10>"}


def _fmt(s, dtype):
    return s.format(T="double" if dtype == "f64" else "float", F=dtype)


def _logml_expect(n, dtype, gp_expect):
    s = {"f64": "logdet_tile_f64", "f32": "logdet_tile_f32"}[dtype]
    return f"{s}<{(n + 15) // 16}, {'true' if n % 16 == 0 else 'false'}, true>" if n <= 96 else gp_expect


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for dtype in ("f64", "f32"):
        g = f"gj_auto_{dtype}"
        table = dict(GJ_AUTO)
        if dtype == "f32":
            table[80] = "gj_tile4_f32<5, true, 1"    # the last size of the one-wavefront form of the fp32 tile4 kernel
            table[256] = "gj_tile4_f32<16, false, 16"
        table.pop(160)
        for n in sorted(table):
            out.append(Case(g + ("_small" if n <= 24 else ("_onewave" if n <= 64 else ("_multiwave" if n <= 128 else "_wide"))), "inverse", "gj", dtype, n, "auto", 0, "",
                            _fmt(table[n], dtype)))
        for n in (48, 100):
            out.append(Case(f"gj_singular_{dtype}", "inverse", "gj", dtype, n, "auto", 0, "", _fmt(GJ_AUTO[n], dtype), "singular"))
        for n, e in GJ_TILEP.items():
            out.append(Case(f"gj_forced_{dtype}", "inverse", "gj", dtype, n, "tilep", 0, "", _fmt(e, dtype)))
        for n, e in ((20, "gj_row<{T}, 32>"), (64, "gj_row<{T}, 64>")):
            out.append(Case(f"gj_forced_{dtype}", "inverse", "gj", dtype, n, "row", 0, "", _fmt(e, dtype)))
        for n, e in (CHOL_F64 if dtype == "f64" else CHOL_F32).items():
            out.append(Case(f"chol_{dtype}" + ("_small" if n <= 16 else ("_onewave" if n <= 112 else "_wide")), "inverse", "chol", dtype, n,
                            "auto", 0, "", e))
        for algo, spd in (("gj", "false"), ("chol", "true")):
            for n, nt, full in ((17, 2, "false"), (64, 4, "true")):
                for nrhs in (1, 16):
                    out.append(Case(f"solve_{dtype}", "solve", algo, dtype, n, "auto", nrhs, "", f"solve_tile_{dtype}<{nt}, {full}, {spd}>"))
        out.append(Case(f"solve_{dtype}", "solve", "gj", dtype, 24, "auto", 17, "", _fmt("gj_rowlane2<{T}, 24, true, 0>", dtype)))
        out.append(Case(f"solve_{dtype}", "solve", "chol", dtype, 24, "auto", 17, "", f"spd_tile_{dtype}<2, false>"))
        out.append(Case(f"solve_{dtype}", "solve", "gj", dtype, 40, "auto", 3, "pivot", _fmt("solve_row<{T}, 64, 4>", dtype)))
        for n, e in ((17, "logdet_tile_{F}<2, false, false>"), (96, "logdet_tile_{F}<6, true, false>")):
            out.append(Case(f"logdet_{dtype}", "logdet", "chol", dtype, n, "auto", 0, "", _fmt(e, dtype)))
        for n in (33, 64):
            out.append(Case(f"logdet_{dtype}", "logdet", "gj", dtype, n, "auto", 0, "", _fmt("logdet_row<{T}, 64>", dtype)))
        for n, e in (GP_F64 if dtype == "f64" else GP_F32).items():
            for op in ("mean", "variance", "logml"):
                out.append(Case(f"gp_{dtype}" + ("_small" if n <= 20 else ("_onewave" if n <= 112 or dtype == "f32" else "_wide")), op, "chol",
                                dtype, n, "auto", 0, "", _logml_expect(n, dtype, e) if op == "logml" else e))
    # a process of its own, the strided call its first launch: only then does the 64 x 64 fp64 launch take the front route
    out.append(Case("gj_front_f64", "inverse", "gj", "f64", 64, "auto", 0, "", "gj_tile_f64<4, true", "front"))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def screen_cases():
    """the second worker, under MATINV_TILE_SCREEN=1: Gauss-Jordan AUTO behind the screening pass"""
    return tuple(Case(f"gj_screen_{dtype}", "inverse", "gj", dtype, n, "auto", 0, "", _fmt(GJ_AUTO[n], dtype))
                 for dtype in ("f64", "f32") for n in (50, 64, 100, 160))


def groups(screen=False):
    seen = []
    for c in (screen_cases() if screen else cases()):
        if c.group not in seen:
            seen.append(c.group)
    return seen


# ---- float64 references and the existing bounds ------------------------------------------------------------------------------------
def check_anchor(case, outs, info, inputs, M, winv, winfo):
    """outs: {name: array[P, width]} of the one-round call on the pool. Healthy members against float64; the bounds are those of the
    modules cited."""
    n, f64, u = case.n, case.dtype == "f64", U[case.dtype]
    assert np.array_equal(info, winfo), ("info differs from the oracle's", info.tolist(), winfo.tolist())
    ok = np.flatnonzero(winfo == 0)
    bad = np.flatnonzero(winfo != 0)
    for name, v in outs.items():
        assert np.isnan(v[bad]).all(), f"{name} of a flagged member is not all NaN"
        assert np.isfinite(v[ok]).all(), f"{name} of a healthy member is not finite"
    cond = np.linalg.cond(M[ok])
    worst = 0.0
    if case.op == "inverse":
        got = outs["X"].astype(np.float64)
        for j, k in enumerate(ok):
            if f64:  # tests/_switch_worker.py: rel_err < max(1e-10, 1e-15 cond n 8)
                err, tol = rel_err(got[k], winv[k], n), max(1e-10, 1e-15 * cond[j] * n * 8)
            else:    # tests/_switch_worker.py: relative Frobenius error < 2e-6 max(cond, 10)
                err, tol = np.linalg.norm(got[k] - winv[k]) / np.linalg.norm(winv[k]), 2e-6 * max(cond[j], 10.0)
            worst = max(worst, err / tol)
            assert err < tol, (case_id(case), int(k), err, tol)
    elif case.op == "solve":  # tests/test_gpu_solve.py check_close
        nrhs = case.nrhs
        bs = inputs["B"].astype(np.float64).reshape(P, nrhs, n).transpose(0, 2, 1)
        got = outs["X"].astype(np.float64).reshape(P, nrhs, n).transpose(0, 2, 1)
        want = np.linalg.solve(M[ok], bs[ok])
        for j, k in enumerate(ok):
            if f64:
                floor = 1e-3 * np.abs(want[j]).max()
                err, tol = (np.abs(got[k] - want[j]) / np.maximum(np.abs(want[j]), floor)).max(), max(1e-10, 1e-15 * cond[j] * n)
            else:
                err, tol = np.linalg.norm(got[k] - want[j]) / np.linalg.norm(want[j]), 1e-5 * cond[j]
            worst = max(worst, err / tol)
            assert err < tol, (case_id(case), int(k), err, tol)
    elif case.op == "logdet":  # tests/test_gpu_logdet.py check_logdet
        wsign, wld = np.linalg.slogdet(M[ok])
        for j, k in enumerate(ok):
            b = n * n * u * cond[j] + n * u * max(1.0, abs(wld[j]))
            err = abs(float(outs["logabsdet"][k, 0]) - wld[j])
            worst = max(worst, err / b)
            assert outs["sign"][k, 0] == wsign[j] and err <= b, (case_id(case), int(k), err, b)
    elif case.op == "logml":  # tests/test_gpu_logdet.py check_logml
        dd = inputs["d"].astype(np.float64)[ok]
        q = np.einsum("ki,ki->k", dd, np.linalg.solve(M[ok], dd[:, :, None])[:, :, 0])
        sign, ld = np.linalg.slogdet(M[ok])
        assert (sign == 1).all()
        want = -0.5 * q - 0.5 * ld - 0.5 * n * math.log(2 * math.pi)
        for j, k in enumerate(ok):
            q_tol = 0.5 * abs(q[j]) * (max(1e-10, 1e-15 * cond[j] * n) if f64 else 1e-5 * cond[j])
            tol = 0.5 * (n * n * u * cond[j] + n * u * max(1.0, abs(ld[j]))) + q_tol
            err = abs(float(outs["logml"][k, 0]) - want[j])
            worst = max(worst, err / tol)
            assert err <= tol, (case_id(case), int(k), err, tol)
    else:  # tests/test_gpu_parity.py test_pipeline_synthetic: |err| < 1e-10 (fp64), 2e-5 (fp32)
        aa = inputs["a"].astype(np.float64)[ok]
        rhs = inputs["d"].astype(np.float64)[ok] if case.op == "mean" else aa
        s = np.einsum("ki,ki->k", aa, np.linalg.solve(M[ok], rhs[:, :, None])[:, :, 0])
        want = s if case.op == "mean" else inputs["e"].astype(np.float64)[ok, 0] - s
        err, tol = np.abs(outs["out"][ok, 0].astype(np.float64) - want).max(), (1e-10 if f64 else 2e-5)
        worst = err / tol
        assert err < tol, (case_id(case), err, tol)
    return worst


# ---- the GPU side ---------------------------------------------------------------------------------------------------------------------
SENTINEL = -12345.0


def main(argv):
    import torch
    api = importlib.import_module("cuda-matrix-inversion_amd.api")
    assert os.environ.get("MATINV_TILE_GRID_MULT") == "1" and os.environ.get("MATINV_DEBUG_REJECTS") == "1"
    assert os.environ.get("MATINV_GJ_POLICY") in (None, "", "natural"), "the default Gauss-Jordan policy is what is claimed bit-stable"
    assert torch.cuda.is_available()
    screen = os.environ.get("MATINV_TILE_SCREEN") == "1"
    todo = [c for c in (screen_cases() if screen else cases()) if c.group in argv]
    assert todo, f"no case in the groups {argv}"
    ALGO = {"gj": api.ALGO_GAUSS_JORDAN, "chol": api.ALGO_CHOLESKY}
    KERNEL = {"auto": api.KERNEL_AUTO, "tilep": api.KERNEL_TILEP, "row": api.KERNEL_ROW}
    bits = {torch.float64: torch.int64, torch.float32: torch.int32}

    def name_of(c):
        code = api.F64 if c.dtype == "f64" else api.F32
        if c.op == "inverse":
            return api.kernel_name(ALGO[c.algo], code, c.n, KERNEL[c.kernel])
        if c.op == "solve":
            return api.solve_kernel_name(ALGO[c.algo], code, c.n, c.nrhs, KERNEL[c.kernel])
        if c.op == "logdet":
            return api.logdet_kernel_name(ALGO[c.algo], code, c.n, KERNEL[c.kernel])
        if c.op == "logml":
            return api.logml_kernel_name(code, c.n)
        return api.gp_kernel_name(code, c.n, c.op == "variance")

    def widths(c):
        n = c.n
        return {"inverse": {"X": n * n}, "solve": {"X": n * c.nrhs}, "logdet": {"sign": 1, "logabsdet": 1}, "logml": {"logml": 1}}.get(c.op, {"out": 1})

    def call(c, t, batch):
        """one call of the entry point on `batch` items; returns ({name: tensor[batch, width]}, info, growth of the reject counter)"""
        dt = next(iter(t.values())).dtype
        outs = {k: torch.full((batch, w), SENTINEL, dtype=dt, device="cuda") for k, w in widths(c).items()}
        info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
        api.debug_rejects(reset=True)
        flat = {k: v.reshape(-1) for k, v in t.items()}
        o = {k: v.reshape(-1) for k, v in outs.items()}
        n = c.n
        if c.op == "inverse":
            api.inverse_batched(flat["A"], n, ALGO[c.algo], out=o["X"], info=info, kernel=KERNEL[c.kernel], batch=batch)
        elif c.op == "solve":
            api.solve_batched(flat["A"], flat["B"], n, c.nrhs, ALGO[c.algo], info=info, out=o["X"], kernel=KERNEL[c.kernel], batch=batch)
        elif c.op == "logdet":
            api.logdet_batched(flat["A"], n, ALGO[c.algo], sign=o["sign"], out=o["logabsdet"], info=info, kernel=KERNEL[c.kernel], batch=batch)
        elif c.op == "logml":
            api.logml_batched(n, flat["B"], flat["c"], flat["d"], out=o["logml"], batchSize=batch, info=info)
        elif c.op == "mean":
            api.calcluateMean(n, flat["a"], flat["B"], flat["c"], flat["d"], Means=o["out"], batchSize=batch, info=info)
        else:
            api.calcluateVariance(n, flat["a"], flat["B"], flat["c"], flat["e"], Variances=o["out"], batchSize=batch, info=info)
        torch.cuda.synchronize()
        return outs, info, api.debug_rejects()

    def same_bits(x, y):
        return torch.equal(x.contiguous().view(bits[x.dtype]), y.contiguous().view(bits[y.dtype]))

    for c in todo:
        old_policy = api.set_gj_policy(api.GJ_PIVOT) if c.policy == "pivot" else None
        name = name_of(c)
        assert c.expect in name, f"{case_id(c)}: expected a kernel of the family {c.expect!r}, the library names {name!r}"
        batch = batch_of(name)
        if screen:  # the screening kernels are one-wavefront kernels on 256 * 16 workgroups, also in front of the tile4 family
            batch = max(batch, BATCH_ONE_WAVE)  # csrc/tile_impl.hpp:1071, csrc/tile4_impl.hpp:315
        inputs, M, kinds = pool_of(c)
        winv, winfo = oracle_info(c)
        assert winfo.tolist() == [intended_info(k, c.n) for k in kinds], "the pool is not what tests/test_grid_stride_cpu.py checked"
        pool = {k: torch.from_numpy(v).cuda() for k, v in inputs.items()}
        healthy = torch.from_numpy(winfo == 0).cuda()
        spd = torch.from_numpy(np.flatnonzero(np.array([k == "spd" for k in kinds]))).cuda()
        head = batch % P
        idx = torch.arange(batch, device="cuda") % P
        t = {k: v[idx].contiguous() for k, v in pool.items()}
        hb = healthy[idx]
        n_flagged = int((winfo != 0).sum()) * (batch // P) + int((winfo[:head] != 0).sum())
        n_singular = sum((batch // P) + (k < head) for k, kind in enumerate(kinds) if kind == "zero_row")
        grid, grid2 = fallback_grid(c, name), second_grid(c, name)

        def forget_history():
            # an all-accepted launch of this size and dtype resets the reject hint: the next launch runs unscreened. (The hint of the
            # 64 x 64 fp64 front route is only written by a front launch: see the "front" case.)
            if c.algo == "gj":
                call(c, {k: v[spd] for k, v in pool.items()}, int(spd.numel()))

        front_results = None
        if c.variant == "front":
            # Nothing of this size and dtype has run in this process: the launch is unscreened and takes the FRONT route, the
            # symmetric-only kernel over the batch and the two-arm kernel on 256 * 8 workgroups over the not-symmetric list
            # (csrc/tile_impl.hpp:1055-1057). It rejects more than a quarter, so the second launch is screened: no front route.
            assert len(todo) == 1 and not screen
            st0 = api.sym_front_stats()
            first = call(c, t, batch)
            st1 = api.sym_front_stats()
            assert st1["front_launches"] == st0["front_launches"] + 1 and st1["direct_launches"] == st0["direct_launches"], (st0, st1)
            assert st1["last_batch"] == batch and st1["last_not_symmetric"] > 256 * 8, st1
            second = call(c, t, batch)
            st2 = api.sym_front_stats()
            assert (st2["front_launches"], st2["direct_launches"]) == (st1["front_launches"], st1["direct_launches"]), (st1, st2)
            front_results = (first, second)
            route = f" front route, {st1['last_not_symmetric']} not symmetric > 2048;"

        # 1. the anchor
        forget_history()
        a_outs, a_info, r_pool = call(c, pool, P)
        for k, v in inputs.items():
            assert same_bits(pool[k], torch.from_numpy(v).cuda()), f"anchor: input {k} was modified"
        worst = check_anchor(c, {k: v.cpu().numpy() for k, v in a_outs.items()}, a_info.cpu().numpy(), inputs, M, winv, winfo)
        _, again_info, r_pool2 = call(c, pool, P)  # behind the screening pass now, where there is one: the list is as long
        assert r_pool2 == r_pool and torch.equal(again_info, a_info), (case_id(c), r_pool, r_pool2)
        # 2. the head of the last, ragged repetition of the pool
        forget_history()
        h_outs, h_info, r_head = call(c, {k: v[:head].contiguous() for k, v in pool.items()}, head)
        hh = healthy[:head]
        assert torch.equal(h_info, a_info[:head]), f"{case_id(c)}: info of the first {head} members alone differs"
        for k in a_outs:
            assert same_bits(h_outs[k][hh], a_outs[k][:head][hh]), f"{case_id(c)}: {k} of the first {head} members alone differs"
        want_rejects = (batch // P) * r_pool + r_head

        def verify(launch, outs, info, rejects):
            what = f"{case_id(c)} ({name}), batch {batch}, launch {launch}"
            for k, v in pool.items():
                assert same_bits(t[k], v[idx]), f"{what}: input {k} was modified"
            bad_rows = torch.nonzero(info != a_info[idx]).flatten()
            assert bad_rows.numel() == 0, f"{what}: info differs from the one-round call at {bad_rows[:8].tolist()}: " \
                f"{info[bad_rows[:8]].tolist()} for {a_info[idx][bad_rows[:8]].tolist()}"
            assert int((info != 0).sum()) == n_flagged and int((~hb).sum()) == n_flagged, f"{what}: flagged items"
            assert not bool(info[hb].any())
            for k, v in outs.items():
                want = a_outs[k][idx]
                if not same_bits(v[hb], want[hb]):
                    rows = torch.nonzero((v.view(bits[v.dtype]) != want.view(bits[v.dtype])).any(dim=1) & hb).flatten()
                    raise AssertionError(f"{what}: {k} differs from the one-round call in {rows.numel()} healthy items, first "
                                         f"{rows[:8].tolist()} (grid rounds {[int(r) for r in rows[:8] // 256]}...)")
                assert bool(torch.isnan(v[~hb]).all()), f"{what}: {k} of a flagged item is not all NaN"
            assert rejects == want_rejects, f"{what}: the reject lists took {rejects} entries, {batch // P} * {r_pool} + {r_head} = " \
                f"{want_rejects} expected"
            if grid is not None:
                assert rejects > grid[1], f"{what}: {rejects} rejects do not wrap the grid of {grid[0]} ({grid[1]})"
            if grid2 is not None:
                assert n_singular > grid2[1], f"{what}: {n_singular} singular items do not wrap the grid of {grid2[0]} ({grid2[1]})"

        # 3. and 4. the strided call, twice
        if front_results is not None:
            for launch, r in enumerate(front_results, 1):
                verify(launch, *r)
            rejects = front_results[1][2]
        else:
            route = ""
            forget_history()
            for launch in (1, 2):
                outs, info, rejects = call(c, t, batch)
                verify(launch, outs, info, rejects)
            del outs
        if old_policy is not None:
            api.set_gj_policy(old_policy)
        wraps = f"rejects {rejects} > {grid[1]} ({grid[0]})" if grid else f"rejects {rejects} (no fixed fallback grid)"
        if grid2:
            wraps += f", singular {n_singular} > {grid2[1]} ({grid2[0]})"
        print(f"{case_id(c)}: {name} batch {batch}{route} {wraps} anchor err/bound {worst:.3f} ok", flush=True)
        del t, pool, a_outs, front_results
    print("stride-worker ok", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
