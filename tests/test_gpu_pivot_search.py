"""The pivot search of every pivoting kernel, pinned row by row: matrices with ONE candidate of order 1 per elimination step, at a chosen
row, every other candidate of order delta (tests/_pivot_cases.py; what a search that misses the row once costs is shown on the CPU by
tests/test_pivot_cases_cpu.py: at least 8 times the bound, where a correct search stays below 1/8 of it). The permutations walk every
pair (step mod 16, pivot row mod 16), every (tile column, tile row), pivots inside and outside their own block of four, both parities,
each as A and as A^T. What a worker process does per list: tests/_pivot_worker.py.

No tolerance is new: the bounds are those of tests/test_gpu_parity.py, tests/test_gpu_solve.py and tests/test_gpu_logdet.py at each
matrix's own condition number (below 5), the sign of the determinant and every count are exact, the screened run is compared bit for bit."""
import functools
import os
import subprocess
import sys

import pytest

import _pivot_worker as PW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_pivot_worker.py")
GROUPS = [(dt, g) for dt in ("f64", "f32") for g in PW.GROUPS[dt]]
TIMEOUT = {"small": 30, "onewave": 30, "multiwave": 45, "wide": 45, "forced": 45}  # a worker takes 2 to 4 s, most of it start-up


def run_worker(args, screen, timeout):
    env = dict(os.environ, MATINV_DEBUG_REJECTS="1", MATINV_TILE_SCREEN=screen)
    p = subprocess.run([sys.executable, WORKER] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=timeout)
    print(p.stdout[-20000:])
    assert p.returncode == 0 and "pivot-worker ok" in p.stdout, (p.stdout[-3000:], p.stderr[-4000:])
    return [ln for ln in p.stdout.splitlines() if ln.startswith("BITS ")]


@functools.lru_cache(maxsize=None)
def unscreened_once(dtype, group):
    """the BITS lines of the unscreened worker, or the exception it ended with: a worker that failed (or faulted) is not started again"""
    try:
        return run_worker(["all", dtype] + list(PW.GROUPS[dtype][group]), "0", TIMEOUT[group])
    except (AssertionError, subprocess.TimeoutExpired) as e:
        return e


def unscreened(dtype, group):
    result = unscreened_once(dtype, group)
    if isinstance(result, BaseException):
        raise result
    return result


@pytest.mark.parametrize("dtype,group", GROUPS)
def test_pivot_lists(dtype, group):
    """AUTO (the pivoting kernel behind the natural-order one produced the bits: the counter says so), the PIVOT policy, every forced
    family that serves the size, and the sign and value of the log-determinant"""
    bits = unscreened(dtype, group)
    assert len(bits) == 2 * len(PW.GROUPS[dtype][group])


@pytest.mark.parametrize("dtype,group", GROUPS)
def test_pivot_lists_behind_the_screening_pass(dtype, group):
    """the AUTO route again under MATINV_TILE_SCREEN=1: the same counts and the same output bits"""
    want = unscreened(dtype, group)  # first: where the unscreened worker failed, the screened one is not started
    assert run_worker(["auto", dtype] + list(PW.GROUPS[dtype][group]), "1", TIMEOUT[group]) == want


def test_both_routes_of_the_64x64_fp64_kernel():
    """no member is symmetric: the first launch of a process runs the symmetric-only kernel in front and hands the whole batch over,
    the second takes the two-arm kernel directly; same bits, same counts"""
    run_worker(["front"], "0", 30)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_solve_routes(dtype):
    """the fused solve (its rejects go to the row solve), the row solve under the PIVOT policy, the composed route"""
    run_worker(["solve", dtype], "0", 30)
