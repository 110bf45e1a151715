"""The acceptance test of the natural-order Gauss-Jordan kernels, |m| <= 4, pinned AT its threshold at every position: matrices whose
one offending multiplier is exactly +-4 (accepted) or one ulp beyond (rejected), at a chosen pivot and row, counted through
MATINV_DEBUG_REJECTS=1. The constructions, the float64 model that shows where each multiplier lands, and the lists: tests/_accept_cases.py
(checked on the CPU by tests/test_accept_cases_cpu.py). What a worker process does per list: tests/_accept_worker.py.

Every group runs twice, under MATINV_TILE_SCREEN=0 and =1 (rejects of the first block step then come out of the screening kernels): the
same counts and the same output bits. No tolerance is new: the numeric bounds are those of tests/test_gpu_parity.py and
tests/test_gpu_solve.py at each matrix's own condition number, every other comparison is a count or bitwise.

The fused solve (csrc/solve_tile_impl.hpp) gives every matrix the verdict of the inverse route. These tests found that it did not: it
used to update, and test, only the tile rows that still held unpivoted rows, so a type B matrix whose already pivoted row lies in an
EARLIER tile row formed no multiplier beyond 4 there and was solved by the fused kernel where inverse_batched hands the same matrix over
(rejects of the solve / reject variants in the thinned lists then: fp64 52/53, 78/84, 104/143 at n = 17, 33, 64; fp32 52/53, 78/84,
118/157). The Gauss-Jordan form now carries the pivoted tile rows through the columns still to be pivoted, for the test alone."""
import functools
import os
import subprocess
import sys

import pytest

import _accept_worker as AW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_accept_worker.py")
GROUPS = [(dt, g) for dt in ("f64", "f32") for g in AW.GROUPS[dt]]

def run_worker(args, screen):
    env = dict(os.environ, MATINV_DEBUG_REJECTS="1", MATINV_TILE_SCREEN=screen)
    p = subprocess.run([sys.executable, WORKER] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=300)
    print(p.stdout[-20000:])
    assert p.returncode == 0 and "accept-worker ok" in p.stdout, (p.stdout[-3000:], p.stderr[-4000:])
    return [ln for ln in p.stdout.splitlines() if ln.startswith("BITS ")]


@functools.lru_cache(maxsize=None)
def unscreened(dtype, group):
    return run_worker(["inverse", dtype] + list(AW.GROUPS[dtype][group]), "0")


@pytest.mark.parametrize("dtype,group", GROUPS)
def test_threshold_lists(dtype, group):
    bits = unscreened(dtype, group)
    assert len(bits) == 3 * len(AW.GROUPS[dtype][group])


@pytest.mark.parametrize("dtype,group", GROUPS)
def test_threshold_lists_behind_the_screening_pass(dtype, group):
    """the same verdict bit for bit: counts and every output bit of the screened run equal the unscreened run's"""
    assert run_worker(["inverse", dtype] + list(AW.GROUPS[dtype][group]), "1") == unscreened(dtype, group)


def test_symmetric_lists_on_the_front_kernel():
    """64 x 64 fp64, the symmetric members only, first launch of its process: every call runs the symmetric-only kernel in front and finds
    nothing not symmetric; the same counts. (In the `onewave` worker the same members run in the lower-tile arm of the two-arm kernel.)"""
    assert len(run_worker(["front"], "0")) == 3


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_fused_solve_values_and_scaling(dtype):
    run_worker(["solve-values", dtype], "0")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_fused_solve_counts_match_the_inverse_route(dtype):
    """the counter against the reject variants in the list and, where both run the same sweep, against inverse_batched's"""
    run_worker(["solve-counts", dtype], "0")
