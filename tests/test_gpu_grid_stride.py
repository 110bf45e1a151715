"""Every batch-striding kernel for several rounds of its grid, rejects included: one worker process per group of cases under
MATINV_TILE_GRID_MULT=1 MATINV_DEBUG_REJECTS=1 (the library reads its switches once per process). What a case is, what is compared
and why nothing here needs a tolerance of its own: tests/_stride_worker.py. The pools and the launch sites the batch sizes are derived
from are checked on the CPU in tests/test_grid_stride_cpu.py."""
import os
import subprocess
import sys

import pytest

import _stride_worker as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_stride_worker.py")
# the groups of tests/_stride_worker.py cases(), one process each (tests/test_grid_stride_cpu.py compares the two lists)
GROUPS = ["gj_auto_f64_small", "gj_auto_f64_onewave", "gj_auto_f64_multiwave", "gj_auto_f64_wide", "gj_singular_f64", "gj_forced_f64",
          "chol_f64_small", "chol_f64_onewave", "chol_f64_wide", "solve_f64", "logdet_f64", "gp_f64_small", "gp_f64_onewave", "gp_f64_wide",
          "gj_auto_f32_small", "gj_auto_f32_onewave", "gj_auto_f32_multiwave", "gj_auto_f32_wide", "gj_singular_f32", "gj_forced_f32",
          "chol_f32_small", "chol_f32_onewave", "chol_f32_wide", "solve_f32", "logdet_f32", "gp_f32_onewave", "gj_front_f64"]
SCREEN_GROUPS = ["gj_screen_f64", "gj_screen_f32"]


def run_worker(group, extra_env, listed):
    e = dict(os.environ)
    e.update({"MATINV_TILE_GRID_MULT": "1", "MATINV_DEBUG_REJECTS": "1"})
    e.update(extra_env)
    p = subprocess.run([sys.executable, WORKER, group], capture_output=True, text=True, env=e, timeout=600)
    print(p.stdout[-20000:])
    assert p.returncode == 0 and "stride-worker ok" in p.stdout, (p.stdout[-3000:], p.stderr[-4000:])
    for c in listed:
        if c.group == group:
            assert any(line.startswith(W.case_id(c) + ": ") and line.endswith(" ok") for line in p.stdout.splitlines()), W.case_id(c)


@pytest.mark.parametrize("group", GROUPS)
def test_strided_call_gives_the_bits_of_the_one_round_call(group):
    run_worker(group, {}, W.cases())


@pytest.mark.parametrize("group", SCREEN_GROUPS)
def test_strided_call_behind_the_screening_pass(group):
    run_worker(group, {"MATINV_TILE_SCREEN": "1"}, W.screen_cases())
