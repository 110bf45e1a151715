"""Which compiled kernels can a request reach, and does the generated sweep (tests/_instantiations.py) run each of them at the edges
of its range? Reads the kernels' host-side launch stubs (symbol names only) from the built library; no GPU.

A name the library reports equals the demangled stub name up to trailing default template arguments (the prefix rule bench.py
uses for profiles/traffic.json: matinv_gj_tile_f64<4, true, true> is the stub matinv_gj_tile_f64<4, true, true, false>).
"""
import re
import shutil
import subprocess

import pytest

import _instantiations as inst
from conftest import pkg

NM = shutil.which("nm") or shutil.which("llvm-nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
pytestmark = pytest.mark.skipif(NM is None, reason="no nm on this machine")

# Kernels no route function names: pattern of the stub name -> how the suite reaches it. Everything else must be named by a route.
F = r"f(64|32)"
T = r"(double|float)"
B = r"(true|false)"
REACHED_OTHERWISE = {
    # second kernels of a launch: the matrices the first pass rejected, through a device-side work list
    rf"matinv_(gj|chol|gp)_lds_worklist<{T}>": "rejects of the generated batches (general / not-SPD items of the tile sweeps)",
    rf"matinv_gj_row_worklist<{T}, \d+>": "singular items the pivoting tile work-list kernel hands on",
    rf"matinv_solve_row_worklist<{T}, \d+, \d+>": "general items the fused Gauss-Jordan solve rejects",
    # the screening pass and the early-exit natural-order kernels behind it
    rf"matinv_gj_tile_screen_{F}<\d+, {B}>": "test_gpu_instantiations.test_screened_launches_give_the_same_bits (MATINV_TILE_SCREEN=1)",
    rf"matinv_gj_tile4_screen_{F}<\d+>": "test_gpu_instantiations.test_screened_launches_give_the_same_bits (MATINV_TILE_SCREEN=1)",
    # multi-launch paths: every kernel of the chain runs in any case of that path
    rf"matinv_bgj_\w+<{T}.*>": "any BLOCKED Gauss-Jordan case",
    rf"matinv_(bgp|bldl|binv)_\w+<{T}.*>": "any BLOCKED Cholesky / blocked pipeline case",
    rf"matinv_solve_gemm<{T}>": "any composed solve case (nrhs 17)",
    rf"matinv_logml_combine<{T}>": "any logml case beyond the bordered tile kernel (n > 96)",
    r"matinv_segcopy": "the batching queue: test_binqueue / test_gpu_cli, not a size-dependent instantiation",
}

# A form of a kernel that differs from the named one in a TRAILING template argument only: the prefix rule cannot tell it from the named
# form, so a route name claims it too. Kept here so that how it is reached stays written down (and checked to exist).
SAME_NAME_OTHER_FORM = {
    rf"matinv_gj_tile_{F}<[34], {B}, true, true>": "EARLY form behind the screening pass: test_screened_launches_give_the_same_bits",
}


def stub_names():
    out = subprocess.run([NM, "-C", "--defined-only", pkg("_lib").LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        i = line.find("__device_stub__")
        if i < 0:
            continue
        s = line[i + len("__device_stub__"):]
        m = re.match(r"\w+", s)
        end = m.end()
        if s[end:end + 1] == "<":  # template arguments: up to the matching bracket
            depth = 0
            for j in range(end, len(s)):
                depth += {"<": 1, ">": -1}.get(s[j], 0)
                if depth == 0:
                    end = j + 1
                    break
        names.add(s[:end])
    return names


STUBS = stub_names() if NM else set()


def matches(name, stub):
    return stub == name or stub.startswith(name[:-1] + ",")


def test_library_holds_kernel_stubs():
    assert len(STUBS) > 300, len(STUBS)
    assert "matinv_gj_lds<double>" in STUBS and "matinv_segcopy" in STUBS


def test_every_enumerated_name_is_a_compiled_kernel():
    names = {name for _, name in inst.served()}
    assert len(names) > 150
    missing = sorted(n for n in names if not any(matches(n, s) for s in STUBS))
    assert not missing, f"named by a route function but not compiled: {missing}"


def test_every_compiled_kernel_is_reached():
    names = {name for _, name in inst.served()}
    unclaimed, claimed_by_table = [], {}
    for s in sorted(STUBS):
        if any(matches(n, s) for n in names):
            continue
        rule = next((p for p in REACHED_OTHERWISE if re.fullmatch(p, s)), None)
        if rule is None:
            unclaimed.append(s)
        else:
            claimed_by_table.setdefault(rule, []).append(s)
    assert not unclaimed, f"compiled, but no route names them and the table does not say how they are reached: {unclaimed}"
    idle = sorted(set(REACHED_OTHERWISE) - set(claimed_by_table))
    idle += [p for p in SAME_NAME_OTHER_FORM if not any(re.fullmatch(p, s) for s in STUBS)]
    assert not idle, f"table rows that match no compiled kernel: {idle}"
    print(f"{len(STUBS)} stubs: {len(STUBS) - sum(map(len, claimed_by_table.values()))} named by a route, "
          f"{sum(map(len, claimed_by_table.values()))} by the table")


def test_case_list_holds_both_ends_of_every_name():
    """counted here from scratch, one library call per (route, n), not from the generator's own table"""
    ends = {}
    for r in inst.routes():
        for n in inst.sizes():
            name = inst.route_name(r, n)
            if name:
                lo, hi = ends.get((r, name), (n, n))
                ends[(r, name)] = (min(lo, n), max(hi, n))
    have = set(inst.cases())
    missing = [(r, name, n) for (r, name), (lo, hi) in ends.items() for n in (lo, hi) if inst.Case(r, name, n) not in have]
    assert not missing, missing[:10]
    assert len(ends) == len(inst.served())
    # the sizes at which the host code branches without the name saying so
    t = inst.blocked_gj_two_level_min()
    gj_blocked = {c.n for c in have if c.route == inst.Route("inverse", "gj", "f64", "blocked", 0)}
    assert {1, t - 1, t, inst.N_MAX} <= gj_blocked
    # and the fp32 pipeline sizes either side of where its LDS fallback kernel drops to one workgroup per CU
    for entry in ("mean", "variance"):
        ns = {c.n for c in have if c.route == inst.Route(entry, "", "f32", "", 0)}
        assert {inst.PIPELINE_F32_LDS_MAX, inst.PIPELINE_F32_LDS_MAX + 1} <= ns
    assert all(inst.batch_of(c.n) <= 2 for c in have if c.n > 256)
    ids = [inst.case_id(c) for c in inst.cases()]
    assert len(set(ids)) == len(ids)


def test_a_refused_request_has_no_name():
    """forced families just past the end of their range, and everything beyond n = 1024"""
    api = inst.api
    assert api.kernel_name(inst.GJ, inst.F32, 300, api.KERNEL_TILE) == ""  # was matinv_gj_tile4_f32<19, ...>: not compiled
    assert api.kernel_name(inst.CH, inst.F64, 193, api.KERNEL_TILE) == ""
    assert api.kernel_name(inst.CH, inst.F64, 64, api.KERNEL_TILEP) == "" == api.kernel_name(inst.CH, inst.F64, 64, api.KERNEL_ROW)
    assert api.kernel_name(inst.GJ, inst.F64, 65, api.KERNEL_ROW) == "" == api.kernel_name(inst.GJ, inst.F64, 17, api.KERNEL_ROWLANE)
    for r in inst.routes():
        assert inst.route_name(r, inst.N_MAX + 1) == "", r
        for n in inst.refused(r):
            assert inst.route_name(r, n) == ""
    assert api.gp_kernel_name(inst.F64, 100) == "matinv_gp_spd_tile_f64<7>" == api.gp_kernel_name(inst.F64, 100, variance=True)
    assert api.gp_kernel_name(inst.F32, 137) == "matinv_gp_spd_tile_f32<9>" and api.gp_kernel_name(inst.F32, 161) == "matinv_bgp_update<float>"
    assert api.gp_kernel_name(inst.F64, 12) == "matinv_gj_rowlane<double, 16, false, true, true>"
    assert api.logml_kernel_name(inst.F64, 96) == "matinv_logdet_tile_f64<6, true, true>"
    assert api.logml_kernel_name(inst.F64, 97) == api.gp_kernel_name(inst.F64, 97, variance=True)
