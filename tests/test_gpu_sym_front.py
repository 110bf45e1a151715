"""Unscreened 64 x 64 fp64 Gauss-Jordan launches take one of two routes (csrc/tile_impl.hpp: launch_gj_tile_natural): FRONT = the
symmetric-only kernel matinv_gj_tile_f64<4, true, true, false, true> over the batch, then the two-arm kernel over the matrices it found
not symmetric; DIRECT = the two-arm kernel over the batch. The route is chosen by launch history alone (csrc/tile_kernels.hip:
tile_policy_use_sym_front) and must never show in a result. What this file pins:

* a symmetric batch, a mixed batch with rejects out of both kernels, and a not-symmetric list longer than the second launch's grid
  (2 048 workgroups) give the same bits on both routes, the same info and the same count of hand-overs to the pivoting kernel;
* the history rule: front until a completed front launch found a quarter of its batch not symmetric, then direct with one probe at
  every 32nd launch (matinv_sym_front_stats);
* the device-table entry point (a BatchRef that is not contiguous) on the front route.

Routes are selected the way a caller meets them: a fresh process starts on the front route; a process that has inverted an R + n I
batch and synchronised is on the direct route for its next 31 launches. Every step asserts its route through sym_front_stats.
The expected value is numpy.linalg.inv at the bound of test_gpu_sym_sweep.py, rel_err < max(1e-10, 1e-15 cond n), inputs built as
there (R + R^T + n I: cond <= 2.3; R + R^T + 2 n diag(+-1): cond <= 1.8; R + n I is strictly diagonally dominant by rows, cond < 10)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import as_mats, general_batch, spd_batch
from test_gpu_sym_sweep import N, ROOT, built, check_each, flat, indefinite_batch

pytestmark = pytest.mark.gpu

# One child process runs a list of steps (a JSON file): {"src": input.npy, "inv": where the inverse goes or None, "info": ..., "after":
# where the input buffer as it is afterwards goes or None, "table": call the device-table entry, "same_as": index of an earlier step whose
# inverse this one must equal bit for bit}. One STEP line per step: the route it took and what the counters say after a synchronise.
WORKER = r"""
import ctypes, importlib, json, sys, numpy as np, torch
sys.path.insert(0, %r)
api = importlib.import_module("cuda-matrix-inversion_amd.api")
L = importlib.import_module("cuda-matrix-inversion_amd._lib").lib()
n, kept = 64, {}
for k, st in enumerate(json.load(open(sys.argv[1]))):
    a = np.load(st["src"])
    batch = a.size // (n * n)
    api.debug_rejects(reset=True)
    before = api.sym_front_stats()
    d = torch.from_numpy(a).cuda()
    if st.get("table"):
        # scattered slots, 64 values of padding each, visited in another order than the batch's: nothing contiguous about it
        slot = n * n + 64
        order = [(7 * i) %% batch for i in range(batch)]
        assert sorted(order) == list(range(batch))
        d_in = torch.zeros(batch * slot, dtype=torch.float64, device="cuda")
        d_out = torch.zeros_like(d_in)
        for i, o in enumerate(order):
            d_in[o * slot:o * slot + n * n] = d[i * n * n:(i + 1) * n * n]
        tin = (ctypes.c_void_p * batch)(*[d_in.data_ptr() + 8 * o * slot for o in order])
        tout = (ctypes.c_void_p * batch)(*[d_out.data_ptr() + 8 * o * slot for o in order])
        torch.cuda.synchronize()
        before = api.sym_front_stats()
        # the reference's signature: void, no error code -- on any failure the entry prints the library's message and ends the
        # process (abi.hip: die_on), which run_steps reports with that text; info is not returned through this entry either
        L.inverse_gauss_batched_device.restype = None
        L.inverse_gauss_batched_device(None, n, tin, tout, batch)
        torch.cuda.synchronize()
        res = d_out.cpu().numpy()
        x = np.concatenate([res[o * slot:o * slot + n * n] for o in order])
        info = np.zeros(batch, dtype=np.int32)
    else:
        dinfo = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
        dx = api.inverse_batched(d, n, api.ALGO_GAUSS_JORDAN, info=dinfo, batch=batch)
        torch.cuda.synchronize()
        x, info = dx.cpu().numpy(), dinfo.cpu().numpy()
    after = api.sym_front_stats()
    rec = {"front": after["front_launches"] - before["front_launches"], "direct": after["direct_launches"] - before["direct_launches"],
           "not_symmetric": after["last_not_symmetric"], "last_batch": after["last_batch"], "rejects": api.debug_rejects(reset=True),
           "kernel": api.kernel_name(api.ALGO_GAUSS_JORDAN, api.F64, n)}
    if st.get("same_as") is not None:
        rec["same"] = bool(np.array_equal(x, kept[st["same_as"]][0]) and np.array_equal(info, kept[st["same_as"]][1]))
    if st.get("keep"):
        kept[k] = (x, info)
    if st.get("inv"):
        np.save(st["inv"], x)
        np.save(st["info"], info)
    if st.get("after"):
        np.save(st["after"], d.cpu().numpy())
    print("STEP", json.dumps(rec))
print("WORKER-OK")
""" % ROOT


def run_steps(tmp_path, tag, steps):
    """steps: dicts with "a" (flat batch) and the worker's options -> per step (record, inverse or None, info or None, after or None)"""
    spec, saved = [], {}
    for k, st in enumerate(steps):
        s = {key: v for key, v in st.items() if key not in ("a", "save", "save_after")}
        key = id(st["a"])
        if key not in saved:
            saved[key] = str(tmp_path / f"{tag}{k}_a.npy")
            np.save(saved[key], st["a"])
        s["src"] = saved[key]
        if st.get("save"):
            s["inv"], s["info"] = str(tmp_path / f"{tag}{k}_inv.npy"), str(tmp_path / f"{tag}{k}_info.npy")
        if st.get("save_after"):
            s["after"] = str(tmp_path / f"{tag}{k}_after.npy")
        spec.append(s)
    path = str(tmp_path / f"{tag}_steps.json")
    json.dump(spec, open(path, "w"))
    r = subprocess.run([sys.executable, "-c", WORKER, path], env=dict(os.environ, MATINV_DEBUG_REJECTS="1"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "WORKER-OK" in r.stdout, r.stdout + r.stderr
    recs = [json.loads(ln.split(" ", 1)[1]) for ln in r.stdout.splitlines() if ln.startswith("STEP")]
    assert len(recs) == len(steps)
    assert all(rec["kernel"].startswith("matinv_gj_tile_f64<4, true, true") for rec in recs), recs
    out = []
    for rec, s in zip(recs, spec):
        out.append((rec, np.load(s["inv"]) if "inv" in s else None, np.load(s["info"]) if "info" in s else None,
                    np.load(s["after"]) if "after" in s else None))
    return out


def took(rec, route):
    assert (rec["front"], rec["direct"]) == ((1, 0) if route == "front" else (0, 1)), (route, rec)


def dominant(batch, seed):
    """R + n I: accepted by the natural order, not symmetric"""
    return as_mats(general_batch(N, batch, seed=seed), N) + N * np.eye(N)


def symmetric_256():
    sym = as_mats(spd_batch(N, 256, seed=9101), N).copy()
    sym[128:] = indefinite_batch(128, seed=9102)
    return sym


def mixed_512():
    """alternating symmetric / R + n I; ten built rejects among the symmetric ones, ten U(0,1) matrices among the others"""
    sym, gen = as_mats(spd_batch(N, 256, seed=9103), N).copy(), dominant(256, seed=9104)
    plan = [(2, 0, 1e-3), (3, 0, 0.0), (30, 6, 1e-3), (31, 6, 0.0), (50, 40, 1e-3), (51, 40, 0.0), (70, 9, 1e-3), (71, 9, 0.0),
            (254, 61, 1e-3), (255, 61, 0.0)]
    for k, i, delta in plan:
        sym[k] = built(sym[k], i, delta)
    assert np.array_equal(sym, sym.transpose(0, 2, 1))
    uni = [0, 1, 17, 64, 99, 128, 129, 200, 254, 255]
    gen[uni] = as_mats(general_batch(N, len(uni), seed=9105), N)
    mixed = np.empty((512, N, N))
    mixed[0::2], mixed[1::2] = sym, gen
    return mixed, [2 * k for k, _, _ in plan], [2 * k + 1 for k in uni]


@pytest.fixture(scope="module")
def batches():
    mixed, built_at, uniform_at = mixed_512()
    return {"sym": symmetric_256(), "mixed": mixed, "built_at": built_at, "uniform_at": uniform_at, "long": dominant(2304, seed=9106)}


@pytest.fixture(scope="module")
def direct_runs(tmp_path_factory, batches):
    """one process on the direct route: an R + n I batch first (a front launch that finds all of it not symmetric), then the cases"""
    steps = [{"a": flat(dominant(256, seed=9100))}] + [{"a": flat(batches[k]), "save": True} for k in ("sym", "mixed", "long")]
    runs = run_steps(tmp_path_factory.mktemp("direct"), "direct", steps)
    took(runs[0][0], "front")
    assert (runs[0][0]["not_symmetric"], runs[0][0]["last_batch"]) == (256, 256), runs[0][0]
    for rec, _, _, _ in runs[1:]:
        took(rec, "direct")
    return dict(zip(("sym", "mixed", "long"), runs[1:]))


@pytest.fixture(scope="module")
def front_runs(tmp_path_factory, batches):
    """a fresh process: the symmetric batch (front, nothing found), then the mixed one (front as well)"""
    steps = [{"a": flat(batches["sym"]), "save": True}, {"a": flat(batches["mixed"]), "save": True, "save_after": True}]
    runs = run_steps(tmp_path_factory.mktemp("front"), "front", steps)
    took(runs[0][0], "front")
    assert (runs[0][0]["not_symmetric"], runs[0][0]["last_batch"]) == (0, 256), runs[0][0]
    took(runs[1][0], "front")
    assert (runs[1][0]["not_symmetric"], runs[1][0]["last_batch"]) == (256, 512), runs[1][0]
    return {"sym": runs[0], "mixed": runs[1]}


def test_symmetric_batch_on_each_route(batches, front_runs, direct_runs):
    mats = batches["sym"]
    (frec, fx, finfo, _), (drec, dx, dinfo, _) = front_runs["sym"], direct_runs["sym"]
    assert np.array_equal(fx, dx) and np.array_equal(finfo, dinfo)
    assert not finfo.any()
    check_each(fx, mats, "symmetric, front route")
    x = fx.reshape(-1, N, N)
    assert np.array_equal(x, x.transpose(0, 2, 1))
    assert frec["rejects"] == 0 and drec["rejects"] == 0, (frec, drec)


def test_mixed_batch_with_rejects(batches, front_runs, direct_runs):
    mats = batches["mixed"]
    (frec, fx, finfo, after), (drec, dx, dinfo, _) = front_runs["mixed"], direct_runs["mixed"]
    assert np.array_equal(fx, dx) and np.array_equal(finfo, dinfo)
    assert not finfo.any(), finfo[finfo != 0]
    # the not-symmetric hand-overs are not rejects: the count is what the direct route hands to the pivoting kernel, no more
    print(f"rejects: front {frec['rejects']}, direct {drec['rejects']} (ten built, up to ten U(0,1))")
    assert frec["rejects"] == drec["rejects"], (frec, drec)
    assert len(batches["built_at"]) <= drec["rejects"] <= len(batches["built_at"]) + len(batches["uniform_at"])
    assert np.array_equal(after.view(np.uint64), flat(mats).view(np.uint64)), "the input buffer was written to"
    # the U(0,1) matrices are judged against the direct route only (their condition is whatever it is); everything else by the bound
    rest = np.setdiff1d(np.arange(len(mats)), batches["uniform_at"])
    check_each(fx.reshape(-1, N * N)[rest], mats[rest], "mixed, front route")


def test_not_symmetric_list_longer_than_the_second_grid(tmp_path, batches, direct_runs):
    mats = batches["long"]
    (rec, fx, finfo, _), = run_steps(tmp_path, "long", [{"a": flat(mats), "save": True}])
    took(rec, "front")
    assert (rec["not_symmetric"], rec["last_batch"]) == (2304, 2304), rec
    assert rec["rejects"] == 0, rec
    _, dx, dinfo, _ = direct_runs["long"]
    assert np.array_equal(fx, dx) and np.array_equal(finfo, dinfo)
    assert not finfo.any()
    some = np.arange(0, 2304, 36)
    assert len(some) == 64
    check_each(fx.reshape(-1, N * N)[some], mats[some], "2 304 x R + n I, front route")


def test_history_picks_the_route(tmp_path):
    sym = flat(as_mats(spd_batch(N, 64, seed=9107), N))
    gen = flat(dominant(64, seed=9108))
    steps = [{"a": sym, "keep": True}, {"a": gen}] + [{"a": sym, "same_as": 0} for _ in range(33)]
    recs = [r[0] for r in run_steps(tmp_path, "hint", steps)]
    took(recs[0], "front")
    assert (recs[0]["not_symmetric"], recs[0]["last_batch"]) == (0, 64)
    took(recs[1], "front")
    assert (recs[1]["not_symmetric"], recs[1]["last_batch"]) == (64, 64)
    for k in range(2, 33):  # 31 launches in the direct state: the count of the last front launch stands
        took(recs[k], "direct")
        assert (recs[k]["not_symmetric"], recs[k]["last_batch"]) == (64, 64), (k, recs[k])
    took(recs[33], "front")  # the 32nd probes, and finds a symmetric batch
    assert (recs[33]["not_symmetric"], recs[33]["last_batch"]) == (0, 64)
    took(recs[34], "front")  # ... which ends the direct state
    assert sum(r["front"] for r in recs) == 4 and sum(r["direct"] for r in recs) == 31
    assert all(r["same"] for r in recs[2:]), [k for k, r in enumerate(recs) if k >= 2 and not r["same"]]
    assert all(r["rejects"] == 0 for r in recs)


def test_device_table_entry_on_the_front_route(tmp_path):
    mats = np.empty((192, N, N))
    mats[0::2], mats[1::2] = as_mats(spd_batch(N, 96, seed=9109), N), dominant(96, seed=9110)
    a = flat(mats)
    (trec, tx, _, _), (crec, cx, cinfo, _) = run_steps(tmp_path, "table", [{"a": a, "table": True, "save": True}, {"a": a, "save": True}])
    took(trec, "front")
    assert (trec["not_symmetric"], trec["last_batch"]) == (96, 192), trec
    took(crec, "direct")  # half of the table launch was not symmetric
    assert np.array_equal(tx, cx)
    assert not cinfo.any()
    check_each(tx, mats, "device table, front route")
