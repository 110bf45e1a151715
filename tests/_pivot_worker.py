"""Worker of tests/test_gpu_pivot_search.py: the lists of tests/_pivot_cases.py (one dominant pivot candidate per step, at a chosen row)
on the GPU, ONE process per (mode, dtype, group of sizes) under MATINV_DEBUG_REJECTS=1 (the library reads its switches once per process;
MATINV_TILE_SCREEN=0 or 1 is set by the caller).

  all <dtype> <n> ...    per size: `auto` below, then the same list under matinv_set_gj_policy(PIVOT) and with kernel= TILEP, ROW, LDS,
                         GLOBAL, BLOCKED wherever matinv_kernel_name is non-empty, then the log-determinant (AUTO / ROW / GLOBAL where
                         matinv_logdet_kernel_name is non-empty) of the whole list: sign exactly parity(pi) prod sign(D), logabsdet
                         within the bound of tests/test_gpu_logdet.py against numpy.linalg.slogdet in float64, info 0.
  auto <dtype> <n> ...   inverse_batched on the AUTO route, the list without its identity members: info 0, every inverse within the bound
                         (the elementwise measure in both dtypes: max(1e-10, 1e-15 cond n), 1e-5 cond), the input bitwise untouched; where
                         a natural-order kernel serves n the reject counter grows by exactly the batch (the pivoting kernel produced the
                         bits) and the identity members alone leave it at 0. Prints `BITS ...` lines (count and a digest of the output
                         bits) that the test compares between the unscreened and the screened run.
  front                  64 x 64 fp64 as the first launches of the process: no member is symmetric, so the first call runs the
                         symmetric-only kernel in front and finds the whole batch not symmetric, the second call takes the direct route
                         (matinv_sym_front_stats); same bits, same info, same counter.
  solve <dtype>          matinv_solve_batched, Gauss-Jordan, n = 17, 33, 64: the fused route with nrhs 1 and 16, the same under the PIVOT
                         policy (the row solve), the composed route with nrhs 17; X within the bound of tests/test_gpu_solve.py against
                         numpy.linalg.solve in float64; without the policy the counter equals inverse_batched's on the same list.

Prints err / bound per size and kernel name. Exits non-zero at the first failure and starts nothing after it."""
import hashlib
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import _pivot_cases as P  # noqa: E402

GROUPS = {
    "f64": {"small": (2, 8, 9, 16, 17, 25), "onewave": (26, 32, 33, 48, 49, 64), "multiwave": (65, 80, 97, 112, 128),
            "wide": (129, 144, 192), "forced": (100, 159, 160)},
    "f32": {"small": (2, 8, 9, 16, 17, 25), "onewave": (26, 32, 33, 48, 49, 64), "multiwave": (65, 80, 81, 96, 97, 112, 113, 128),
            "wide": (129, 144, 256), "forced": (100, 159, 160)},
}
SOLVE_SIZES = (17, 33, 64)
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}


def main(argv):
    import torch
    api = importlib.import_module("cuda-matrix-inversion_amd.api")
    assert os.environ.get("MATINV_DEBUG_REJECTS") == "1"
    assert os.environ.get("MATINV_GJ_POLICY") in (None, "", "natural"), "the counts are the default policy's"
    assert torch.cuda.is_available()
    mode = argv[0]
    GJ = api.ALGO_GAUSS_JORDAN
    FAMILIES = (("tilep", api.KERNEL_TILEP), ("row", api.KERNEL_ROW), ("lds", api.KERNEL_LDS), ("global", api.KERNEL_GLOBAL),
                ("blocked", api.KERNEL_BLOCKED))

    def fail(msg):
        print("FAIL " + msg, flush=True)
        sys.exit(1)

    def invert(flat, n, kernel=api.KERNEL_AUTO):
        """one inverse_batched call: (outputs [B, n*n] numpy, info, growth of the reject counter); the input must come back untouched"""
        batch = len(flat)
        d = torch.from_numpy(np.ascontiguousarray(flat).reshape(-1)).cuda()
        info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
        api.debug_rejects(reset=True)
        x = api.inverse_batched(d, n, GJ, info=info, batch=batch, kernel=kernel)
        torch.cuda.synchronize()
        if d.cpu().numpy().tobytes() != np.ascontiguousarray(flat).tobytes():
            fail(f"n={n} kernel {kernel}: the input was written to")
        return x.cpu().numpy().reshape(batch, -1), info.cpu().numpy(), api.debug_rejects(reset=True)

    def solve(flat, b, n, nrhs):
        batch = len(flat)
        d = torch.from_numpy(np.ascontiguousarray(flat).reshape(-1)).cuda()
        db = torch.from_numpy(np.ascontiguousarray(b).reshape(-1)).cuda()
        info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
        api.debug_rejects(reset=True)
        x = api.solve_batched(d, db, n, nrhs, GJ, info=info, batch=batch)
        torch.cuda.synchronize()
        return x.cpu().numpy().reshape(batch, -1), info.cpu().numpy(), api.debug_rejects(reset=True)

    def check_inverse(what, dtype, n, cs, got, info, want, cond):
        """info 0 and every matrix within the bound; returns the largest err / bound. want [B, n, n] indexed [row, col]"""
        if info.any():
            k = int(np.flatnonzero(info)[0])
            fail(f"{what}: info {info[info != 0][:8].tolist()}, first at {P.case_text(n, cs[k])}")
        ratio = P.elementwise(got.reshape(len(got), n, n).transpose(0, 2, 1), want) / P.bound(dtype, cond, n)
        if not (ratio < 1.0).all():
            k = int(np.nanargmax(np.where(np.isnan(ratio), np.inf, ratio)))
            fail(f"{what}: err / bound {ratio[k]:.3g} at {P.case_text(n, cs[k])} ({int((~(ratio < 1.0)).sum())} of {len(ratio)} beyond the bound)")
        print(f"{what}: {len(got)} matrices, largest err / bound {ratio.max():.3g} ok", flush=True)
        return float(ratio.max())

    def auto(dtype, n):
        code = api.F64 if dtype == "f64" else api.F32
        mats, flat, _, _, ident = P.matrices(dtype, n)
        cs = P.cases(n)
        want, cond = P.reference(mats)
        name = api.kernel_name(GJ, code, n, api.KERNEL_AUTO)
        natural = any(part in name for part in ("gj_rowlane2<", "gj_tile_f", "gj_tile4_f"))
        for call, sel in (("pivoted", ~ident), ("identity", ident)):
            idx = np.flatnonzero(sel)
            got, info, count = invert(flat[idx], n)
            what = f"auto {dtype} n={n} {name} {call}"
            check_inverse(what, dtype, n, [cs[k] for k in idx], got, info, want[idx], cond[idx])
            expect = len(idx) if call == "pivoted" else 0
            print(f"{what}: rejects {count}" + (f" (expected {expect})" if natural else ""), flush=True)
            if natural and count != expect:
                fail(f"{what}: the reject counter grew by {count}, expected {expect}")
            print(f"BITS {dtype} {n} {call} {count} {hashlib.sha256(got.tobytes() + info.tobytes()).hexdigest()}", flush=True)

    def forced(dtype, n):
        code = api.F64 if dtype == "f64" else api.F32
        mats, flat, _, _, ident = P.matrices(dtype, n)
        keep = np.flatnonzero(~ident)
        cs = [P.cases(n)[k] for k in keep]
        want, cond = P.reference(mats[keep])
        old = api.set_gj_policy(api.GJ_PIVOT)
        try:
            name = api.kernel_name(GJ, code, n, api.KERNEL_AUTO)
            got, info, _ = invert(flat[keep], n)
        finally:
            api.set_gj_policy(old)
        check_inverse(f"policy-pivot {dtype} n={n} {name}", dtype, n, cs, got, info, want, cond)
        for fam, kernel in FAMILIES:
            name = api.kernel_name(GJ, code, n, kernel)
            if name:
                got, info, _ = invert(flat[keep], n, kernel)
                check_inverse(f"{fam} {dtype} n={n} {name}", dtype, n, cs, got, info, want, cond)

    def logdet(dtype, n):
        code = api.F64 if dtype == "f64" else api.F32
        mats, flat, _, sign, _ = P.matrices(dtype, n)
        cs = P.cases(n)
        a64 = np.asarray(mats, dtype=np.float64)
        wsign, wld = np.linalg.slogdet(a64)
        assert np.array_equal(wsign, sign)
        tol = n * n * U[dtype] * np.linalg.cond(a64) + n * U[dtype] * np.maximum(1.0, np.abs(wld))  # tests/test_gpu_logdet.py: bound
        for fam, kernel in (("auto", api.KERNEL_AUTO), ("row", api.KERNEL_ROW), ("global", api.KERNEL_GLOBAL)):
            name = api.logdet_kernel_name(GJ, code, n, kernel)
            if not name:
                continue
            d = torch.from_numpy(np.ascontiguousarray(flat).reshape(-1)).cuda()
            info = torch.full((len(flat),), -7, dtype=torch.int32, device="cuda")
            s, ld = api.logdet_batched(d, n, GJ, info=info, kernel=kernel, batch=len(flat))
            torch.cuda.synchronize()
            s, ld, info = s.cpu().numpy().astype(np.float64), ld.cpu().numpy().astype(np.float64), info.cpu().numpy()
            what = f"logdet-{fam} {dtype} n={n} {name}"
            if info.any():
                fail(f"{what}: info {info[info != 0][:8].tolist()}")
            if not np.array_equal(s, sign):
                bad = np.flatnonzero(s != sign)
                fail(f"{what}: wrong sign for {len(bad)} of {len(s)}, first {[P.case_text(n, cs[k]) for k in bad[:8]]}")
            ratio = np.abs(ld - wld) / tol
            if not (ratio <= 1.0).all():
                k = int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio)))
                fail(f"{what}: err / bound {ratio[k]:.3g} at {P.case_text(n, cs[k])}")
            print(f"{what}: {len(s)} signs exact, largest err / bound {ratio.max():.3g} ok", flush=True)

    if mode in ("all", "auto"):
        dtype = argv[1]
        for n in [int(v) for v in argv[2:]]:
            auto(dtype, n)
            if mode == "all":
                forced(dtype, n)
                logdet(dtype, n)
    elif mode == "front":
        n, dtype = 64, "f64"
        mats, flat, _, _, ident = P.matrices(dtype, n)
        if any(np.array_equal(m, m.T) for m in mats):
            fail("front: a member of the list is symmetric")
        keep = np.flatnonzero(~ident)
        cs = [P.cases(n)[k] for k in keep]
        want, cond = P.reference(mats[keep])
        runs, st = [], [api.sym_front_stats()]
        for call in ("first", "second"):
            runs.append(invert(flat[keep], n))
            st.append(api.sym_front_stats())
            print(f"front {call}: rejects {runs[-1][2]} stats {st[-1]}", flush=True)
            check_inverse(f"front {call} {dtype} n={n}", dtype, n, cs, runs[-1][0], runs[-1][1], want, cond)
        if (st[1]["front_launches"], st[1]["direct_launches"]) != (st[0]["front_launches"] + 1, st[0]["direct_launches"]):
            fail(f"front: the first call was not a front launch: {st[0]} -> {st[1]}")
        if (st[1]["last_not_symmetric"], st[1]["last_batch"]) != (len(keep), len(keep)):
            fail(f"front: the front kernel found {st[1]['last_not_symmetric']} of {st[1]['last_batch']} not symmetric, expected all")
        if (st[2]["front_launches"], st[2]["direct_launches"]) != (st[1]["front_launches"], st[1]["direct_launches"] + 1):
            fail(f"front: the second call did not take the direct route: {st[1]} -> {st[2]}")
        if not (np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2] == len(keep)):
            fail(f"front: the two routes differ (rejects {runs[0][2]} and {runs[1][2]}, batch {len(keep)})")
        print(f"front: {len(keep)} matrices, the same bits and {runs[0][2]} rejects on both routes ok", flush=True)
    elif mode == "solve":
        dtype = argv[1]
        code = api.F64 if dtype == "f64" else api.F32
        for n in SOLVE_SIZES:
            mats, flat, _, _, ident = P.matrices(dtype, n)
            keep = np.flatnonzero(~ident)
            cs = [P.cases(n)[k] for k in keep]
            flat, a64 = flat[keep], np.asarray(mats[keep], dtype=np.float64)
            cond = np.linalg.cond(a64)
            icount = invert(flat, n)[2]
            if icount != len(keep):
                fail(f"solve {dtype} n={n}: inverse_batched counted {icount} rejects on a batch of {len(keep)}")
            for nrhs, policy, prefix in ((1, None, "matinv_solve_tile_"), (16, None, "matinv_solve_tile_"), (1, api.GJ_PIVOT, "matinv_solve_row<"),
                                         (16, api.GJ_PIVOT, "matinv_solve_row<"), (17, None, "matinv_gj_")):
                b = np.random.default_rng([n, nrhs]).standard_normal((len(flat), n * nrhs)).astype(P.NP_DTYPES[dtype])
                old = api.set_gj_policy(policy) if policy is not None else None
                try:
                    name = api.solve_kernel_name(GJ, code, n, nrhs, api.KERNEL_AUTO)
                    x, info, count = solve(flat, b, n, nrhs)
                finally:
                    if old is not None:
                        api.set_gj_policy(old)
                what = f"solve {dtype} n={n} nrhs={nrhs}{' policy-pivot' if policy is not None else ''} {name}"
                if not name.startswith(prefix):
                    fail(f"{what}: expected a kernel named {prefix}...")
                if info.any():
                    fail(f"{what}: info {info[info != 0][:8].tolist()}")
                if policy is None and count != icount:
                    fail(f"{what}: {count} rejects, inverse_batched on the same list {icount}")
                bs = b.astype(np.float64).reshape(len(flat), nrhs, n).transpose(0, 2, 1)
                want = np.linalg.solve(a64, bs)
                got = x.astype(np.float64).reshape(len(flat), nrhs, n).transpose(0, 2, 1)
                worst = 0.0
                for k in range(len(flat)):  # tests/test_gpu_solve.py check_close
                    if dtype == "f64":
                        floor = 1e-3 * np.abs(want[k]).max()
                        err, tol = (np.abs(got[k] - want[k]) / np.maximum(np.abs(want[k]), floor)).max(), max(1e-10, 1e-15 * cond[k] * n)
                    else:
                        err, tol = np.linalg.norm(got[k] - want[k]) / np.linalg.norm(want[k]), 1e-5 * cond[k]
                    worst = max(worst, err / tol)
                    if not err < tol:
                        fail(f"{what}: err {err:.3g} bound {tol:.3g} at {P.case_text(n, cs[k])}")
                print(f"{what}: {len(flat)} systems, rejects {count}, largest err / bound {worst:.3g} ok", flush=True)
    else:
        fail(f"unknown mode {mode!r}")
    print("pivot-worker ok", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
