#!/usr/bin/env python3
"""Time the batched leave-one-out cross-validation (matinv_loo_batched) against a kernel this feature did not touch, in the same run
and alternating with it: matinv_inverse_batched(CHOLESKY) on the materialised M = B + diag c at the same sizes -- the first step of
what a user had to do before (inverse, read the diagonal, batched mat-vec).

    python tools/time_loo.py [--batch 100000] [--window 0.5] [--out DIR] [--quick]

Device events around back-to-back launches. Both cases of a shape are warmed up first; then three rounds, each timing every case once
over a window of at least --window seconds (so the cases alternate); the median of a case's three windows is reported, with their
spread (max / min - 1) beside it. Rates are matrices per second. "HBM" is the fraction of 8 TB/s that the bytes the kernel must move
would take at that rate: the lower 16 x 16 tiles of B plus c and d in and 2 n + 1 elements out for LOO, A in and A^-1 out for the
inverse. Prints a markdown table; writes loo_times.json under --out.
"""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
api = importlib.import_module("cuda-matrix-inversion_amd.api")

PEAK = 8e12
CASES = ("loo", "inverse_chol")


def window_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def run_shape(n, dt, batch, window):
    f64 = dt == torch.float64
    code = api.F64 if f64 else api.F32
    esz = 8 if f64 else 4
    g = torch.Generator(device="cuda").manual_seed(n)
    b = torch.rand(batch * n * n, dtype=dt, device="cuda", generator=g)
    m = b.view(batch, n, n)
    m.add_(m.transpose(1, 2).clone())
    m.view(batch, n * n)[:, :: n + 1] += float(n)  # R + R^T + n I: SPD
    vc, vd = (torch.rand(batch * n, dtype=dt, device="cuda", generator=g) for _ in range(2))
    a = b.clone()  # M = B + diag c, materialised for the inverse
    a.view(batch, n * n)[:, :: n + 1] += vc.view(batch, n)
    inv = torch.empty_like(a)
    mean, var = (torch.empty(batch * n, dtype=dt, device="cuda") for _ in range(2))
    logpl = torch.empty(batch, dtype=dt, device="cuda")
    info = torch.empty(batch, dtype=torch.int32, device="cuda")
    fns = {
        "loo": lambda: api.loo_batched(n, b, vc, vd, mean=mean, var=var, logpl=logpl, info=info),
        "inverse_chol": lambda: api.inverse_batched(a, n, api.ALGO_CHOLESKY, out=inv, info=info),
    }
    reps = {}
    for k, fn in fns.items():  # warm up both cases of this shape, and size their windows
        fn()
        torch.cuda.synchronize()
        assert int(info.abs().sum()) == 0, k
        reps[k] = max(1, int(window * 1e3 / max(window_ms(fn, 3), 1e-3)))
    ms = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            ms[k].append(window_ms(fn, reps[k]))
    nt = (n + 15) // 16
    lower = nt * (nt + 1) // 2 * 256
    nbytes = {"loo": (lower + 2 * n + 2 * n + 1) * esz, "inverse_chol": 2 * n * n * esz}
    kernels = {"loo": api.loo_kernel_name(code, n), "inverse_chol": api.kernel_name(api.ALGO_CHOLESKY, code, n)}
    row = {"dtype": "f64" if f64 else "f32", "n": n, "batch": batch}
    for k in fns:
        t = sorted(ms[k])
        row[k] = {"kernel": kernels[k], "ms": t[1], "windows_ms": ms[k], "spread": t[2] / t[0] - 1.0, "per_s": batch / t[1] * 1e3,
                  "hbm": batch * nbytes[k] / (t[1] * 1e-3) / PEAK}
    row["loo_over_inverse_chol"] = row["loo"]["per_s"] / row["inverse_chol"]["per_s"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="64 x 64 only, short windows (for profiling runs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_loo.py needs a GPU"
    torch.cuda.set_device(0)
    shapes = [(n, dt) for dt in (torch.float64, torch.float32) for n in (16, 32, 64, 96)]
    if args.quick:
        shapes, args.window = [(64, torch.float64), (64, torch.float32)], min(args.window, 0.05)
    print("| dtype | n | " + " | ".join(f"{k} /s | HBM | spread" for k in CASES) + " | loo / inverse(CHOL) |")
    print("|---|---|" + "---|" * (3 * len(CASES) + 1))
    rows = []
    for n, dt in shapes:
        r = run_shape(n, dt, args.batch, args.window)
        rows.append(r)
        cells = " | ".join(f"{r[k]['per_s']:.3e} | {r[k]['hbm']:.2f} | {100 * r[k]['spread']:.1f} %" for k in CASES)
        print(f"| {r['dtype']} | {n} | {cells} | {r['loo_over_inverse_chol']:.2f} |", flush=True)
    print()
    for r in rows:
        for k in CASES:
            print(f"{r['dtype']} n={r['n']:3d} {k:13s} {r[k]['kernel']}")
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "loo_times.json"), "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
