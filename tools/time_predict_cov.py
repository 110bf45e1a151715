#!/usr/bin/env python3
"""Time the joint predictive covariance between Q query points per matrix (matinv_predict_cov_batched) against the route a caller had
before, in the same run and alternating with it:
  inverse_torch: materialise M = B + diag c (not timed), matinv_inverse_batched(CHOLESKY) on it, then torch bmm for alpha = K d,
                 mean = A^T alpha and cov = E - A^T (K A).

    python tools/time_predict_cov.py [--batch 100000] [--window 0.5] [--out DIR] [--quick]

Device events around back-to-back launches. Both cases of a shape are warmed up first; then three rounds, each timing every case once over
a window of at least --window seconds (so the cases alternate); the median of a case's three windows is reported, with their spread
(max / min - 1) beside it. Rates are matrices per second (each with its Q means and Q x Q covariance). Prints a markdown table; writes
predict_cov_times.json under --out.
"""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
api = importlib.import_module("cuda-matrix-inversion_amd.api")

CASES = ("predict_cov", "inverse_torch")


def window_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def run_shape(n, nquery, dt, batch, window):
    f64 = dt == torch.float64
    code = api.F64 if f64 else api.F32
    g = torch.Generator(device="cuda").manual_seed(n)
    b = torch.rand(batch * n * n, dtype=dt, device="cuda", generator=g)
    m = b.view(batch, n, n)
    m.add_(m.transpose(1, 2).clone())
    m.view(batch, n * n)[:, :: n + 1] += float(n)  # R + R^T + n I: SPD
    vc, vd = (torch.rand(batch * n, dtype=dt, device="cuda", generator=g) for _ in range(2))
    va = torch.randn(batch * nquery * n, dtype=dt, device="cuda", generator=g)
    ve = torch.rand(batch * nquery * nquery, dtype=dt, device="cuda", generator=g)
    e3 = ve.view(batch, nquery, nquery)
    e3.add_(e3.transpose(1, 2).clone())  # symmetric, so that both routes read the same E
    ve.view(batch, nquery * nquery)[:, :: nquery + 1] += 2.0
    a = b.clone()  # M = B + diag c, materialised for the inverse
    a.view(batch, n * n)[:, :: n + 1] += vc.view(batch, n)
    inv = torch.empty_like(a)
    mean = torch.empty(batch * nquery, dtype=dt, device="cuda")
    cov = torch.empty(batch * nquery * nquery, dtype=dt, device="cuda")
    info = torch.empty(batch, dtype=torch.int32, device="cuda")
    a3 = va.view(batch, nquery, n)  # row i = a_i, i.e. A^T of the n x Q cross-covariance matrix
    a3t = a3.transpose(1, 2)

    def inverse_torch():
        api.inverse_batched(a, n, api.ALGO_CHOLESKY, out=inv, info=info)
        k = inv.view(batch, n, n)
        al = torch.bmm(k, vd.view(batch, n, 1))
        return torch.bmm(a3, al).view(batch, nquery), e3 - torch.bmm(a3, torch.bmm(k, a3t))

    fns = {
        "predict_cov": lambda: api.predict_cov_batched(n, b, vc, vd, va, ve, mean=mean, cov=cov, info=info),
        "inverse_torch": inverse_torch,
    }
    reps = {}
    for k, fn in fns.items():  # warm up every case of this shape, and size their windows
        fn()
        torch.cuda.synchronize()
        assert int(info.abs().sum()) == 0, k
        reps[k] = max(1, int(window * 1e3 / max(window_ms(fn, 2), 1e-3)))
    # the two routes compute the same thing (cov is symmetric, so its column-major packing is its row-major one)
    tol = 1e-9 if f64 else 2e-3
    wm, wc = inverse_torch()
    for got, want in ((mean.view(batch, nquery), wm), (cov.view(batch, nquery, nquery), wc)):
        assert float((got - want).abs().max()) <= tol * max(float(want.abs().max()), 1.0), "the routes disagree"
    del wm, wc
    ms = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            ms[k].append(window_ms(fn, reps[k]))
    kernels = {"predict_cov": api.predict_cov_kernel_name(code, n), "inverse_torch": api.kernel_name(api.ALGO_CHOLESKY, code, n) + " + torch"}
    row = {"dtype": "f64" if f64 else "f32", "n": n, "nquery": nquery, "batch": batch}
    for k in fns:
        t = sorted(ms[k])
        row[k] = {"kernel": kernels[k], "ms": t[1], "windows_ms": ms[k], "spread": t[2] / t[0] - 1.0, "per_s": batch / t[1] * 1e3}
    row["predict_cov_over_inverse_torch"] = row["predict_cov"]["per_s"] / row["inverse_torch"]["per_s"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="64 x 64, Q = 16 only, short windows (for profiling runs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_predict_cov.py needs a GPU"
    torch.cuda.set_device(0)
    shapes = [(n, q, dt) for dt in (torch.float64, torch.float32) for n in (16, 32, 64, 96) for q in (16, 64)]
    if args.quick:
        shapes, args.window = [(64, 16, torch.float64), (64, 16, torch.float32)], min(args.window, 0.05)
    print("| dtype | n | Q | predict_cov /s | spread | inverse + torch /s | spread | predict_cov / inverse + torch |")
    print("|---|---|---|---|---|---|---|---|")
    rows = []
    for n, q, dt in shapes:
        r = run_shape(n, q, dt, args.batch, args.window)
        rows.append(r)
        print(f"| {r['dtype']} | {n} | {q} | {r['predict_cov']['per_s']:.3e} | {100 * r['predict_cov']['spread']:.1f} % | "
              f"{r['inverse_torch']['per_s']:.3e} | {100 * r['inverse_torch']['spread']:.1f} % | "
              f"{r['predict_cov_over_inverse_torch']:.2f} |", flush=True)
        if args.out:  # after every shape: a run cut short keeps what it measured
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "predict_cov_times.json"), "w") as f:
                json.dump(rows, f, indent=1)
        torch.cuda.empty_cache()
    print()
    for r in rows:
        for k in CASES:
            print(f"{r['dtype']} n={r['n']:3d} Q={r['nquery']:2d} {k:14s} {r[k]['kernel']}")


if __name__ == "__main__":
    main()
