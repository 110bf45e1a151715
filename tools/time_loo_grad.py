#!/usr/bin/env python3
"""Time the gradients of the batched GP leave-one-out log pseudo-likelihood (matinv_loo_grad_batched) against what a user had to do
before, in the same run and alternating with it: materialise M = B + diag c (not timed), matinv_inverse_batched(CHOLESKY) on it, then
torch for alpha = K d, kappa = diag K, beta = K (alpha / kappa), H = K diag(s) K, G and the contraction einsum("kij,kpij->kp", G, dM),
plus gradc from the diagonal and logpl. The LOO kernel itself (matinv_loo_batched, all three outputs) is timed alongside: the LOO-gradient
kernel runs its sweep, then about as many MFMAs again and NT times its panel stagings.

    python tools/time_loo_grad.py [--batch 100000] [--window 0.5] [--out DIR] [--quick]

Device events around back-to-back launches. All cases of a shape are warmed up first; then three rounds, each timing every case once
over a window of at least --window seconds (so the cases alternate); the median of a case's three windows is reported, with their
spread (max / min - 1) beside it. Rates are matrices per second. "HBM" is the fraction of 8 TB/s that the bytes the LOO-gradient kernel
must move would take at that rate: the lower 16 x 16 tiles of B and of the P derivative matrices plus c and d in, P + n + 1 elements
out. Prints a markdown table; writes loo_grad_times.json under --out.
"""
import argparse
import importlib
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
api = importlib.import_module("cuda-matrix-inversion_amd.api")

PEAK = 8e12
CASES = ("loo_grad", "inverse_torch", "loo")


def window_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def run_shape(n, nparam, dt, batch, window):
    f64 = dt == torch.float64
    code = api.F64 if f64 else api.F32
    esz = 8 if f64 else 4
    g = torch.Generator(device="cuda").manual_seed(n)
    b = torch.rand(batch * n * n, dtype=dt, device="cuda", generator=g)
    m = b.view(batch, n, n)
    m.add_(m.transpose(1, 2).clone())
    m.view(batch, n * n)[:, :: n + 1] += float(n)  # R + R^T + n I: SPD
    vc, vd = (torch.rand(batch * n, dtype=dt, device="cuda", generator=g) for _ in range(2))
    dm = torch.randn(batch * nparam * n * n, dtype=dt, device="cuda", generator=g)
    dmv = dm.view(batch * nparam, n, n)
    dmv.add_(dmv.transpose(1, 2).clone())  # symmetric, as the einsum of the old route needs it
    a = b.clone()  # M = B + diag c, materialised for the inverse
    a.view(batch, n * n)[:, :: n + 1] += vc.view(batch, n)
    inv = torch.empty_like(a)
    grad = torch.empty(batch * nparam, dtype=dt, device="cuda")
    gradc, mean, var = (torch.empty(batch * n, dtype=dt, device="cuda") for _ in range(3))
    logpl, logpl_loo = (torch.empty(batch, dtype=dt, device="cuda") for _ in range(2))
    info = torch.empty(batch, dtype=torch.int32, device="cuda")
    dm4 = dm.view(batch, nparam, n, n)

    def old_route():
        api.inverse_batched(a, n, api.ALGO_CHOLESKY, out=inv, info=info)
        k = inv.view(batch, n, n)
        al = torch.einsum("kij,kj->ki", k, vd.view(batch, n))
        kap = torch.diagonal(k, dim1=1, dim2=2)
        bb = al / kap
        be = torch.einsum("kij,kj->ki", k, bb)
        s = (1 + al * bb) / kap
        h = torch.matmul(k * s[:, None, :], k)
        ab = al[:, :, None] * be[:, None, :]
        gm = 0.5 * (ab + ab.transpose(1, 2)) - 0.5 * h
        lp = (0.5 * torch.log(kap) - 0.5 * al * bb).sum(dim=1) - 0.5 * n * math.log(2 * math.pi)
        return torch.einsum("kij,kpij->kp", gm, dm4), torch.diagonal(gm, dim1=1, dim2=2), lp

    fns = {
        "loo_grad": lambda: api.loo_grad_batched(n, b, vc, vd, dm, grad=grad, gradc=gradc, logpl=logpl, info=info),
        "inverse_torch": old_route,
        "loo": lambda: api.loo_batched(n, b, vc, vd, mean=mean, var=var, logpl=logpl_loo, info=info),
    }
    reps = {}
    for k, fn in fns.items():  # warm up every case of this shape, and size their windows
        fn()
        torch.cuda.synchronize()
        assert int(info.abs().sum()) == 0, k
        reps[k] = max(1, int(window * 1e3 / max(window_ms(fn, 3), 1e-3)))
    # the two routes compute the same thing
    want = old_route()[0].reshape(-1)
    scale = float(want.abs().max())
    assert float((grad - want).abs().max()) <= (1e-9 if f64 else 2e-3) * max(scale, 1.0), "the two routes disagree"
    ms = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            ms[k].append(window_ms(fn, reps[k]))
    nt = (n + 15) // 16
    lower = nt * (nt + 1) // 2 * 256
    nbytes = ((nparam + 1) * lower + 2 * n + nparam + n + 1) * esz
    kernels = {"loo_grad": api.loo_grad_kernel_name(code, n), "inverse_torch": api.kernel_name(api.ALGO_CHOLESKY, code, n) + " + torch",
               "loo": api.loo_kernel_name(code, n)}
    row = {"dtype": "f64" if f64 else "f32", "n": n, "nparam": nparam, "batch": batch}
    for k in fns:
        t = sorted(ms[k])
        row[k] = {"kernel": kernels[k], "ms": t[1], "windows_ms": ms[k], "spread": t[2] / t[0] - 1.0, "per_s": batch / t[1] * 1e3}
    row["loo_grad"]["hbm"] = batch * nbytes / (row["loo_grad"]["ms"] * 1e-3) / PEAK
    row["loo_grad_over_inverse_torch"] = row["loo_grad"]["per_s"] / row["inverse_torch"]["per_s"]
    row["loo_grad_over_loo"] = row["loo_grad"]["per_s"] / row["loo"]["per_s"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="64 x 64, P = 1 only, short windows (for profiling runs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_loo_grad.py needs a GPU"
    torch.cuda.set_device(0)
    shapes = [(n, p, dt) for dt in (torch.float64, torch.float32) for n in (16, 32, 64, 96) for p in (1, 4)]
    if args.quick:
        shapes, args.window = [(64, 1, torch.float64), (64, 1, torch.float32)], min(args.window, 0.05)
    print("| dtype | n | P | loo_grad /s | HBM | spread | inverse + torch /s | spread | loo_grad / old route | loo /s | loo_grad / loo |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    rows = []
    for n, p, dt in shapes:
        r = run_shape(n, p, dt, args.batch, args.window)
        rows.append(r)
        print(f"| {r['dtype']} | {n} | {p} | {r['loo_grad']['per_s']:.3e} | {r['loo_grad']['hbm']:.2f} | {100 * r['loo_grad']['spread']:.1f} % | "
              f"{r['inverse_torch']['per_s']:.3e} | {100 * r['inverse_torch']['spread']:.1f} % | {r['loo_grad_over_inverse_torch']:.2f} | "
              f"{r['loo']['per_s']:.3e} | {r['loo_grad_over_loo']:.2f} |", flush=True)
        if args.out:  # after every shape: a run that is cut short keeps what it measured
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "loo_grad_times.json"), "w") as f:
                json.dump(rows, f, indent=1)
    print()
    for r in rows:
        for k in CASES:
            print(f"{r['dtype']} n={r['n']:3d} P={r['nparam']} {k:15s} {r[k]['kernel']}")


if __name__ == "__main__":
    main()
