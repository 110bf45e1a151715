#!/usr/bin/env python3
"""Time the batched linear solve X = A^-1 B: the fused path (AUTO), the composed path (inverse + batched product, forced through
matinv_solve_batched_ex) and the inversion alone, on a batch of 100 000.

For 16 < n <= 64 the inverse's AUTO family is TILE, and matinv_solve_batched_ex(TILE) means the fused path, so the composed path
cannot be forced with that family: it is timed with TILEP (the MFMA pivoting inverse) instead, and "composed(AUTO inverse)" is
derived as inverse(AUTO) + [composed(TILEP) - inverse(TILEP)], i.e. the AUTO inverse plus the measured cost of the product step.

    python tools/time_solve.py [--batch 100000] [--window 0.5] [--out DIR] [--quick]

Device events around back-to-back launches; every case is warmed up, then timed over windows of at least --window seconds, the
median of 3 windows reported. Rates are matrices per second; "HBM" is the fraction of 8 TB/s that the algorithmic bytes
(solve: (n^2 + 2 n nrhs) sizeof(T); inverse: 2 n^2 sizeof(T)) per matrix would take at that rate. Prints a markdown table; writes solve_times.json under --out when given.
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


def timed(fn, window):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    reps = max(1, int(window * 1e3 / max(s.elapsed_time(e), 1e-3)))
    res = []
    for _ in range(3):
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        res.append(s.elapsed_time(e) / reps)
    return sorted(res)[1]


def inputs(n, nrhs, batch, dt, general):
    g = torch.Generator(device="cuda").manual_seed(n * 100 + nrhs)
    a = torch.rand(batch * n * n, dtype=dt, device="cuda", generator=g)
    if not general:
        m = a.view(batch, n, n)
        m.add_(m.transpose(1, 2).clone())
        m.view(batch, n * n)[:, :: n + 1] += float(n)  # R + R^T + n I: SPD
    b = torch.rand(batch * n * nrhs, dtype=dt, device="cuda", generator=g)
    return a, b


def run_case(n, nrhs, dt, batch, window, general=False):
    f64 = dt == torch.float64
    code = api.F64 if f64 else api.F32
    esz = 8 if f64 else 4
    a, b = inputs(n, nrhs, batch, dt, general)
    x = torch.empty_like(b)
    inv = torch.empty_like(a)
    info = torch.empty(batch, dtype=torch.int32, device="cuda")
    algo = api.ALGO_GAUSS_JORDAN
    auto = api.select_kernel(algo, code, n)
    family = api.KERNEL_TILEP if (general or auto == api.KERNEL_TILE) else auto
    row = {"dtype": "f64" if f64 else "f32", "n": n, "nrhs": nrhs, "input": "general" if general else "spd", "batch": batch,
           "fused_kernel": api.solve_kernel_name(algo, code, n, nrhs), "composed_family": family}
    t_f = timed(lambda: api.solve_batched(a, b, n, nrhs, algo, info=info, out=x), window)
    xf = x.clone()
    t_c = timed(lambda: api.solve_batched(a, b, n, nrhs, algo, info=info, out=x, kernel=family), window)
    t_i = timed(lambda: api.inverse_batched(a, n, algo, out=inv, info=info), window)
    t_if = timed(lambda: api.inverse_batched(a, n, algo, out=inv, info=info, kernel=family), window) if family != auto else t_i
    t_ca = t_i + (t_c - t_if)  # AUTO inverse + the product step
    sb = (n * n + 2 * n * nrhs) * esz
    ib = 2 * n * n * esz
    rate = lambda t: batch / t * 1e3  # noqa: E731
    row.update({
        "fused_ms": t_f, "composed_ms": t_c, "inverse_ms": t_i, "inverse_family_ms": t_if, "composed_auto_inverse_ms": t_ca,
        "fused_per_s": rate(t_f), "composed_per_s": rate(t_c), "composed_auto_inverse_per_s": rate(t_ca), "inverse_per_s": rate(t_i),
        "fused_hbm": batch * sb / (t_f * 1e-3) / PEAK, "composed_hbm": batch * sb / (t_c * 1e-3) / PEAK,
        "inverse_hbm": batch * ib / (t_i * 1e-3) / PEAK, "fused_over_composed": t_c / t_f, "fused_over_composed_auto": t_ca / t_f,
        "max_abs_diff_fused_composed": float((xf - x).abs().max()),
    })
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="one case only (for profiling runs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_solve.py needs a GPU"
    torch.cuda.set_device(0)
    cases = [(n, nrhs, dt, False) for dt in (torch.float64, torch.float32) for n in (16, 17, 32, 64) for nrhs in (1, 16)]
    cases += [(64, 1, torch.float64, True), (64, 16, torch.float64, True), (64, 1, torch.float32, True)]
    if args.quick:
        cases = [(64, 1, torch.float64, False), (64, 16, torch.float32, False), (64, 1, torch.float64, True)]
    rows = []
    hdr = ("| dtype | input | n | nrhs | fused kernel | fused /s | HBM | composed family | composed /s | composed (AUTO inverse) /s | "
           "inverse alone /s | HBM | fused / composed | fused / composed (AUTO inverse) |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    names = {v: k for k, v in vars(api).items() if k.startswith("KERNEL_")}
    print(hdr)
    for n, nrhs, dt, general in cases:
        r = run_case(n, nrhs, dt, args.batch, args.window, general)
        rows.append(r)
        print(f"| {r['dtype']} | {r['input']} | {n} | {nrhs} | `{r['fused_kernel']}` | {r['fused_per_s']:.3e} | {r['fused_hbm']:.2f} | "
              f"{names[r['composed_family']][7:]} | {r['composed_per_s']:.3e} | {r['composed_auto_inverse_per_s']:.3e} | "
              f"{r['inverse_per_s']:.3e} | {r['inverse_hbm']:.2f} | {r['fused_over_composed']:.2f} | {r['fused_over_composed_auto']:.2f} |",
              flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "solve_times.json"), "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
