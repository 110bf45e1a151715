#!/usr/bin/env python3
"""Time the batched whitening with Mahalanobis distances, log-determinant and Gaussian log-density (matinv_whiten_batched, all four
outputs) against the route a caller had before, in the same run and alternating with it:
  torch.linalg.cholesky on C, torch.linalg.solve_triangular for W = L^-1 (X - m), the square-sum for maha, 2 sum log diag L for the
  log-determinant and the log-density from the two;
and with matinv_colour_batched (Y = m + L Z and the factor) at the same (q, S) beside it as the yardstick: similar traffic, independent
MFMAs where the substitution has a dependent chain.

    python tools/time_whiten.py [--batch 100000] [--window 0.5] [--out DIR] [--quick]

The method is tools/time_sample.py's: device events around back-to-back launches; every case of a shape is warmed up first; then three
rounds, each timing every case once over a window of at least --window seconds (so the cases alternate); the median of a case's three
windows is reported, with their spread (max / min - 1) beside it. Rates are matrices per second (each with its S points). "HBM" is the
fraction of 8 TB/s that the bytes the whiten kernel must move amount to: q^2 / 2 + q + q S elements read, q S + 2 S + 1 written. Prints a
markdown table; writes whiten_times.json under --out.
"""
import argparse
import importlib
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_sample import agree, measure, spd  # noqa: E402

api = importlib.import_module("cuda-matrix-inversion_amd.api")
HBM_PEAK = 8e12


def run_whiten(q, npoint, dt, batch, window):
    f64 = dt == torch.float64
    g = torch.Generator(device="cuda").manual_seed(q)
    c = spd(batch, q, dt, g, q)
    vm = torch.rand(batch * q, dtype=dt, device="cuda", generator=g)
    vx = torch.randn(batch * npoint * q, dtype=dt, device="cuda", generator=g)
    w, y = torch.empty_like(vx), torch.empty_like(vx)
    maha, logpdf = (torch.empty(batch * npoint, dtype=dt, device="cuda") for _ in range(2))
    logdet = torch.empty(batch, dtype=dt, device="cuda")
    fac = torch.empty_like(c)
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    c3, x3 = c.view(batch, q, q), vx.view(batch, npoint, q).transpose(1, 2)  # x3[k] = X_k, q x S
    const = q * math.log(2 * math.pi)

    def torch_route():
        lo = torch.linalg.cholesky(c3)
        wt = torch.linalg.solve_triangular(lo, x3 - vm.view(batch, q, 1), upper=False)
        mh = (wt * wt).sum(dim=1)
        ld = 2 * torch.log(torch.diagonal(lo, dim1=1, dim2=2)).sum(dim=1)
        return wt, mh, ld, -0.5 * (mh + ld[:, None] + const)

    fns = {"whiten": lambda: api.whiten_batched(q, c, vm, vx, W=w, maha=maha, logdet=logdet, logpdf=logpdf, info=info),
           "torch": torch_route,
           "colour": lambda: api.colour_batched(q, c, vm, vx, Y=y, L=fac, info=info)}
    row = {"dtype": "f64" if f64 else "f32", "q": q, "npoint": npoint, "batch": batch}
    res = measure(fns, info, window)
    wt, mh, ld, lp = torch_route()
    agree(w.view(batch, npoint, q).transpose(1, 2), wt, f64, "W")
    agree(maha.view(batch, npoint), mh, f64, "maha")
    agree(logdet, ld, f64, "logdet")
    agree(logpdf.view(batch, npoint), lp, f64, "logpdf")
    del wt, mh, ld, lp
    code = api.F64 if f64 else api.F32
    kernels = {"whiten": api.whiten_kernel_name(code, q), "colour": api.colour_kernel_name(code, q),
               "torch": "torch.linalg.cholesky + solve_triangular + square-sum + 2 log diag"}
    for k in fns:
        row[k] = dict(res[k], kernel=kernels[k], per_s=batch / res[k]["ms"] * 1e3)
    nbytes = (q * q / 2 + q + q * npoint + q * npoint + 2 * npoint + 1) * (8 if f64 else 4)
    row["hbm_bytes_per_matrix"] = nbytes
    row["hbm_frac"] = nbytes * row["whiten"]["per_s"] / HBM_PEAK
    row["ours_over_torch"] = row["whiten"]["per_s"] / row["torch"]["per_s"]
    row["ours_over_colour"] = row["whiten"]["per_s"] / row["colour"]["per_s"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="q = 64, S = 16 only, short windows (for profiling runs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_whiten.py needs a GPU"
    torch.cuda.set_device(0)
    dts = (torch.float64, torch.float32)
    shapes = [(q, s, dt) for dt in dts for q in (16, 32, 64, 96) for s in (16, 64)]
    if args.quick:
        shapes, args.window = [(64, 16, dt) for dt in dts], min(args.window, 0.05)
    print("| dtype | q | S | whiten /s | spread | HBM | torch route /s | spread | whiten / torch route | colour /s | spread | whiten / colour |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    rows = []
    for shape in shapes:
        r = run_whiten(*shape, args.batch, args.window)
        rows.append(r)
        print(f"| {r['dtype']} | {r['q']} | {r['npoint']} | {r['whiten']['per_s']:.3e} | {100 * r['whiten']['spread']:.1f} % | "
              f"{r['hbm_frac']:.2f} | {r['torch']['per_s']:.3e} | {100 * r['torch']['spread']:.1f} % | {r['ours_over_torch']:.2f} | "
              f"{r['colour']['per_s']:.3e} | {100 * r['colour']['spread']:.1f} % | {r['ours_over_colour']:.2f} |", flush=True)
        if args.out:  # after every shape: a run cut short keeps what it measured
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "whiten_times.json"), "w") as f:
                json.dump(rows, f, indent=1)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
