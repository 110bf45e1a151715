#!/usr/bin/env python3
"""Time the multi-output GP solves (matinv_multi_target_batched; alpha, logml and mean requested) against the two routes a caller had
before, in the same run and alternating with them:
  D calls:  D x (logml_batched + logml_grad_batched(want=("alpha",)) + predict_batched(want=("mean",))), one target vector each, which
            factorises the same matrix 3 D times;
  torch:    torch.linalg.cholesky on M, torch.cholesky_solve for alpha = M^-1 Y, torch.bmm for mean = A alpha, the dot products for quad
            and 2 sum log diag L for the log-determinant.

    python tools/time_multi_target.py [--batch 100000] [--window 0.5] [--out DIR] [--quick]

The method is tools/time_whiten.py's: device events around back-to-back launches; every case of a shape is warmed up first; then three
rounds, each timing every case once over a window of at least --window seconds (so the cases alternate); the median of a case's three
windows is reported, with their spread (max / min - 1) beside it. Rates are matrices per second (each with its D targets and Q queries).
"HBM" is the fraction of 8 TB/s that the bytes the multi-target kernel must move amount to: n^2 / 2 + n + D n + ceil(D / 16) Q n elements
read, D n + 2 D + 1 + D Q written (of which this request stores D n + D + D Q). Prints a markdown table; writes multi_target_times.json
under --out.
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


def run_multi_target(n, D, Q, dt, batch, window):
    f64 = dt == torch.float64
    g = torch.Generator(device="cuda").manual_seed(n)
    b = spd(batch, n, dt, g, n)
    vc = torch.rand(batch * n, dtype=dt, device="cuda", generator=g)
    vy = torch.randn(batch * D * n, dtype=dt, device="cuda", generator=g)
    va = torch.randn(batch * Q * n, dtype=dt, device="cuda", generator=g)
    alpha = torch.empty_like(vy)
    logml = torch.empty(batch * D, dtype=dt, device="cuda")
    mean = torch.empty(batch * D * Q, dtype=dt, device="cuda")
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    # the D-call route: target t of every matrix packed on its own, outputs per target
    yt = [vy.view(batch, D, n)[:, t].contiguous().view(-1) for t in range(D)]
    a1, l1, m1 = torch.empty(batch * n, dtype=dt, device="cuda"), torch.empty(batch, dtype=dt, device="cuda"), \
        torch.empty(batch * Q, dtype=dt, device="cuda")
    m3 = b.view(batch, n, n) + torch.diag_embed(vc.view(batch, n))
    y3, a3 = vy.view(batch, D, n).transpose(1, 2), va.view(batch, Q, n)  # y3[k] = Y_k, n x D; a3[k] = A_k, Q x n
    const = n * math.log(2 * math.pi)

    def d_calls():
        for t in range(D):
            api.logml_batched(n, b, vc, yt[t], out=l1, info=info)
            api.logml_grad_batched(n, b, vc, yt[t], None, alpha=a1, info=info, want=())
            api.predict_batched(n, b, vc, yt[t], va, None, mean=m1, info=info, want=())

    def torch_route():
        lo = torch.linalg.cholesky(m3)
        al = torch.cholesky_solve(y3, lo)
        ld = 2 * torch.log(torch.diagonal(lo, dim1=1, dim2=2)).sum(dim=1)
        quad = (y3 * al).sum(dim=1)
        return al, -0.5 * (quad + ld[:, None] + const), torch.bmm(a3, al)

    fns = {"multi_target": lambda: api.multi_target_batched(n, b, vc, vy, va, alpha=alpha, logml=logml, mean=mean, info=info, want=()),
           "d_calls": d_calls, "torch": torch_route}
    row = {"dtype": "f64" if f64 else "f32", "n": n, "ntarget": D, "nquery": Q, "batch": batch}
    res = measure(fns, info, window)
    al, lm, mn = torch_route()
    agree(alpha.view(batch, D, n).transpose(1, 2), al, f64, "alpha")
    agree(logml.view(batch, D), lm, f64, "logml")
    agree(mean.view(batch, D, Q).transpose(1, 2), mn, f64, "mean")
    del al, lm, mn
    code = api.F64 if f64 else api.F32
    kernels = {"multi_target": api.multi_target_kernel_name(code, n),
               "d_calls": f"{D} x ({api.logml_kernel_name(code, n)} + {api.logml_grad_kernel_name(code, n)} + {api.predict_kernel_name(code, n)})",
               "torch": "torch.linalg.cholesky + cholesky_solve + bmm + 2 log diag"}
    for k in fns:
        row[k] = dict(res[k], kernel=kernels[k], per_s=batch / res[k]["ms"] * 1e3)
    groups = (D + 15) // 16
    nbytes = (n * n / 2 + n + D * n + groups * Q * n + D * n + 2 * D + 1 + D * Q) * (8 if f64 else 4)
    row["hbm_bytes_per_matrix"] = nbytes
    row["hbm_frac"] = nbytes * row["multi_target"]["per_s"] / HBM_PEAK
    row["ours_over_d_calls"] = row["multi_target"]["per_s"] / row["d_calls"]["per_s"]
    row["ours_over_torch"] = row["multi_target"]["per_s"] / row["torch"]["per_s"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="n = 64, (D, Q) = (16, 16) only, short windows (for profiling runs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_multi_target.py needs a GPU"
    torch.cuda.set_device(0)
    dts = (torch.float64, torch.float32)
    shapes = [(n, D, Q, dt) for dt in dts for n in (16, 32, 64, 96) for D, Q in ((4, 16), (16, 16), (16, 64))]
    if args.quick:
        shapes, args.window = [(64, 16, 16, dt) for dt in dts], min(args.window, 0.05)
    print("| dtype | n | D | Q | multi-target /s | spread | HBM | D calls /s | spread | multi-target / D calls | torch route /s | spread | "
          "multi-target / torch route |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    rows = []
    for shape in shapes:
        r = run_multi_target(*shape, args.batch, args.window)
        rows.append(r)
        print(f"| {r['dtype']} | {r['n']} | {r['ntarget']} | {r['nquery']} | {r['multi_target']['per_s']:.3e} | "
              f"{100 * r['multi_target']['spread']:.1f} % | {r['hbm_frac']:.2f} | {r['d_calls']['per_s']:.3e} | "
              f"{100 * r['d_calls']['spread']:.1f} % | {r['ours_over_d_calls']:.2f} | {r['torch']['per_s']:.3e} | "
              f"{100 * r['torch']['spread']:.1f} % | {r['ours_over_torch']:.2f} |", flush=True)
        if args.out:  # after every shape: a run cut short keeps what it measured
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "multi_target_times.json"), "w") as f:
                json.dump(rows, f, indent=1)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
