#!/usr/bin/env python3
"""Time the leave-one-out cross-validation of the trend GP (matinv_trend_loo_batched; mean, var and logpl requested) against the two routes
a caller had before, in the same run and alternating with them:
  trend_grad: trend_grad_batched with gradc and alpha and nparam = 0, then in torch P_ii = (sum_t alpha_ti^2 - 2 gradc_i) / D (a
              cancelling difference) and the three outputs by elementwise operations and one sum;
  inverse:    inverse_batched on M for Kinv, then in torch Kinv [H | Y], A = H^T Kinv H, its Cholesky factor, U = Kinv H L_A^-T,
              P_ii = Kinv_ii - sum_b U_ib^2, alpha = Kinv Y - U U^T Y and the same elementwise operations.

    python tools/time_trend_loo.py [--batch 100000] [--window 0.5] [--out DIR] [--quick]

The method is tools/time_trend_grad.py's: device events around back-to-back launches; every case of a shape is
warmed up first; then three rounds, each timing every case once over a window of at least --window seconds (so the cases alternate); the
median of a case's three windows is reported, with their spread (max / min - 1) beside it. Rates are matrices per second (each with its K
basis vectors and D targets). "HBM" is the fraction of 8 TB/s that the bytes the kernel must move amount to: n^2 / 2 + n + K n + D n
elements read, n + D n + D written. n = 130 runs the global form (one workgroup per matrix, written to be correct, not fast) on a fiftieth
of the batch, and K is held to n / 2 (n = 16 runs K = 8). Ours must agree with both routes. Prints a markdown table; writes
trend_loo_times.json under --out.
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


def run_trend_loo(n, K, D, dt, batch, window):
    f64 = dt == torch.float64
    K = min(K, n // 2)  # as tools/time_trend_grad.py: with K near n the projection P vanishes
    g = torch.Generator(device="cuda").manual_seed(n)
    b = spd(batch, n, dt, g, n)
    vc = torch.rand(batch * n, dtype=dt, device="cuda", generator=g)
    vh = torch.randn(batch * K * n, dtype=dt, device="cuda", generator=g)
    vh.view(batch, K, n)[:, 0] = 1.0
    vy = torch.randn(batch * D * n, dtype=dt, device="cuda", generator=g)
    mean, var, logpl = torch.empty_like(vy), torch.empty_like(vc), torch.empty(batch * D, dtype=dt, device="cuda")
    gradc, alpha = torch.empty_like(vc), torch.empty_like(vy)
    kinv = torch.empty(batch * n * n, dtype=dt, device="cuda")
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    mflat = (b.view(batch, n, n) + torch.diag_embed(vc.view(batch, n))).reshape(-1)
    h3 = vh.view(batch, K, n).transpose(1, 2)  # h3[k] = H_k, n x K
    y3 = vy.view(batch, D, n)
    hy3 = torch.cat([h3, y3.transpose(1, 2)], dim=2).contiguous()
    const = 0.5 * n * math.log(2 * math.pi)

    def outputs(pd, al):
        """(mean, var, logpl) from P_ii (batch x n) and alpha (batch x D x n)"""
        rp = 1.0 / pd
        w = al * rp[:, None, :]
        return y3 - w, rp, (0.5 * torch.log(pd)[:, None, :] - 0.5 * al * w).sum(dim=2) - const

    def grad_route():
        api.trend_grad_batched(n, b, vc, vh, vy, None, gradc=gradc, alpha=alpha, info=info, want=(), nbasis=K, nparam=0)
        al = alpha.view(batch, D, n)
        return outputs(((al * al).sum(dim=1) - 2 * gradc.view(batch, n)) / D, al)

    def inverse_route():
        api.inverse_batched(mflat, n, api.ALGO_CHOLESKY, out=kinv, info=info)
        ki = kinv.view(batch, n, n)
        khy = ki @ hy3
        kh, ky = khy[:, :, :K], khy[:, :, K:]
        la = torch.linalg.cholesky_ex(h3.transpose(1, 2) @ kh).L
        u = torch.linalg.solve_triangular(la, kh.transpose(1, 2), upper=False).transpose(1, 2)  # Kinv H L_A^-T
        al = (ky - u @ (u.transpose(1, 2) @ y3.transpose(1, 2))).transpose(1, 2)
        return outputs(torch.diagonal(ki, dim1=1, dim2=2) - (u * u).sum(dim=2), al)

    fns = {"trend_loo": lambda: api.trend_loo_batched(n, b, vc, vh, vy, mean=mean, var=var, logpl=logpl, info=info, want=(), nbasis=K),
           "trend_grad": grad_route, "inverse": inverse_route}
    row = {"dtype": "f64" if f64 else "f32", "n": n, "nbasis": K, "ntarget": D, "batch": batch}
    res = measure(fns, info, window)
    # ours against the inverse route (other kernels, the same inputs) must agree. The trend_grad route recovers P_ii from a cancelling
    # difference: its deviation is recorded and reported, not asserted (trend_grad_valid false: its values are off, its rate stands)
    m, v, lp = inverse_route()
    agree(mean.view(batch, D, n), m, f64, "mean against the inverse route")
    agree(var.view(batch, n), v, f64, "var against the inverse route")
    agree(logpl.view(batch, D), lp, f64, "logpl against the inverse route")
    m, v, lp = grad_route()
    dev = {}
    for what, got, want in (("mean", mean.view(batch, D, n), m), ("var", var.view(batch, n), v), ("logpl", logpl.view(batch, D), lp)):
        d = float((got - want).abs().max()) / max(float(got.abs().max()), 1.0)
        dev[what] = d if math.isfinite(d) else None
    row["trend_grad_rel_deviation"] = dev
    row["trend_grad_valid"] = all(d is not None and d <= (1e-9 if f64 else 2e-3) for d in dev.values())
    if not row["trend_grad_valid"]:
        print(f"trend_grad route deviates: n={n} K={K} D={D} {row['dtype']} {dev}", file=sys.stderr, flush=True)
    del m, v, lp
    code = api.F64 if f64 else api.F32
    kernels = {"trend_loo": api.trend_loo_kernel_name(code, n),
               "trend_grad": f"{api.trend_grad_kernel_name(code, n)} + torch elementwise",
               "inverse": f"{api.kernel_name(api.ALGO_CHOLESKY, code, n)} + torch bmm / cholesky_ex / solve_triangular + elementwise"}
    for k in fns:
        row[k] = dict(res[k], kernel=kernels[k], per_s=batch / res[k]["ms"] * 1e3)
    nbytes = (n * n / 2 + n + K * n + D * n + n + D * n + D) * (8 if f64 else 4)
    row["hbm_bytes_per_matrix"] = nbytes
    row["hbm_frac"] = nbytes * row["trend_loo"]["per_s"] / HBM_PEAK
    row["ours_over_trend_grad"] = row["trend_loo"]["per_s"] / row["trend_grad"]["per_s"]
    row["ours_over_inverse"] = row["trend_loo"]["per_s"] / row["inverse"]["per_s"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="n = 64, (K, D) = (4, 16) only, short windows (for profiling runs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_trend_loo.py needs a GPU"
    torch.cuda.set_device(0)
    dts = (torch.float64, torch.float32)
    shapes = [(n, K, D, dt) for dt in dts for n in (16, 32, 64, 96, 130) for K, D in ((1, 1), (4, 16), (16, 16))]
    if args.quick:
        shapes, args.window = [(64, 4, 16, dt) for dt in dts], min(args.window, 0.05)
    print("| dtype | n | K | D | trend LOO /s | spread | HBM | trend_grad route /s | spread | ours / trend_grad route | inverse route /s | "
          "spread | ours / inverse route |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    rows = []
    for n, K, D, dt in shapes:
        r = run_trend_loo(n, K, D, dt, args.batch if n <= 96 else max(1, args.batch // 50), args.window)
        rows.append(r)
        print(f"| {r['dtype']} | {r['n']} | {r['nbasis']} | {r['ntarget']} | {r['trend_loo']['per_s']:.3e} | "
              f"{100 * r['trend_loo']['spread']:.1f} % | {r['hbm_frac']:.2f} | {r['trend_grad']['per_s']:.3e} | "
              f"{100 * r['trend_grad']['spread']:.1f} % | {r['ours_over_trend_grad']:.2f} | {r['inverse']['per_s']:.3e} | "
              f"{100 * r['inverse']['spread']:.1f} % | {r['ours_over_inverse']:.2f} |", flush=True)
        if args.out:  # after every shape: a run cut short keeps what it measured
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "trend_loo_times.json"), "w") as f:
                json.dump(rows, f, indent=1, allow_nan=False)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
