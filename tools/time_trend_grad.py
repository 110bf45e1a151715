#!/usr/bin/env python3
"""Time the gradients of the trend GP's restricted log marginal likelihood (matinv_trend_grad_batched; grad and logml requested) against
the two routes a caller had before, in the same run and alternating with them:
  composed: inverse_batched on M for Kinv, then in torch Kinv H, A = H^T Kinv H, P = Kinv - Kinv H A^-1 H^T Kinv, alpha = P Y,
            G = alpha alpha^T - D P by baddbmm and grad by einsum against dM; one trend_batched for logml (the matrix factorised twice);
  torch:    torch.linalg.cholesky_ex on M, torch.cholesky_solve for Kinv [H | Y], torch.cholesky_inverse for Kinv,
            torch.linalg.cholesky_ex on A, the same algebra, logml from the dot products and the two 2 sum log diag L.

    python tools/time_trend_grad.py [--batch 100000] [--window 0.5] [--out DIR] [--quick]

The method is tools/time_multi_target_grad.py's: device events around back-to-back launches; every case of a
shape is warmed up first; then three rounds, each timing every case once over a window of at least --window seconds (so the cases
alternate); the median of a case's three windows is reported, with their spread (max / min - 1) beside it. Rates are matrices per second
(each with its K basis vectors, D targets and P derivative matrices). "HBM" is the fraction of 8 TB/s that the bytes the kernel must move
amount to: n^2 / 2 + n + K n + D n + P n^2 / 2 elements read, P + D written by this request. n = 130 runs the global form (one
workgroup per matrix, written to be correct, not fast) on a fiftieth of the batch, and K is held to n / 2 (n = 16 runs K = 8). Ours must
agree with the composed route; where the torch route's own values do not agree with ours the row is marked (torch_valid false) and
carries no ratio against it. Prints a markdown table; writes trend_grad_times.json under --out.
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


def run_trend_grad(n, K, D, P, dt, batch, window):
    f64 = dt == torch.float64
    K = min(K, n // 2)  # n = 16 runs K = 8: with K = n the projection P vanishes and A of a random basis is singular to fp32
    g = torch.Generator(device="cuda").manual_seed(n)
    b = spd(batch, n, dt, g, n)
    vc = torch.rand(batch * n, dtype=dt, device="cuda", generator=g)
    vh = torch.randn(batch * K * n, dtype=dt, device="cuda", generator=g)
    vh.view(batch, K, n)[:, 0] = 1.0
    vy = torch.randn(batch * D * n, dtype=dt, device="cuda", generator=g)
    dms = torch.randn(batch * P * n * n, dtype=dt, device="cuda", generator=g)
    dm4 = dms.view(batch, P, n, n)
    for p in range(P):  # symmetric, one p at a time to keep the transient small
        dm4[:, p].add_(dm4[:, p].transpose(1, 2).clone())
    grad = torch.empty(batch * P, dtype=dt, device="cuda")
    logml = torch.empty(batch * D, dtype=dt, device="cuda")
    lm1 = torch.empty_like(logml)
    kinv = torch.empty(batch * n * n, dtype=dt, device="cuda")
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    m3 = b.view(batch, n, n) + torch.diag_embed(vc.view(batch, n))
    mflat = m3.reshape(-1)
    h3 = vh.view(batch, K, n).transpose(1, 2)  # h3[k] = H_k, n x K
    y3 = vy.view(batch, D, n).transpose(1, 2)  # y3[k] = Y_k, n x D
    hy3 = torch.cat([h3, y3], dim=2).contiguous()
    const = (n - K) * math.log(2 * math.pi)

    def algebra(ki, kh, ky):
        """grad from Kinv, Kinv H and Kinv Y; also the factor of A and alpha"""
        # cholesky_ex: no host check between the launches; where the route's own Kinv H is wrong (see torch_valid) A need not be
        # positive definite, and the row is then marked, not aborted
        la = torch.linalg.cholesky_ex(h3.transpose(1, 2) @ kh).L
        u = torch.linalg.solve_triangular(la, kh.transpose(1, 2), upper=False).transpose(1, 2)  # Kinv H L_A^-T
        al = ky - u @ (u.transpose(1, 2) @ y3)
        pm = torch.baddbmm(ki, u, u.transpose(1, 2), alpha=-1.0)
        gm = torch.baddbmm(pm, al, al.transpose(1, 2), beta=-float(D))
        return 0.5 * torch.einsum("kij,kpij->kp", gm, dm4), la, al

    def composed():
        api.inverse_batched(mflat, n, api.ALGO_CHOLESKY, out=kinv, info=info)
        ki = kinv.view(batch, n, n)
        khy = ki @ hy3
        gr, _, _ = algebra(ki, khy[:, :, :K], khy[:, :, K:])
        api.trend_batched(n, b, vc, vh, vy, logml=lm1, info=info, want=(), nbasis=K)
        return gr

    def torch_route():
        lo = torch.linalg.cholesky_ex(m3).L
        khy = torch.cholesky_solve(hy3, lo)
        gr, la, al = algebra(torch.cholesky_inverse(lo), khy[:, :, :K], khy[:, :, K:])
        ld = 2 * torch.log(torch.diagonal(lo, dim1=1, dim2=2)).sum(dim=1) + 2 * torch.log(torch.diagonal(la, dim1=1, dim2=2)).sum(dim=1)
        quad = (y3 * al).sum(dim=1)
        return gr, -0.5 * (quad + ld[:, None] + const)

    fns = {"trend_grad": lambda: api.trend_grad_batched(n, b, vc, vh, vy, dms, grad=grad, logml=logml, info=info, want=(), nbasis=K),
           "composed": composed, "torch": torch_route}
    row = {"dtype": "f64" if f64 else "f32", "n": n, "nbasis": K, "ntarget": D, "nparam": P, "batch": batch}
    gr, lm = torch_route()
    torch.cuda.synchronize()
    res = measure(fns, info, window)
    # ours against the composed route (other kernels, the same inputs) must agree. The torch route's values, taken from one synchronised
    # call in front of the timed windows and again behind them, are compared and not asserted: a deviation beyond the tolerance of
    # `agree`, or a value that is not finite, makes the row's torch comparison invalid (torch_valid false, ours_over_torch null) and is
    # reported on stderr; the route's rate is still recorded, as the rate of the calls as issued
    agree(logml, lm1, f64, "logml against trend_batched")
    agree(grad.view(batch, P), composed(), f64, "grad against the composed route")
    gr2, lm2 = torch_route()
    dev = {}
    for when, (tg, tl) in (("before", (gr, lm)), ("after", (gr2, lm2))):
        for what, got, want in (("grad", grad.view(batch, P), tg), ("logml", logml.view(batch, D), tl)):
            d = float((got - want).abs().max()) / max(float(want.abs().max()), 1.0)
            dev[f"{what}_{when}"] = d if math.isfinite(d) else None  # None: the torch route returned a value that is not finite
    row["torch_rel_deviation"] = dev
    row["torch_valid"] = all(d is not None and d <= (1e-9 if f64 else 2e-3) for d in dev.values())
    if not row["torch_valid"]:
        print(f"torch route deviates: n={n} K={K} D={D} P={P} {row['dtype']} {dev}", file=sys.stderr, flush=True)
    del gr, lm, gr2, lm2
    code = api.F64 if f64 else api.F32
    kernels = {"trend_grad": api.trend_grad_kernel_name(code, n),
               "composed": f"{api.kernel_name(api.ALGO_CHOLESKY, code, n)} + torch bmm / cholesky_ex / solve_triangular / baddbmm / einsum + "
                           f"{api.trend_kernel_name(code, n)}",
               "torch": "torch.linalg.cholesky_ex + cholesky_solve + cholesky_inverse + baddbmm + einsum"}
    for k in fns:
        row[k] = dict(res[k], kernel=kernels[k], per_s=batch / res[k]["ms"] * 1e3)
    nbytes = (n * n / 2 + n + K * n + D * n + P * n * n / 2 + P + D) * (8 if f64 else 4)
    row["hbm_bytes_per_matrix"] = nbytes
    row["hbm_frac"] = nbytes * row["trend_grad"]["per_s"] / HBM_PEAK
    row["ours_over_composed"] = row["trend_grad"]["per_s"] / row["composed"]["per_s"]
    row["ours_over_torch"] = row["trend_grad"]["per_s"] / row["torch"]["per_s"] if row["torch_valid"] else None
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="n = 64, (K, D, P) = (4, 16, 4) only, short windows (for profiling runs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_trend_grad.py needs a GPU"
    torch.cuda.set_device(0)
    dts = (torch.float64, torch.float32)
    shapes = [(n, K, D, P, dt) for dt in dts for n in (16, 32, 64, 96, 130) for K, D, P in ((1, 1, 1), (4, 16, 4), (16, 16, 4))]
    if args.quick:
        shapes, args.window = [(64, 4, 16, 4, dt) for dt in dts], min(args.window, 0.05)
    print("| dtype | n | K | D | P | trend grad /s | spread | HBM | composed /s | spread | ours / composed | torch route /s | spread | "
          "ours / torch route |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    rows = []
    for n, K, D, P, dt in shapes:
        r = run_trend_grad(n, K, D, P, dt, args.batch if n <= 96 else max(1, args.batch // 50), args.window)
        rows.append(r)
        print(f"| {r['dtype']} | {r['n']} | {r['nbasis']} | {r['ntarget']} | {r['nparam']} | {r['trend_grad']['per_s']:.3e} | "
              f"{100 * r['trend_grad']['spread']:.1f} % | {r['hbm_frac']:.2f} | {r['composed']['per_s']:.3e} | "
              f"{100 * r['composed']['spread']:.1f} % | {r['ours_over_composed']:.2f} | {r['torch']['per_s']:.3e} | "
              f"{100 * r['torch']['spread']:.1f} % | {'%.2f' % r['ours_over_torch'] if r['torch_valid'] else 'torch values invalid'} |",
              flush=True)
        if args.out:  # after every shape: a run cut short keeps what it measured
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "trend_grad_times.json"), "w") as f:
                json.dump(rows, f, indent=1, allow_nan=False)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
