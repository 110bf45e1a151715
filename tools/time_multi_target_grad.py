#!/usr/bin/env python3
"""Time the gradients of the multi-output GP log marginal likelihood (matinv_multi_target_grad_batched; grad and logml requested) against
the two routes a caller had before, in the same run and alternating with them:
  D calls:  D x logml_grad_batched(grad), one target vector each, summed with torch, plus one multi_target_batched for logml: the same
            matrix factorised D + 1 times and every dM_p streamed D times;
  torch:    torch.linalg.cholesky on M, torch.cholesky_solve for alpha = M^-1 Y, torch.cholesky_inverse for K = M^-1,
            G = alpha alpha^T - D K by bmm, grad by einsum against dM, logml from the dot products and 2 sum log diag L.

    python tools/time_multi_target_grad.py [--batch 100000] [--window 0.5] [--out DIR] [--quick]

The method is tools/time_multi_target.py's: device events around back-to-back launches; every case of a shape is warmed up first; then
three rounds, each timing every case once over a window of at least --window seconds (so the cases alternate); the median of a case's
three windows is reported, with their spread (max / min - 1) beside it. Rates are matrices per second (each with its D targets and P
derivative matrices). "HBM" is the fraction of 8 TB/s that the bytes the kernel must move amount to: n^2 / 2 + n + D n + P n^2 / 2
elements read, P + n + D + D n written (of which this request stores P + D; with D > 16 the D n elements of alpha go out to the
workspace and come back through L2). Ours must agree with the D-call route; where the torch route's own values do not agree with them
the row is marked (torch_valid false) and carries no ratio against it. Prints a markdown table; writes multi_target_grad_times.json
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


def run_multi_target_grad(n, D, P, dt, batch, window):
    f64 = dt == torch.float64
    g = torch.Generator(device="cuda").manual_seed(n)
    b = spd(batch, n, dt, g, n)
    vc = torch.rand(batch * n, dtype=dt, device="cuda", generator=g)
    vy = torch.randn(batch * D * n, dtype=dt, device="cuda", generator=g)
    dms = torch.randn(batch * P * n * n, dtype=dt, device="cuda", generator=g)
    dm4 = dms.view(batch, P, n, n)
    for p in range(P):  # symmetric, one p at a time to keep the transient small
        dm4[:, p].add_(dm4[:, p].transpose(1, 2).clone())
    grad = torch.empty(batch * P, dtype=dt, device="cuda")
    logml = torch.empty(batch * D, dtype=dt, device="cuda")
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    # the D-call route: target t of every matrix packed on its own
    yt = [vy.view(batch, D, n)[:, t].contiguous().view(-1) for t in range(D)]
    g1, gsum, lm1 = torch.empty_like(grad), torch.empty_like(grad), torch.empty_like(logml)
    m3 = b.view(batch, n, n) + torch.diag_embed(vc.view(batch, n))
    y3 = vy.view(batch, D, n).transpose(1, 2)  # y3[k] = Y_k, n x D
    const = n * math.log(2 * math.pi)

    def d_calls():
        gsum.zero_()
        for t in range(D):
            api.logml_grad_batched(n, b, vc, yt[t], dms, grad=g1, info=info, want=())
            gsum.add_(g1)
        api.multi_target_batched(n, b, vc, vy, None, logml=lm1, info=info, want=())

    def torch_route():
        lo = torch.linalg.cholesky(m3)
        al = torch.cholesky_solve(y3, lo)
        gm = torch.baddbmm(torch.cholesky_inverse(lo), al, al.transpose(1, 2), beta=-float(D))
        ld = 2 * torch.log(torch.diagonal(lo, dim1=1, dim2=2)).sum(dim=1)
        quad = (y3 * al).sum(dim=1)
        return 0.5 * torch.einsum("kij,kpij->kp", gm, dm4), -0.5 * (quad + ld[:, None] + const)

    fns = {"multi_target_grad": lambda: api.multi_target_grad_batched(n, b, vc, vy, dms, grad=grad, logml=logml, info=info, want=()),
           "d_calls": d_calls, "torch": torch_route}
    row = {"dtype": "f64" if f64 else "f32", "n": n, "ntarget": D, "nparam": P, "batch": batch}
    gr, lm = torch_route()
    torch.cuda.synchronize()
    res = measure(fns, info, window)
    # ours against the D-call route (other kernels, the same inputs) must agree. The torch route's values, taken from one synchronised
    # call in front of the timed windows and again behind them, are compared and not asserted: a deviation beyond the tolerance of
    # `agree`, or a value that is not finite, makes the row's torch comparison invalid (torch_valid false, ours_over_torch null) and is
    # reported on stderr; the route's rate is still recorded, as the rate of the calls as issued
    agree(grad.view(batch, P), gsum.view(batch, P), f64, "grad against the D calls")
    agree(logml, lm1, f64, "logml against multi_target_batched")
    gr2, lm2 = torch_route()
    dev = {}
    for when, (tg, tl) in (("before", (gr, lm)), ("after", (gr2, lm2))):
        for what, got, want in (("grad", grad.view(batch, P), tg), ("logml", logml.view(batch, D), tl)):
            d = float((got - want).abs().max()) / max(float(want.abs().max()), 1.0)
            dev[f"{what}_{when}"] = d if math.isfinite(d) else None  # None: the torch route returned a value that is not finite
    row["torch_rel_deviation"] = dev
    row["torch_valid"] = all(d is not None and d <= (1e-9 if f64 else 2e-3) for d in dev.values())
    if not row["torch_valid"]:
        print(f"torch route deviates: n={n} D={D} P={P} {row['dtype']} {dev}", file=sys.stderr, flush=True)
    del gr2, lm2
    del gr, lm
    code = api.F64 if f64 else api.F32
    kernels = {"multi_target_grad": api.multi_target_grad_kernel_name(code, n),
               "d_calls": f"{D} x {api.logml_grad_kernel_name(code, n)} + {api.multi_target_kernel_name(code, n)}",
               "torch": "torch.linalg.cholesky + cholesky_solve + cholesky_inverse + baddbmm + einsum"}
    for k in fns:
        row[k] = dict(res[k], kernel=kernels[k], per_s=batch / res[k]["ms"] * 1e3)
    nbytes = (n * n / 2 + n + D * n + P * n * n / 2 + P + n + D + D * n) * (8 if f64 else 4)
    row["hbm_bytes_per_matrix"] = nbytes
    row["hbm_frac"] = nbytes * row["multi_target_grad"]["per_s"] / HBM_PEAK
    row["ours_over_d_calls"] = row["multi_target_grad"]["per_s"] / row["d_calls"]["per_s"]
    row["ours_over_torch"] = row["multi_target_grad"]["per_s"] / row["torch"]["per_s"] if row["torch_valid"] else None
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="n = 64, (D, P) = (16, 4) only, short windows (for profiling runs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_multi_target_grad.py needs a GPU"
    torch.cuda.set_device(0)
    dts = (torch.float64, torch.float32)
    shapes = [(n, D, P, dt) for dt in dts for n in (16, 32, 64, 96) for D, P in ((4, 1), (16, 1), (16, 4), (64, 4))]
    if args.quick:
        shapes, args.window = [(64, 16, 4, dt) for dt in dts], min(args.window, 0.05)
    print("| dtype | n | D | P | multi-target grad /s | spread | HBM | D calls /s | spread | ours / D calls | torch route /s | spread | "
          "ours / torch route |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    rows = []
    for shape in shapes:
        r = run_multi_target_grad(*shape, args.batch, args.window)
        rows.append(r)
        print(f"| {r['dtype']} | {r['n']} | {r['ntarget']} | {r['nparam']} | {r['multi_target_grad']['per_s']:.3e} | "
              f"{100 * r['multi_target_grad']['spread']:.1f} % | {r['hbm_frac']:.2f} | {r['d_calls']['per_s']:.3e} | "
              f"{100 * r['d_calls']['spread']:.1f} % | {r['ours_over_d_calls']:.2f} | {r['torch']['per_s']:.3e} | "
              f"{100 * r['torch']['spread']:.1f} % | {'%.2f' % r['ours_over_torch'] if r['torch_valid'] else 'torch values invalid'} |",
              flush=True)
        if args.out:  # after every shape: a run cut short keeps what it measured
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "multi_target_grad_times.json"), "w") as f:
                json.dump(rows, f, indent=1, allow_nan=False)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
