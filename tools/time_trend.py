#!/usr/bin/env python3
"""Time the GP regression with a linear trend (matinv_trend_batched; all seven outputs requested) against the two routes a caller had
before, in the same run and alternating with them:
  composed: multi_target_batched on [H | Y] (alpha = Kinv [H | Y] and log det M), predict_batched for e - a^T Kinv a, and the K x K
            algebra (A = H^T Kinv H, its Cholesky factor, beta, the corrections, r^T A^-1 r) as small torch launches: two factorisations
            of every matrix, and n (K + D) elements written and read back;
  torch:    torch.linalg.cholesky on M, torch.cholesky_solve for Kinv [H | Y | A^T], and the same small algebra.

    python tools/time_trend.py [--batch 100000] [--window 0.3] [--out DIR] [--quick]

The method is tools/time_multi_target.py's: device events around back-to-back launches; every case of a shape is
warmed up first; then FIVE rounds, each timing every case once over a window of at least --window seconds (so the cases alternate); the
median of a case's five windows is reported, with their spread (max / min - 1) beside it. Rates are matrices per second (each with its K
basis vectors, D targets and Q queries). A row is a loss when the fused rate is below the composed one by more than the composed route's
own spread. K is held to n / 2 (at n = 16 the shape (16, 16, 64) runs with K = 8): with a random basis A = H^T Kinv H loses its
conditioning as K approaches n (cond2 1.4e5 at n = K = 16), and the fp32 routes then disagree beyond what `agree` allows. The batch is
--batch up to n = 96 and --batch / 50 beyond, where the global-memory kernels keep a working copy per matrix.
"HBM" is the fraction of 8 TB/s that the bytes the tile kernel must move amount to: n^2 / 2 + n + K n + D n +
(ceil(D / 16) + 1) Q (n + K) + Q elements read, K^2 + D K + D n + 2 D + D Q + Q written. Prints a markdown table; writes trend_times.json
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
from time_sample import agree, spd, window_ms  # noqa: E402

api = importlib.import_module("cuda-matrix-inversion_amd.api")
HBM_PEAK = 8e12
ROUNDS = 5


def measure(fns, info, window):
    """time_sample.measure with five rounds: {case: median ms, windows, spread}"""
    reps = {}
    for k, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        assert int(info.abs().sum()) == 0, k
        reps[k] = max(1, int(window * 1e3 / max(window_ms(fn, 2), 1e-3)))
    ms = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            ms[k].append(window_ms(fn, reps[k]))
    out = {}
    for k in fns:
        t = sorted(ms[k])
        out[k] = {"ms": t[ROUNDS // 2], "windows_ms": ms[k], "spread": t[-1] / t[0] - 1.0}
    return out


def run_trend(n, K, D, Q, dt, batch, window):
    f64 = dt == torch.float64
    g = torch.Generator(device="cuda").manual_seed(n)
    new = lambda *shape: torch.randn(*shape, dtype=dt, device="cuda", generator=g)  # noqa: E731
    b = spd(batch, n, dt, g, n)
    vc = torch.rand(batch * n, dtype=dt, device="cuda", generator=g)
    hy = new(batch, K + D, n)  # [H | Y] packed as the composed route wants it
    hy[:, 0] = 1.0
    vh, vy = hy[:, :K].contiguous().view(-1), hy[:, K:].contiguous().view(-1)
    va, vg, ve = new(batch * Q * n), new(batch, Q, K), torch.rand(batch * Q, dtype=dt, device="cuda", generator=g) + n
    vg[:, :, 0] = 1.0
    vg = vg.view(-1)
    empty = lambda count: torch.empty(count, dtype=dt, device="cuda")  # noqa: E731
    outs = dict(beta=empty(batch * D * K), covbeta=empty(batch * K * K), alpha=empty(batch * D * n), quad=empty(batch * D),
                logml=empty(batch * D), mean=empty(batch * D * Q), var=empty(batch * Q))
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    sol, ld, pv = empty(batch * (K + D) * n), empty(batch), empty(batch * Q)
    m3 = b.view(batch, n, n) + torch.diag_embed(vc.view(batch, n))
    h3, y3 = vh.view(batch, K, n).transpose(1, 2), vy.view(batch, D, n).transpose(1, 2)  # n x K, n x D
    a3, g3, e2 = va.view(batch, Q, n), vg.view(batch, Q, K), ve.view(batch, Q)
    rhs = torch.cat([h3, y3, a3.transpose(1, 2)], dim=2).contiguous()
    const = (n - K) * math.log(2 * math.pi)

    def algebra(kh, ky, res_var, logdet):
        """the K x K part: kh = Kinv H (n x K), ky = Kinv Y (n x D), res_var = e - a^T Kinv a"""
        la = torch.linalg.cholesky(torch.bmm(h3.transpose(1, 2), kh))
        beta = torch.cholesky_solve(torch.bmm(kh.transpose(1, 2), y3), la)  # K x D
        alpha = ky - torch.bmm(kh, beta)
        quad = (y3 * alpha).sum(dim=1)
        lda = 2 * torch.log(torch.diagonal(la, dim1=1, dim2=2)).sum(dim=1)
        logml = -0.5 * (quad + (logdet + lda)[:, None] + const)
        mean = torch.bmm(a3, alpha) + torch.bmm(g3, beta)  # Q x D
        r = g3 - torch.bmm(a3, kh)  # Q x K
        z = torch.linalg.solve_triangular(la, r.transpose(1, 2), upper=False)
        return beta, torch.cholesky_inverse(la), alpha, quad, logml, mean, res_var + (z * z).sum(dim=1)

    def composed():
        api.multi_target_batched(n, b, vc, hy.view(-1), alpha=sol, logdet=ld, info=info, want=())
        api.predict_batched(n, b, vc, None, va, ve, var=pv, info=info, want=())
        s3 = sol.view(batch, K + D, n)
        return algebra(s3[:, :K].transpose(1, 2), s3[:, K:].transpose(1, 2), pv.view(batch, Q), ld)

    def torch_route():
        lo = torch.linalg.cholesky(m3)
        s = torch.cholesky_solve(rhs, lo)
        logdet = 2 * torch.log(torch.diagonal(lo, dim1=1, dim2=2)).sum(dim=1)
        aka = (a3.transpose(1, 2) * s[:, :, K + D:]).sum(dim=1)
        return algebra(s[:, :, :K], s[:, :, K:K + D], e2 - aka, logdet)

    fns = {"trend": lambda: api.trend_batched(n, b, vc, vh, vy, va, vg, ve, **outs, info=info, want=(), nbasis=K),
           "composed": composed, "torch": torch_route}
    row = {"dtype": "f64" if f64 else "f32", "n": n, "nbasis": K, "ntarget": D, "nquery": Q, "batch": batch}
    res = measure(fns, info, window)
    beta, covbeta, alpha, quad, logml, mean, var = torch_route()
    agree(outs["beta"].view(batch, D, K).transpose(1, 2), beta, f64, "beta")
    agree(outs["covbeta"].view(batch, K, K), covbeta, f64, "covbeta")
    agree(outs["alpha"].view(batch, D, n).transpose(1, 2), alpha, f64, "alpha")
    agree(outs["logml"].view(batch, D), logml, f64, "logml")
    agree(outs["mean"].view(batch, D, Q).transpose(1, 2), mean, f64, "mean")
    agree(outs["var"].view(batch, Q), var, f64, "var")
    del beta, covbeta, alpha, quad, logml, mean, var
    code = api.F64 if f64 else api.F32
    kernels = {"trend": api.trend_kernel_name(code, n),
               "composed": f"{api.multi_target_kernel_name(code, n)} + {api.predict_kernel_name(code, n)} + the K x K algebra in torch",
               "torch": "torch.linalg.cholesky + cholesky_solve + the K x K algebra in torch"}
    for k in fns:
        row[k] = dict(res[k], kernel=kernels[k], per_s=batch / res[k]["ms"] * 1e3)
    groups = (D + 15) // 16
    nbytes = (n * n / 2 + n + K * n + D * n + (groups + 1) * Q * (n + K) + Q + K * K + D * K + D * n + 2 * D + D * Q + Q) * (8 if f64 else 4)
    row["hbm_bytes_per_matrix"] = nbytes
    row["hbm_frac"] = nbytes * row["trend"]["per_s"] / HBM_PEAK
    row["ours_over_composed"] = row["trend"]["per_s"] / row["composed"]["per_s"]
    row["ours_over_torch"] = row["trend"]["per_s"] / row["torch"]["per_s"]
    row["loses_to_composed"] = row["ours_over_composed"] < 1.0 / (1.0 + row["composed"]["spread"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="n = 64, (K, D, Q) = (4, 16, 16) only, short windows (for profiling runs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_trend.py needs a GPU"
    torch.cuda.set_device(0)
    dts = (torch.float64, torch.float32)
    shapes = [(n, K, D, Q, dt) for dt in dts for n in (16, 32, 64, 96, 130) for K, D, Q in ((1, 1, 16), (4, 16, 16), (16, 16, 64))]
    if args.quick:
        shapes, args.window = [(64, 4, 16, 16, dt) for dt in dts], min(args.window, 0.05)
    print("| dtype | n | K | D | Q | trend /s | spread | HBM | composed /s | spread | trend / composed | torch route /s | spread | "
          "trend / torch route |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    rows = []
    for n, K, D, Q, dt in shapes:
        r = run_trend(n, min(K, n // 2), D, Q, dt, args.batch if n <= 96 else max(1, args.batch // 50), args.window)
        rows.append(r)
        print(f"| {r['dtype']} | {r['n']} | {r['nbasis']} | {r['ntarget']} | {r['nquery']} | {r['trend']['per_s']:.3e} | "
              f"{100 * r['trend']['spread']:.1f} % | {r['hbm_frac']:.2f} | {r['composed']['per_s']:.3e} | "
              f"{100 * r['composed']['spread']:.1f} % | {r['ours_over_composed']:.2f}{' (loss)' if r['loses_to_composed'] else ''} | "
              f"{r['torch']['per_s']:.3e} | {100 * r['torch']['spread']:.1f} % | {r['ours_over_torch']:.2f} |", flush=True)
        if args.out:  # after every shape: a run cut short keeps what it measured
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "trend_times.json"), "w") as f:
                json.dump(rows, f, indent=1)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
