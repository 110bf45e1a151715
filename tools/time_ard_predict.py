#!/usr/bin/env python3
"""Time GP prediction from coordinates (matinv_ard_predict_batched) against the two routes a caller had before, in the same run and
alternating with them. Both start from the same X, y, theta and Xq and build M, the cross-covariance vectors A and the prior variances E
in torch on every call, as a caller with freshly fitted hyperparameters has to:
    (a) torch builds them, then predict_batched;
    (b) torch builds them, then torch.linalg.cholesky_ex + cholesky_solve.

    python tools/time_ard_predict.py [--batch 100000] [--window 0.25] [--out DIR] [--quick]

Device events around back-to-back launches. All cases of a shape are warmed up first; then three rounds, each timing every case once
over a window of at least --window seconds (so the cases alternate); the median of a case's three windows is reported, with their spread
(max / min - 1) beside it. Rates are matrices per second (each with its Q queries). The new call runs the whole --batch (cut to what its
2 Q outputs per matrix leave room for); the torch routes hold about (d + 3) (n + Q) n elements per matrix in flight, so their batch is
cut to what fits 6 GB and their rate is per matrix all the same (the row says which batch each side ran). "shared" rows share X, y and Xq
across the batch (stride 0); theta is always per matrix. Prints a markdown table; writes ard_predict_times.json under --out.
"""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
api = importlib.import_module("cuda-matrix-inversion_amd.api")

CASES = ("ard_predict", "torch_matinv", "torch_cholesky")


def window_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def phi(s, kind):
    if kind == api.COV_SE:
        return torch.exp(-0.5 * s)
    a = torch.sqrt(5.0 * s)
    return (1.0 + a + (5.0 / 3.0) * s) * torch.exp(-a)


def build(X, Xq, th, n, d, kind):
    """(M (b, n, n), A (b, Q, n), E (b, Q)) in torch from the points (b or 1, n, d), the queries (b or 1, Q, d) and theta (b, d + 2)"""
    sf2, ell, sn2 = th[:, 0].exp(), th[:, 1:d + 1].exp(), th[:, d + 1].exp()
    z, zq = X / ell[:, None, :], Xq / ell[:, None, :]
    m = sf2[:, None, None] * phi(((z[:, :, None, :] - z[:, None, :, :]) ** 2).sum(-1), kind) + \
        sn2[:, None, None] * torch.eye(n, dtype=X.dtype, device=X.device)
    a = sf2[:, None, None] * phi(((zq[:, :, None, :] - z[:, None, :, :]) ** 2).sum(-1), kind)
    return m, a, sf2[:, None].expand(-1, Xq.shape[1]).contiguous()


def run_shape(n, d, Q, dt, kind, shared, batch, window):
    f64 = dt == torch.float64
    code = api.F64 if f64 else api.F32
    esz = 8 if f64 else 4
    batch = max(64, min(batch, int(2e9 / (2 * Q * esz))))
    small = max(64, min(batch, int(6e9 / ((d + 3) * (n + Q) * n * esz))))
    g = torch.Generator(device="cuda").manual_seed(n + d + Q)

    def rand(*shape):
        return torch.rand(*shape, dtype=torch.float64, device="cuda", generator=g)

    nb = 1 if shared else batch
    X = (rand(nb, n, d) * n ** (1.0 / d)).to(dt)
    Xq = (rand(nb, Q, d) * n ** (1.0 / d)).to(dt)
    y = torch.randn(nb, n, dtype=torch.float64, device="cuda", generator=g).to(dt)
    sf2 = 0.5 + 1.5 * rand(batch)
    th = torch.cat([sf2.log()[:, None], (0.5 + 0.5 * rand(batch, d)).log(), ((0.3 + 0.3 * rand(batch)) * sf2).log()[:, None]], 1).to(dt)
    mean = torch.empty(batch * Q, dtype=dt, device="cuda")
    var = torch.empty(batch * Q, dtype=dt, device="cuda")
    info = torch.empty(batch, dtype=torch.int32, device="cuda")
    cut = (lambda t: t) if shared else (lambda t: t[:small].contiguous())
    Xs, Xqs, ys, ths = cut(X), cut(Xq), cut(y), th[:small].contiguous()
    Xa, ya, Xqa = (X[0], y[0], Xq[0]) if shared else (X, y, Xq)  # a 2-D tensor is a shared set to the api

    def new_call():
        api.ard_predict_batched(n, Xa, ya, th, Xqa, kind=kind, mean=mean, var=var, ndim=d, batchSize=batch, info=info, want=())

    def torch_matinv():
        m, a, e = build(Xs, Xqs, ths, n, d, kind)
        return api.predict_batched(n, m.reshape(-1), None, ys.expand(small, n).reshape(-1), a.reshape(-1), e.reshape(-1))

    def torch_cholesky():
        m, a, e = build(Xs, Xqs, ths, n, d, kind)
        L, _ = torch.linalg.cholesky_ex(m)
        rhs = torch.cat([ys.expand(small, n)[:, :, None], a.transpose(1, 2)], dim=2)  # alpha and K A in one solve
        sol = torch.cholesky_solve(rhs, L)
        return torch.einsum("kqi,ki->kq", a, sol[:, :, 0]), e - torch.einsum("kqi,kiq->kq", a, sol[:, :, 1:])

    fns = dict(zip(CASES, (new_call, torch_matinv, torch_cholesky)))
    reps = {}
    for k, fn in fns.items():  # warm up every case of this shape, and size their windows
        fn()
        torch.cuda.synchronize()
        reps[k] = max(1, int(window * 1e3 / max(window_ms(fn, 2), 1e-3)))
    assert int(info.abs().sum()) == 0
    # the three routes compute the same thing: the deviation of the new call from each, relative to the largest value
    dev = {}
    for k in ("torch_matinv", "torch_cholesky"):
        mn, vr = fns[k]()
        dev[k] = (float((mean[:small * Q] - mn.reshape(-1)).abs().max()) / max(1.0, float(mn.abs().max())),
                  float((var[:small * Q] - vr.reshape(-1)).abs().max()) / max(1.0, float(vr.abs().max())))
    assert max(dev["torch_matinv"]) <= (1e-8 if f64 else 5e-3), ("the new call and route (a) disagree", dev)
    ms = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            ms[k].append(window_ms(fn, reps[k]))
    kernels = {"ard_predict": api.ard_predict_kernel_name(code, kind, n), "torch_matinv": "torch + " + api.predict_kernel_name(code, n),
               "torch_cholesky": "torch + torch.linalg"}
    row = {"dtype": "f64" if f64 else "f32", "n": n, "d": d, "nquery": Q, "kind": "se" if kind == api.COV_SE else "matern52",
           "shared": shared}
    for k in fns:
        t = sorted(ms[k])
        b = batch if k == "ard_predict" else small
        row[k] = {"kernel": kernels[k], "batch": b, "ms": t[1], "windows_ms": ms[k], "spread": t[2] / t[0] - 1.0, "per_s": b / t[1] * 1e3}
    row["deviation_mean_var"] = dev
    row["ard_predict_over_torch_matinv"] = row["ard_predict"]["per_s"] / row["torch_matinv"]["per_s"]
    row["ard_predict_over_torch_cholesky"] = row["ard_predict"]["per_s"] / row["torch_cholesky"]["per_s"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="n = 64, d = 2, Q = 16 only, short windows")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_ard_predict.py needs a GPU"
    torch.cuda.set_device(0)
    se, m52 = api.COV_SE, api.COV_MATERN52
    shapes = [(n, d, Q, dt, se, sh) for dt in (torch.float64, torch.float32) for n in (16, 32, 64, 96, 130) for d in (2, 8)
              for Q in (16, 256) for sh in (False, True)]
    shapes += [(64, d, Q, dt, m52, sh) for dt in (torch.float64, torch.float32) for d in (2, 8) for Q in (16, 256) for sh in (False, True)]
    if args.quick:
        shapes, args.window = [(64, 2, 16, torch.float64, se, False), (64, 2, 16, torch.float32, se, True)], min(args.window, 0.05)
    print("| dtype | n | d | Q | kind | inputs | ard_predict /s | spread | (a) torch + predict /s | spread | (b) torch + cholesky /s | spread "
          "| new / (a) | new / (b) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    rows = []
    for n, d, Q, dt, kind, sh in shapes:
        r = run_shape(n, d, Q, dt, kind, sh, args.batch if n <= 96 else min(args.batch, 4000), args.window)
        rows.append(r)
        p, a, b = r["ard_predict"], r["torch_matinv"], r["torch_cholesky"]
        print(f"| {r['dtype']} | {n} | {d} | {Q} | {r['kind']} | {'shared' if sh else 'own'} | {p['per_s']:.3e} | {100 * p['spread']:.1f} % | "
              f"{a['per_s']:.3e} | {100 * a['spread']:.1f} % | {b['per_s']:.3e} | {100 * b['spread']:.1f} % | "
              f"{r['ard_predict_over_torch_matinv']:.1f} | {r['ard_predict_over_torch_cholesky']:.1f} |", flush=True)
        if max(r["deviation_mean_var"]["torch_cholesky"]) > (1e-8 if r["dtype"] == "f64" else 5e-3):
            print(f"  route (b) deviates from the new call by {r['deviation_mean_var']['torch_cholesky']} (mean, var)", flush=True)
        if args.out:  # after every row: a run that is cut short keeps what it measured
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "ard_predict_times.json"), "w") as f:
                json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
