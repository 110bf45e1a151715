#!/usr/bin/env python3
"""Time the GP log marginal likelihood and its gradient from coordinates (matinv_ard_logml_batched) against the two routes a caller had
before, in the same run and alternating with them. Both start from the same X, y and theta and build M and the d + 2 derivative
matrices in torch on every call, as an optimiser step has to:
    (a) torch builds them, then logml_batched + logml_grad_batched;
    (b) torch builds them, then torch.linalg.cholesky_ex + cholesky_solve + cholesky_inverse + einsum.

    python tools/time_ard_logml.py [--batch 100000] [--window 0.25] [--out DIR] [--quick]

Device events around back-to-back launches. All cases of a shape are warmed up first; then three rounds, each timing every case once
over a window of at least --window seconds (so the cases alternate); the median of a case's three windows is reported, with their spread
(max / min - 1) beside it. Rates are matrices per second. The new call runs the whole --batch; the torch routes hold (2 d + 6) n^2
elements per matrix in flight, so their batch is cut to what fits 6 GB and their rate is per matrix all the same (the row says which
batch each side ran). Prints a markdown table; writes ard_logml_times.json under --out.
"""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
api = importlib.import_module("cuda-matrix-inversion_amd.api")

CASES = ("ard", "torch_matinv", "torch_cholesky")
LOG2PI = 1.8378770664093453


def window_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def build(X, th, n, d, kind):
    """(M (b, n, n), dM (b, d + 2, n, n)) in torch from the points (b or 1, n, d) and theta (b, d + 2)"""
    sf2, ell, sn2 = th[:, 0].exp(), th[:, 1:d + 1].exp(), th[:, d + 1].exp()
    z = X / ell[:, None, :]
    d2 = (z[:, :, None, :] - z[:, None, :, :]) ** 2
    s = d2.sum(-1)
    if kind == api.COV_SE:
        phi = torch.exp(-0.5 * s)
        psi = phi
    else:
        a = torch.sqrt(5.0 * s)
        e = torch.exp(-a)
        phi, psi = (1.0 + a + (5.0 / 3.0) * s) * e, (5.0 / 3.0) * (1.0 + a) * e
    eye = torch.eye(n, dtype=X.dtype, device=X.device)
    k0 = sf2[:, None, None] * phi
    noise = sn2[:, None, None] * eye
    dm = torch.cat([k0[:, None], (sf2[:, None, None] * psi)[:, None] * d2.permute(0, 3, 1, 2), noise[:, None]], dim=1)
    return k0 + noise, dm


def run_shape(n, d, dt, kind, shared, batch, window):
    f64 = dt == torch.float64
    code = api.F64 if f64 else api.F32
    esz = 8 if f64 else 4
    small = max(64, min(batch, int(6e9 / ((2 * d + 6) * n * n * esz))))
    g = torch.Generator(device="cuda").manual_seed(n + d)

    def rand(*shape):
        return torch.rand(*shape, dtype=torch.float64, device="cuda", generator=g)

    X = (rand(1 if shared else batch, n, d) * n ** (1.0 / d)).to(dt)
    y = torch.randn(batch, n, dtype=torch.float64, device="cuda", generator=g).to(dt)
    sf2 = 0.5 + 1.5 * rand(batch)
    th = torch.cat([sf2.log()[:, None], (0.5 + 0.5 * rand(batch, d)).log(), ((0.3 + 0.3 * rand(batch)) * sf2).log()[:, None]], 1).to(dt)
    logml = torch.empty(batch, dtype=dt, device="cuda")
    grad = torch.empty(batch * (d + 2), dtype=dt, device="cuda")
    info = torch.empty(batch, dtype=torch.int32, device="cuda")
    Xs, ys, ths = (X if shared else X[:small]), y[:small].contiguous(), th[:small].contiguous()

    def new_call():
        api.ard_logml_batched(n, X, y, th, kind=kind, logml=logml, grad=grad, ndim=d, batchSize=batch, info=info, want=())

    def torch_matinv():
        m, dm = build(Xs, ths, n, d, kind)
        lm = api.logml_batched(n, m.reshape(-1), None, ys.reshape(-1))
        gr = api.logml_grad_batched(n, m.reshape(-1), None, ys.reshape(-1), dm.reshape(-1), want=("grad",))[0]
        return lm, gr

    def torch_cholesky():
        m, dm = build(Xs, ths, n, d, kind)
        L, _ = torch.linalg.cholesky_ex(m)
        al = torch.cholesky_solve(ys[:, :, None], L)[:, :, 0]
        k = torch.cholesky_inverse(L)
        lm = -0.5 * ((ys * al).sum(1) + 2.0 * torch.diagonal(L, dim1=1, dim2=2).log().sum(1) + n * LOG2PI)
        return lm, 0.5 * torch.einsum("kij,kpij->kp", al[:, :, None] * al[:, None, :] - k, dm)

    fns = {"ard": new_call, "torch_matinv": torch_matinv, "torch_cholesky": torch_cholesky}
    reps = {}
    for k, fn in fns.items():  # warm up every case of this shape, and size their windows
        fn()
        torch.cuda.synchronize()
        reps[k] = max(1, int(window * 1e3 / max(window_ms(fn, 2), 1e-3)))
    assert int(info.abs().sum()) == 0
    # the three routes compute the same thing: the deviation of the new call from each, relative to the largest value
    dev = {}
    for k in ("torch_matinv", "torch_cholesky"):
        lm, gr = fns[k]()
        dev[k] = (float((logml[:small] - lm).abs().max()) / max(1.0, float(lm.abs().max())),
                  float((grad[:small * (d + 2)] - gr.reshape(-1)).abs().max()) / max(1.0, float(gr.abs().max())))
    assert max(dev["torch_matinv"]) <= (1e-8 if f64 else 5e-3), ("the new call and route (a) disagree", dev)
    ms = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            ms[k].append(window_ms(fn, reps[k]))
    kernels = {"ard": api.ard_logml_kernel_name(code, kind, n),
               "torch_matinv": "torch + " + api.logml_kernel_name(code, n) + " + " + api.logml_grad_kernel_name(code, n),
               "torch_cholesky": "torch + torch.linalg"}
    row = {"dtype": "f64" if f64 else "f32", "n": n, "d": d, "kind": "se" if kind == api.COV_SE else "matern52", "shared_x": shared}
    for k in fns:
        t = sorted(ms[k])
        b = batch if k == "ard" else small
        row[k] = {"kernel": kernels[k], "batch": b, "ms": t[1], "windows_ms": ms[k], "spread": t[2] / t[0] - 1.0, "per_s": b / t[1] * 1e3}
    row["deviation_logml_grad"] = dev
    row["ard_over_torch_matinv"] = row["ard"]["per_s"] / row["torch_matinv"]["per_s"]
    row["ard_over_torch_cholesky"] = row["ard"]["per_s"] / row["torch_cholesky"]["per_s"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="n = 64, d = 2 only, short windows")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_ard_logml.py needs a GPU"
    torch.cuda.set_device(0)
    se, m52 = api.COV_SE, api.COV_MATERN52
    shapes = [(n, d, dt, se, sh) for dt in (torch.float64, torch.float32) for n in (16, 32, 64, 96, 130) for d in (2, 8)
              for sh in (False, True)]
    shapes += [(64, d, dt, m52, sh) for dt in (torch.float64, torch.float32) for d in (2, 8) for sh in (False, True)]
    if args.quick:
        shapes, args.window = [(64, 2, torch.float64, se, False), (64, 2, torch.float32, se, False)], min(args.window, 0.05)
    print("| dtype | n | d | kind | X | ard /s | spread | (a) torch + matinv /s | spread | (b) torch + cholesky /s | spread | ard / (a) | ard / (b) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    rows = []
    for n, d, dt, kind, sh in shapes:
        r = run_shape(n, d, dt, kind, sh, args.batch if n <= 96 else min(args.batch, 4000), args.window)
        rows.append(r)
        print(f"| {r['dtype']} | {n} | {d} | {r['kind']} | {'shared' if sh else 'own'} | {r['ard']['per_s']:.3e} | "
              f"{100 * r['ard']['spread']:.1f} % | {r['torch_matinv']['per_s']:.3e} | {100 * r['torch_matinv']['spread']:.1f} % | "
              f"{r['torch_cholesky']['per_s']:.3e} | {100 * r['torch_cholesky']['spread']:.1f} % | {r['ard_over_torch_matinv']:.1f} | "
              f"{r['ard_over_torch_cholesky']:.1f} |", flush=True)
        if max(r["deviation_logml_grad"]["torch_cholesky"]) > (1e-8 if r["dtype"] == "f64" else 5e-3):
            print(f"  route (b) deviates from the new call by {r['deviation_logml_grad']['torch_cholesky']} (logml, grad)", flush=True)
        if args.out:  # after every row: a run that is cut short keeps what it measured
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "ard_logml_times.json"), "w") as f:
                json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
