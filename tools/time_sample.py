#!/usr/bin/env python3
"""Time the batched Cholesky factor with coloured samples (matinv_colour_batched) and the joint posterior samples of a GP
(matinv_sample_batched) against the routes a caller had before, in the same run and alternating with them:
  (a) colour:  torch.linalg.cholesky on C, then torch.baddbmm for Y = m + L Z;
  (b) sample:  matinv_predict_cov_batched for mean and cov, then the same two torch calls on cov.

    python tools/time_sample.py [--batch 100000] [--window 0.5] [--out DIR] [--quick]

Device events around back-to-back launches. Both cases of a shape are warmed up first; then three rounds, each timing every case once over
a window of at least --window seconds (so the cases alternate); the median of a case's three windows is reported, with their spread
(max / min - 1) beside it. Rates are matrices per second (each with its factor and its S samples). Prints a markdown table; writes
sample_times.json under --out.
"""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
api = importlib.import_module("cuda-matrix-inversion_amd.api")


def window_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def measure(fns, info, window):
    """warm up every case, size the windows, three alternating rounds: {case: median ms, windows, spread}"""
    reps = {}
    for k, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        assert int(info.abs().sum()) == 0, k
        reps[k] = max(1, int(window * 1e3 / max(window_ms(fn, 2), 1e-3)))
    ms = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            ms[k].append(window_ms(fn, reps[k]))
    out = {}
    for k in fns:
        t = sorted(ms[k])
        out[k] = {"ms": t[1], "windows_ms": ms[k], "spread": t[2] / t[0] - 1.0}
    return out


def spd(batch, q, dt, g, shift):
    """R + R^T + shift I, packed; symmetric, so its column-major packing is its row-major one"""
    c = torch.rand(batch * q * q, dtype=dt, device="cuda", generator=g)
    m = c.view(batch, q, q)
    m.add_(m.transpose(1, 2).clone())
    c.view(batch, q * q)[:, :: q + 1] += float(shift)
    return c


def agree(got, want, f64, what):
    tol = 1e-9 if f64 else 2e-3
    assert float((got - want).abs().max()) <= tol * max(float(want.abs().max()), 1.0), f"the routes disagree: {what}"


def run_colour(q, nsample, dt, batch, window):
    f64 = dt == torch.float64
    g = torch.Generator(device="cuda").manual_seed(q)
    c = spd(batch, q, dt, g, q)
    vm = torch.rand(batch * q, dtype=dt, device="cuda", generator=g)
    vz = torch.randn(batch * nsample * q, dtype=dt, device="cuda", generator=g)
    y = torch.empty_like(vz)
    fac = torch.empty_like(c)
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    c3, z3 = c.view(batch, q, q), vz.view(batch, nsample, q).transpose(1, 2)  # z3[k] = Z_k, q x S

    def torch_route():
        lo = torch.linalg.cholesky(c3)
        return lo, torch.baddbmm(vm.view(batch, q, 1), lo, z3)

    fns = {"colour": lambda: api.colour_batched(q, c, vm, vz, Y=y, L=fac, info=info), "torch": torch_route}
    row = {"what": "colour", "dtype": "f64" if f64 else "f32", "q": q, "nsample": nsample, "batch": batch}
    res = measure(fns, info, window)
    lo, yt = torch_route()
    agree(fac.view(batch, q, q).transpose(1, 2), lo, f64, "L")
    agree(y.view(batch, nsample, q).transpose(1, 2), yt, f64, "Y")
    del lo, yt
    kernels = {"colour": api.colour_kernel_name(api.F64 if f64 else api.F32, q), "torch": "torch.linalg.cholesky + torch.baddbmm"}
    for k in fns:
        row[k] = dict(res[k], kernel=kernels[k], per_s=batch / res[k]["ms"] * 1e3)
    row["ours_over_torch"] = row["colour"]["per_s"] / row["torch"]["per_s"]
    return row


def run_sample(n, nquery, nsample, dt, batch, window):
    f64 = dt == torch.float64
    code = api.F64 if f64 else api.F32
    g = torch.Generator(device="cuda").manual_seed(n + nquery)
    b = spd(batch, n, dt, g, n)
    vc, vd = (torch.rand(batch * n, dtype=dt, device="cuda", generator=g) for _ in range(2))
    va = torch.randn(batch * nquery * n, dtype=dt, device="cuda", generator=g)
    ve = spd(batch, nquery, dt, g, nquery + 8)  # well above a K a^T: the posterior covariance is positive definite
    vz = torch.randn(batch * nsample * nquery, dtype=dt, device="cuda", generator=g)
    y = torch.empty_like(vz)
    mean = torch.empty(batch * nquery, dtype=dt, device="cuda")
    cov = torch.empty(batch * nquery * nquery, dtype=dt, device="cuda")
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    z3 = vz.view(batch, nsample, nquery).transpose(1, 2)

    def torch_route():
        api.predict_cov_batched(n, b, vc, vd, va, ve, mean=mean, cov=cov, info=info)
        lo = torch.linalg.cholesky(cov.view(batch, nquery, nquery))
        return torch.baddbmm(mean.view(batch, nquery, 1), lo, z3)

    fns = {"sample": lambda: api.sample_batched(n, b, vc, vd, va, ve, vz, Y=y, info=info), "torch": torch_route}
    row = {"what": "sample", "dtype": "f64" if f64 else "f32", "n": n, "q": nquery, "nsample": nsample, "batch": batch}
    res = measure(fns, info, window)
    agree(y.view(batch, nsample, nquery).transpose(1, 2), torch_route(), f64, "Y")
    kernels = {"sample": api.predict_cov_kernel_name(code, n) + " + " + api.colour_kernel_name(code, nquery),
               "torch": api.predict_cov_kernel_name(code, n) + " + torch.linalg.cholesky + torch.baddbmm"}
    for k in fns:
        row[k] = dict(res[k], kernel=kernels[k], per_s=batch / res[k]["ms"] * 1e3)
    row["ours_over_torch"] = row["sample"]["per_s"] / row["torch"]["per_s"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="q = 64, S = 16 only, short windows (for profiling runs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_sample.py needs a GPU"
    torch.cuda.set_device(0)
    dts = (torch.float64, torch.float32)
    colour = [(q, s, dt) for dt in dts for q in (16, 32, 64, 96) for s in (16, 64)]
    sample = [(64, q, 16, dt) for dt in dts for q in (16, 64)]
    if args.quick:
        colour, sample, args.window = [(64, 16, dt) for dt in dts], [(64, 16, 16, dt) for dt in dts], min(args.window, 0.05)
    print("| what | dtype | n | q | S | ours /s | spread | torch route /s | spread | ours / torch route |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    rows = []
    jobs = [("colour", s) for s in colour] + [("sample", s) for s in sample]
    for what, shape in jobs:
        r = run_colour(*shape, args.batch, args.window) if what == "colour" else run_sample(*shape, args.batch, args.window)
        rows.append(r)
        print(f"| {what} | {r['dtype']} | {r.get('n', '')} | {r['q']} | {r['nsample']} | {r[what]['per_s']:.3e} | "
              f"{100 * r[what]['spread']:.1f} % | {r['torch']['per_s']:.3e} | {100 * r['torch']['spread']:.1f} % | "
              f"{r['ours_over_torch']:.2f} |", flush=True)
        if args.out:  # after every shape: a run cut short keeps what it measured
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "sample_times.json"), "w") as f:
                json.dump(rows, f, indent=1)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
