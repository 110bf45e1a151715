#!/usr/bin/env python3
"""Time the Gauss-Jordan entry on a batch of R + n I matrices, 64 x 64 fp64: accepted by the natural order, NOT symmetric -- the batch
on which the symmetric-only kernel of the front route (csrc/tile_impl.hpp: launch_gj_tile_natural) is pure overhead.

    python tools/time_general64.py [batch] [reps]          (honors MATINV_LIB)

Reports, in one fresh process:
  first call   the first launch of the process: the front route (symmetric-only kernel, then the two-arm kernel over the whole batch)
               plus whatever a first launch costs (module load, scratch allocation); wall clock around launch + synchronise
  steady       launches 2 .. reps + 1: the direct route (the first launch found the batch not symmetric); median / min / max of event times
  probe        the next launch that takes the front route again (every 32nd in the direct state), by event time
and the sha256 of the last result, to compare libraries. A library without the front route prints the same lines (its launches are all
direct; "probe" is then just another launch)."""
import hashlib
import importlib
import sys
import time

import torch

sys.path.insert(0, '.')
api = importlib.import_module('cuda-matrix-inversion_amd.api')
n = 64
batch = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
assert reps <= 30, "the 32nd launch in the direct state probes the front route: keep the steady-state launches below it"
stats = getattr(api, 'sym_front_stats', None)
if stats is not None:
    try:
        stats()
    except AttributeError:  # a library from before the front route
        stats = None

torch.manual_seed(5)
a = (torch.rand((batch, n, n), dtype=torch.float64, device='cuda') + n * torch.eye(n, dtype=torch.float64, device='cuda')).reshape(-1).contiguous()
x = torch.empty_like(a)
torch.cuda.synchronize()


def route():
    if stats is None:
        return 'n/a'
    s = stats()
    return f"front {s['front_launches']} direct {s['direct_launches']} last not symmetric {s['last_not_symmetric']} of {s['last_batch']}"


def timed():
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    api.inverse_batched(a, n, api.ALGO_GAUSS_JORDAN, out=x)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


t0 = time.perf_counter()
api.inverse_batched(a, n, api.ALGO_GAUSS_JORDAN, out=x)
torch.cuda.synchronize()
print(f"first call  {1e3 * (time.perf_counter() - t0):.4f} ms (wall)   [{route()}]")
ms = sorted(timed() for _ in range(reps))
print(f"steady      median {ms[len(ms) // 2]:.4f} ms min {ms[0]:.4f} max {ms[-1]:.4f}  ({reps} launches)   [{route()}]")
probe = None
for k in range(reps + 1, 40):
    before = stats()['front_launches'] if stats is not None else 0
    t = timed()
    if stats is None or stats()['front_launches'] != before:
        probe = (k, t)
        break
print(f"probe       launch {probe[0] + 1} of the process: {probe[1]:.4f} ms   [{route()}]" if probe else "probe       none within 40 launches")
print(f"sha {hashlib.sha256(x.cpu().numpy().tobytes()).hexdigest()[:16]}")
