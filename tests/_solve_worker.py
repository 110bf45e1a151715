"""Worker of tests/test_gpu_solve.py for the checks that need an environment set before the library is loaded (it reads its
switches once per process). Usage: _solve_worker.py chunk OUT.npz | rejects. Prints `solve-worker ok`, or raises."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import general_batch, spd_batch  # noqa: E402

api = importlib.import_module("cuda-matrix-inversion_amd.api")


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def solve(a, b, n, nrhs, algo, kernel=api.KERNEL_AUTO):
    batch = a.size // (n * n)
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    x = api.solve_batched(dev(a), dev(b), n, nrhs, algo, info=info, kernel=kernel)
    torch.cuda.synchronize()
    return x.cpu().numpy(), info.cpu().numpy()


def chunk_cases():
    """(name, n, nrhs, algo, kernel, batch) of the composed path; the same list runs in the parent without the switch"""
    return [("gj100", 100, 3, api.ALGO_GAUSS_JORDAN, api.KERNEL_AUTO, 40), ("ch100", 100, 2, api.ALGO_CHOLESKY, api.KERNEL_AUTO, 40),
            ("gj16", 16, 5, api.ALGO_GAUSS_JORDAN, api.KERNEL_AUTO, 9000), ("lds48", 48, 17, api.ALGO_GAUSS_JORDAN, api.KERNEL_LDS, 700)]


def chunk_inputs(n, nrhs, batch):
    a = spd_batch(n, batch, seed=n + nrhs)
    b = np.random.default_rng(n * nrhs).standard_normal(batch * n * nrhs)
    return a, b


def run_chunk(out):
    res = {}
    for name, n, nrhs, algo, kernel, batch in chunk_cases():
        a, b = chunk_inputs(n, nrhs, batch)
        res[name], info = solve(a, b, n, nrhs, algo, kernel)
        assert not info.any(), name
    np.savez(out, **res)


def run_rejects():
    assert os.environ.get("MATINV_DEBUG_REJECTS") == "1"
    n = 64
    for algo in (api.ALGO_GAUSS_JORDAN, api.ALGO_CHOLESKY):
        for dtype in (np.float64, np.float32):
            a = spd_batch(n, 4096, seed=11, dtype=dtype)
            b = np.random.default_rng(12).random(4096 * n * 4).astype(dtype)
            api.debug_rejects(reset=True)
            _, info = solve(a, b, n, 4, algo)
            assert not info.any()
            got = api.debug_rejects()
            assert got == 0, (algo, dtype, got)
    for n in (33, 64):
        g = general_batch(n, 300, seed=13)
        b = np.random.default_rng(14).random(300 * n)
        api.debug_rejects(reset=True)
        x, info = solve(g, b, n, 1, api.ALGO_GAUSS_JORDAN)
        got = api.debug_rejects()
        assert got > 0, (n, got)
        want = np.linalg.solve(g.reshape(-1, n, n).transpose(0, 2, 1), b.reshape(-1, n, 1))
        assert np.abs(x.reshape(-1, n, 1) - want).max() / np.abs(want).max() < 1e-8
        print(f"n={n}: {got} of 300 general matrices went to the row solve")


if __name__ == "__main__":
    torch.cuda.set_device(0)
    if sys.argv[1] == "chunk":
        run_chunk(sys.argv[2])
    elif sys.argv[1] == "rejects":
        run_rejects()
    else:
        raise SystemExit(f"unknown check {sys.argv[1]}")
    print("solve-worker ok")
