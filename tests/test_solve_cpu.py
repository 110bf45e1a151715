"""CPU-side checks of the batched linear solve (matinv_solve_batched*): exports, argument errors, dispatch names. No GPU needed."""
import ctypes

import pytest

from conftest import pkg

SOLVE_NAMES = ["matinv_solve_batched", "matinv_solve_batched_ex", "matinv_solve_kernel_name", "matinv_solve_batched_host"]


def test_solve_symbols_exported():
    lib = pkg("_lib")
    L = lib.lib()
    for name in SOLVE_NAMES:
        assert hasattr(L, name), name
        assert name in lib.NATIVE_NAMES


def test_solve_argument_errors_without_device():
    lib = pkg("_lib")
    L = lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def solve(algo=0, dtype=0, n=4, nrhs=1, a=p, sa=16, b=p, sb=4, x=p, sx=4, batch=2, kernel=0):
        return L.matinv_solve_batched_ex(algo, dtype, n, nrhs, a, sa, b, sb, x, sx, batch, None, None, kernel)

    assert solve(n=0) == lib.ERR_ARG
    assert b"n must be" in L.matinv_last_error()
    assert solve(nrhs=0) == lib.ERR_ARG
    assert b"nrhs" in L.matinv_last_error()
    assert solve(algo=5) == lib.ERR_ARG
    assert solve(dtype=7) == lib.ERR_ARG
    assert solve(kernel=42) == lib.ERR_ARG
    assert solve(sa=15) == lib.ERR_ARG          # strideA < n*n
    assert solve(sb=3) == lib.ERR_ARG           # strideB < n*nrhs
    assert solve(nrhs=2, sb=8, sx=7) == lib.ERR_ARG
    assert solve(a=None) == lib.ERR_ARG
    assert solve(b=None) == lib.ERR_ARG
    assert solve(x=None) == lib.ERR_ARG
    # an empty batch is a no-op before any device call, null pointers included
    assert solve(a=None, b=None, x=None, batch=0) == lib.OK
    assert L.matinv_solve_batched(0, 0, 8, 3, None, 0, None, 0, None, 0, 0, None, None) == lib.OK
    assert L.matinv_solve_batched(0, 0, 2000, 1, p, 4000000, p, 2000, p, 2000, 1, None, None) == lib.ERR_UNSUPPORTED
    # host form: the same checks
    assert L.matinv_solve_batched_host(0, 0, 0, 1, p, p, p, 1, None) == lib.ERR_ARG
    assert L.matinv_solve_batched_host(0, 0, 4, 0, p, p, p, 1, None) == lib.ERR_ARG
    assert L.matinv_solve_batched_host(0, 0, 4, 1, None, p, p, 1, None) == lib.ERR_ARG
    assert L.matinv_solve_batched_host(0, 0, 4, 1, None, None, None, 0, None) == lib.OK


@pytest.mark.parametrize("f64", [True, False])
@pytest.mark.parametrize("algo", [0, 1])
def test_solve_dispatch_names(f64, algo):
    api = pkg("api")
    dt = api.F64 if f64 else api.F32
    tname = "f64" if f64 else "f32"
    spd = "true" if algo == api.ALGO_CHOLESKY else "false"
    for n in (17, 33, 64):
        nt, full = (n + 15) // 16, "true" if n % 16 == 0 else "false"
        for nrhs in (1, 16):
            want = f"matinv_solve_tile_{tname}<{nt}, {full}, {spd}>"
            assert api.solve_kernel_name(algo, dt, n, nrhs) == want
            assert api.solve_kernel_name(algo, dt, n, nrhs, api.KERNEL_TILE) == want
    # the composed path: the inverse's kernel of the family that does the inversion
    for n, nrhs in ((16, 1), (65, 1), (200, 3), (32, 17), (64, 17), (5, 40)):
        assert api.solve_kernel_name(algo, dt, n, nrhs) == api.kernel_name(algo, dt, n), (n, nrhs)
        assert api.solve_kernel_name(algo, dt, n, nrhs, api.KERNEL_TILE) == ""   # fused path: out of range
    assert api.solve_kernel_name(algo, dt, 32, 4, api.KERNEL_LDS) == api.kernel_name(algo, dt, 32, api.KERNEL_LDS)
    assert api.solve_kernel_name(algo, dt, 2000, 1) == ""
    assert api.solve_kernel_name(algo, dt, 32, 0) == ""


def test_solve_tile_outside_range_is_unsupported():
    lib = pkg("_lib")
    L = lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for n, nrhs in ((16, 1), (65, 1), (32, 17), (8, 2)):
        rc = L.matinv_solve_batched_ex(0, 0, n, nrhs, p, n * n, p, n * nrhs, p, n * nrhs, 1, None, None, lib.KERNEL_TILE)
        assert rc == lib.ERR_UNSUPPORTED, (n, nrhs)


def test_solve_pivot_policy_names_the_row_solve():
    api = pkg("api")
    old = api.set_gj_policy(api.GJ_PIVOT)
    try:
        assert api.solve_kernel_name(api.ALGO_GAUSS_JORDAN, api.F64, 64, 1) == "matinv_solve_row<double, 64, 4>"
        assert api.solve_kernel_name(api.ALGO_GAUSS_JORDAN, api.F32, 20, 16) == "matinv_solve_row<float, 32, 16>"
        # Cholesky and an explicit TILE request keep the fused kernel; outside the fused range the composed path follows the policy
        assert api.solve_kernel_name(api.ALGO_CHOLESKY, api.F64, 64, 1) == "matinv_solve_tile_f64<4, true, true>"
        assert api.solve_kernel_name(api.ALGO_GAUSS_JORDAN, api.F64, 64, 1, api.KERNEL_TILE) == "matinv_solve_tile_f64<4, true, false>"
        assert api.solve_kernel_name(api.ALGO_GAUSS_JORDAN, api.F64, 100, 1) == api.kernel_name(api.ALGO_GAUSS_JORDAN, api.F64, 100)
    finally:
        api.set_gj_policy(old)


def test_solve_host_without_gpu_fails_loudly():
    import numpy as np
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    api = pkg("api")
    lib = pkg("_lib")
    a = np.eye(20).reshape(-1)
    b = np.ones(20)
    with pytest.raises(lib.MatinvError) as e:
        api.solve_batched_host(a, b, 20, 1)
    assert e.value.code in (lib.ERR_NO_DEVICE, lib.ERR_HIP)
    assert lib.lib().matinv_last_error()
