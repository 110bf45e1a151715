"""CPU-side checks of the batched log-determinant and log marginal likelihood (matinv_logdet_batched*, matinv_logml_batched*):
exports, argument errors, dispatch names. No GPU needed."""
import ctypes

import pytest

from conftest import pkg

NAMES = ["matinv_logdet_batched", "matinv_logdet_batched_ex", "matinv_logdet_kernel_name", "matinv_logdet_batched_host",
         "matinv_logml_batched", "matinv_logml_batched_host"]


def test_logdet_symbols_exported():
    lib = pkg("_lib")
    L = lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in lib.NATIVE_NAMES
    assert L.matinv_abi_version() == 2
    api = pkg("api")
    for name in ("logdet_batched", "logdet_batched_host", "logml_batched", "logml_batched_host", "logdet_kernel_name"):
        assert callable(getattr(api, name))


def test_logdet_argument_errors_without_device():
    lib = pkg("_lib")
    L = lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def logdet(algo=0, dtype=0, n=4, a=p, sa=16, out=p, sign=p, batch=2, kernel=0):
        return L.matinv_logdet_batched_ex(algo, dtype, n, a, sa, out, sign, batch, None, None, kernel)

    assert logdet(n=0) == lib.ERR_ARG
    assert b"n must be" in L.matinv_last_error()
    assert logdet(n=-3) == lib.ERR_ARG
    assert logdet(algo=5) == lib.ERR_ARG
    assert logdet(dtype=7) == lib.ERR_ARG
    assert logdet(kernel=42) == lib.ERR_ARG
    assert logdet(kernel=-1) == lib.ERR_ARG
    assert logdet(sa=15) == lib.ERR_ARG  # strideA < n*n
    assert b"stride" in L.matinv_last_error()
    assert logdet(a=None) == lib.ERR_ARG
    assert logdet(out=None) == lib.ERR_ARG
    # batch == 0 is a no-op even with NULL pointers; the other arguments are still checked
    assert logdet(a=None, out=None, sign=None, batch=0) == lib.OK
    assert logdet(a=None, out=None, sign=None, batch=0, algo=9) == lib.ERR_ARG
    assert L.matinv_logdet_batched(1, 1, 8, None, 0, None, None, 0, None, None) == lib.OK
    # n = 2000: unsupported -- and that verdict comes after the pointer checks, so it also shows that a NULL dSign is accepted
    assert logdet(n=2000, sa=4000000, batch=1) == lib.ERR_UNSUPPORTED
    assert logdet(n=2000, sa=4000000, batch=1, sign=None) == lib.ERR_UNSUPPORTED
    assert logdet(n=2000, sa=4000000, batch=1, out=None) == lib.ERR_ARG
    # a family without a logdet kernel, and the three with one outside their range: refused before any device call
    for kernel in (lib.KERNEL_LDS, lib.KERNEL_ROWLANE, lib.KERNEL_BLOCKED, lib.KERNEL_TILEP):
        assert logdet(kernel=kernel) == lib.ERR_UNSUPPORTED
    assert logdet(algo=lib.ALGO_GAUSS_JORDAN, kernel=lib.KERNEL_TILE) == lib.ERR_UNSUPPORTED
    assert logdet(algo=lib.ALGO_CHOLESKY, n=97, sa=97 * 97, kernel=lib.KERNEL_TILE) == lib.ERR_UNSUPPORTED
    assert logdet(algo=lib.ALGO_CHOLESKY, kernel=lib.KERNEL_ROW) == lib.ERR_UNSUPPORTED
    assert logdet(algo=lib.ALGO_GAUSS_JORDAN, n=65, sa=65 * 65, kernel=lib.KERNEL_ROW) == lib.ERR_UNSUPPORTED
    # host form: the same checks
    assert L.matinv_logdet_batched_host(0, 0, 0, p, p, p, 1, None) == lib.ERR_ARG
    assert L.matinv_logdet_batched_host(3, 0, 4, p, p, p, 1, None) == lib.ERR_ARG
    assert L.matinv_logdet_batched_host(0, 0, 4, None, p, p, 1, None) == lib.ERR_ARG
    assert L.matinv_logdet_batched_host(0, 0, 4, p, None, p, 1, None) == lib.ERR_ARG
    assert L.matinv_logdet_batched_host(0, 0, 4, None, None, None, 0, None) == lib.OK
    assert L.matinv_logdet_batched_host(0, 0, 2000, p, p, None, 1, None) == lib.ERR_UNSUPPORTED


def test_logml_argument_errors_without_device():
    lib = pkg("_lib")
    L = lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def logml(dtype=0, n=4, b=p, c=p, d=p, out=p, batch=2):
        return L.matinv_logml_batched(dtype, n, b, c, d, out, batch, None, None)

    assert logml(n=0) == lib.ERR_ARG
    assert logml(dtype=2) == lib.ERR_ARG
    assert logml(b=None) == lib.ERR_ARG
    assert logml(d=None) == lib.ERR_ARG
    assert logml(out=None) == lib.ERR_ARG
    assert logml(b=None, c=None, d=None, out=None, batch=0) == lib.OK
    assert logml(b=None, c=None, d=None, out=None, batch=0, dtype=5) == lib.ERR_ARG
    # n = 2000 is refused after the pointer checks: a NULL dCs passes them, a NULL dDs does not
    assert logml(n=2000, batch=1) == lib.ERR_UNSUPPORTED
    assert logml(n=2000, batch=1, c=None) == lib.ERR_UNSUPPORTED
    assert logml(n=2000, batch=1, d=None) == lib.ERR_ARG
    assert L.matinv_logml_batched_host(0, 0, p, p, p, p, 1, None) == lib.ERR_ARG
    assert L.matinv_logml_batched_host(0, 4, None, p, p, p, 1, None) == lib.ERR_ARG
    assert L.matinv_logml_batched_host(0, 4, p, p, None, p, 1, None) == lib.ERR_ARG
    assert L.matinv_logml_batched_host(0, 4, p, p, p, None, 1, None) == lib.ERR_ARG
    assert L.matinv_logml_batched_host(0, 4, None, None, None, None, 0, None) == lib.OK
    assert L.matinv_logml_batched_host(1, 2000, p, None, p, p, 1, None) == lib.ERR_UNSUPPORTED


SIZES = [1, 16, 17, 64, 65, 96, 97, 1024]


@pytest.mark.parametrize("f64", [True, False])
def test_logdet_dispatch_names(f64):
    api = pkg("api")
    dt, tname, cname = (api.F64, "f64", "double") if f64 else (api.F32, "f32", "float")
    GJ, CH = api.ALGO_GAUSS_JORDAN, api.ALGO_CHOLESKY
    glob_spd, glob_lu = f"matinv_logdet_global<{cname}, true>", f"matinv_logdet_global<{cname}, false>"
    for n in SIZES:
        nt, full = (n + 15) // 16, "true" if n % 16 == 0 else "false"
        tile = f"matinv_logdet_tile_{tname}<{nt}, {full}, false>"
        row = f"matinv_logdet_row<{cname}, {32 if n <= 32 else 64}>"
        # AUTO
        assert api.logdet_kernel_name(CH, dt, n) == (tile if n <= 96 else glob_spd), n
        assert api.logdet_kernel_name(GJ, dt, n) == (row if n <= 64 else glob_lu), n
        # forced families inside and outside their range
        assert api.logdet_kernel_name(CH, dt, n, api.KERNEL_TILE) == (tile if n <= 96 else ""), n
        assert api.logdet_kernel_name(GJ, dt, n, api.KERNEL_TILE) == "", n
        assert api.logdet_kernel_name(GJ, dt, n, api.KERNEL_ROW) == (row if n <= 64 else ""), n
        assert api.logdet_kernel_name(CH, dt, n, api.KERNEL_ROW) == "", n
        assert api.logdet_kernel_name(CH, dt, n, api.KERNEL_GLOBAL) == glob_spd, n
        assert api.logdet_kernel_name(GJ, dt, n, api.KERNEL_GLOBAL) == glob_lu, n
        for kernel in (api.KERNEL_LDS, api.KERNEL_ROWLANE, api.KERNEL_BLOCKED, api.KERNEL_TILEP, 42):
            assert api.logdet_kernel_name(CH, dt, n, kernel) == "", (n, kernel)
    for algo in (GJ, CH):
        assert api.logdet_kernel_name(algo, dt, 2000) == ""
        assert api.logdet_kernel_name(algo, dt, 1025, api.KERNEL_GLOBAL) == ""
        assert api.logdet_kernel_name(algo, dt, 0) == ""
    assert api.logdet_kernel_name(7, dt, 32) == ""
    assert api.logdet_kernel_name(CH, 9, 32) == ""


def test_logdet_host_forms_without_gpu_fail_loudly():
    import numpy as np
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    api = pkg("api")
    lib = pkg("_lib")
    a = np.eye(20).reshape(-1)
    d = np.ones(20)
    for call in (lambda: api.logdet_batched_host(a, 20, api.ALGO_CHOLESKY), lambda: api.logdet_batched_host(a, 20),
                 lambda: api.logml_batched_host(20, a, d, d), lambda: api.logml_batched_host(20, a, None, d)):
        with pytest.raises(lib.MatinvError) as e:
            call()
        assert e.value.code in (lib.ERR_NO_DEVICE, lib.ERR_HIP)
        assert lib.lib().matinv_last_error()
