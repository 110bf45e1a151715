"""CPU-side checks of the batched leave-one-out cross-validation (matinv_loo_batched*): exports, argument errors, dispatch names, and
the audit of the compiled LOO kernel forms that the generated instantiation sweep cannot make (tests/_instantiations.py has no `loo`
route: the forms carry the names of the SPD inversion kernels with one more template argument). No GPU needed."""
import ctypes
import re

import pytest

import test_instantiations_cpu as audit
from conftest import pkg

NAMES = ["matinv_loo_batched", "matinv_loo_kernel_name", "matinv_loo_batched_host"]


def test_loo_symbols_exported():
    lib = pkg("_lib")
    L = lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in lib.NATIVE_NAMES
    assert L.matinv_abi_version() == 2
    api = pkg("api")
    for name in ("loo_batched", "loo_batched_host", "loo_kernel_name"):
        assert callable(getattr(api, name))


def test_loo_argument_errors_without_device():
    lib = pkg("_lib")
    L = lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def loo(dtype=0, n=4, b=p, c=p, d=p, mean=p, var=p, logpl=p, batch=2):
        return L.matinv_loo_batched(dtype, n, b, c, d, mean, var, logpl, batch, None, None)

    def host(dtype=0, n=4, b=p, c=p, d=p, mean=p, var=p, logpl=p, batch=2):
        return L.matinv_loo_batched_host(dtype, n, b, c, d, mean, var, logpl, batch, None)

    for f in (loo, host):
        assert f(n=0) == lib.ERR_ARG
        assert b"n must be" in L.matinv_last_error()
        assert f(n=-2) == lib.ERR_ARG
        assert f(dtype=2) == lib.ERR_ARG
        assert f(b=None) == lib.ERR_ARG
        assert f(d=None) == lib.ERR_ARG
        assert f(mean=None, var=None, logpl=None) == lib.ERR_ARG
        assert b"output" in L.matinv_last_error()
        # batch == 0 is a no-op even with NULL pointers; n and dtype are still checked
        assert f(b=None, c=None, d=None, mean=None, var=None, logpl=None, batch=0) == lib.OK
        assert f(b=None, c=None, d=None, mean=None, var=None, logpl=None, batch=0, dtype=5) == lib.ERR_ARG
        assert f(b=None, c=None, d=None, mean=None, var=None, logpl=None, batch=0, n=0) == lib.ERR_ARG
        # n = 2000 is refused after the pointer checks: any single output passes them, and so does a NULL c
        assert f(n=2000, batch=1) == lib.ERR_UNSUPPORTED
        assert f(n=2000, batch=1, var=None, logpl=None) == lib.ERR_UNSUPPORTED
        assert f(n=2000, batch=1, mean=None, logpl=None) == lib.ERR_UNSUPPORTED
        assert f(n=2000, batch=1, mean=None, var=None) == lib.ERR_UNSUPPORTED
        assert f(n=2000, batch=1, c=None) == lib.ERR_UNSUPPORTED
        assert f(n=2000, batch=1, mean=None, var=None, logpl=None) == lib.ERR_ARG
        assert f(n=2000, batch=1, d=None) == lib.ERR_ARG
    assert loo(batch=0x80000000) == lib.ERR_ARG
    assert b"batch" in L.matinv_last_error()


@pytest.mark.parametrize("f64", [True, False])
def test_loo_dispatch_names(f64):
    api = pkg("api")
    dt, t, c = (api.F64, "f64", "double") if f64 else (api.F32, "f32", "float")
    assert api.loo_kernel_name(dt, 1) == f"matinv_spd_tile_{t}<1, false, true>"
    assert api.loo_kernel_name(dt, 15) == f"matinv_spd_tile_{t}<1, false, true>"
    assert api.loo_kernel_name(dt, 16) == f"matinv_spd_tile_{t}<1, true, true>"
    assert api.loo_kernel_name(dt, 17) == f"matinv_spd_tile_{t}<2, false, true>"
    assert api.loo_kernel_name(dt, 96) == f"matinv_spd_tile_{t}<6, true, true>"
    assert api.loo_kernel_name(dt, 97) == f"matinv_chol_global<{c}, true>"
    assert api.loo_kernel_name(dt, 1024) == f"matinv_chol_global<{c}, true>"
    assert api.loo_kernel_name(dt, 0) == "" == api.loo_kernel_name(dt, 1025)
    assert api.loo_kernel_name(9, 32) == "" == api.loo_kernel_name(-1, 200)


def test_loo_host_form_without_gpu_fails_loudly():
    import numpy as np
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    api = pkg("api")
    lib = pkg("_lib")
    a = np.eye(20).reshape(-1)
    d = np.ones(20)
    for call in (lambda: api.loo_batched_host(20, a, d, d), lambda: api.loo_batched_host(20, a, None, d)):
        with pytest.raises(lib.MatinvError) as e:
            call()
        assert e.value.code in (lib.ERR_NO_DEVICE, lib.ERR_HIP)
        assert lib.lib().matinv_last_error()


LOO_FORMS = (r"matinv_spd_tile_f(64|32)<\d+, (true|false), true>", r"matinv_chol_global<(double|float), true>")


@pytest.mark.skipif(audit.NM is None, reason="no nm on this machine")
def test_every_loo_name_is_a_compiled_kernel_and_every_loo_form_is_named():
    """what test_instantiations_cpu checks for the routes of the generated sweep, for the LOO forms: exact names, both directions"""
    api = pkg("api")
    named = {api.loo_kernel_name(dt, n) for dt in (api.F64, api.F32) for n in range(1, 1025)}
    assert "" not in named and len(named) == 2 * (12 + 1)
    missing = sorted(named - audit.STUBS)
    assert not missing, f"named by matinv_loo_kernel_name but not compiled: {missing}"
    compiled = {s for s in audit.STUBS if any(re.fullmatch(p, s) for p in LOO_FORMS)}
    assert compiled, "no LOO form is compiled"
    assert not sorted(compiled - named), f"compiled LOO forms no n reaches: {sorted(compiled - named)}"
