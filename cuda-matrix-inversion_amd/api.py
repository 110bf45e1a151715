"""Host-side mirror of the reference's operator interface for the inversion hot path, over the C ABI.

Names, argument order and meaning follow /root/reference/include/inverse_gpu.h:7-31 (``handle`` dropped: the
reference's hand-written kernels ignore it) and src/gauss_bench.cu:127,275 (calcluateMean / calcluateVariance --
the reference's spelling is kept). Two layers:

* host-pointer family ``*_batched_gpu(n, As, aInvs, batchSize)`` on numpy arrays: calls the identically named
  C symbol (H2D + kernel + D2H inside, synchronous), exactly what ``inverse_bench`` times;
* device family on torch CUDA tensors: ``inverse_batched`` / ``mean_batched`` / ``variance_batched`` / ``solve_batched``
  call the native ``matinv_*`` entry points on torch's current stream with no copies.

A batch is flat memory: matrix k occupies ``[k*n*n, (k+1)*n*n)``, column-major (element (r, c) at c*n + r).
torch is used for device memory and streams only; all arithmetic runs in libmatinv_hip.so.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import (GJ_ADAPTIVE, GJ_NATURAL_FIRST, GJ_PIVOT,  # noqa: F401
                   ALGO_CHOLESKY, ALGO_GAUSS_JORDAN, F32, F64, KERNEL_AUTO, KERNEL_BLOCKED, KERNEL_GLOBAL, KERNEL_LDS,  # noqa: F401
                   KERNEL_ROW, KERNEL_ROWLANE, KERNEL_TILE, KERNEL_TILEP, COV_MATERN52, COV_SE, MatinvError)


def _np_dtype_code(dtype) -> int:
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        return F64
    if dtype == np.float32:
        return F32
    raise TypeError(f"only float32/float64 batches are supported, got {dtype}")


def _torch_dtype_code(t) -> int:
    import torch
    if t.dtype == torch.float64:
        return F64
    if t.dtype == torch.float32:
        return F32
    raise TypeError(f"only float32/float64 batches are supported, got {t.dtype}")


def _dtype_code(dtype) -> int:
    """the *_kernel_name wrappers take a library dtype code or anything numpy reads as a dtype"""
    return dtype if isinstance(dtype, int) else _np_dtype_code(dtype)


def _tensor_ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _array_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _check_info(info, batch, name="batchSize"):
    import torch
    if info is not None and (info.dtype != torch.int32 or info.numel() < batch):
        raise ValueError(f"info must be an int32 tensor with at least `{name}` elements")


# ---------------------------------------------------------------------------------------------- host family
def _call_reference_gpu(name: str, n: int, As: np.ndarray, aInvs: np.ndarray, batchSize: int) -> None:
    if not (isinstance(As, np.ndarray) and isinstance(aInvs, np.ndarray)):
        raise TypeError("host-pointer family takes numpy arrays")
    if As.dtype != aInvs.dtype or not As.flags.c_contiguous or not aInvs.flags.c_contiguous:
        raise ValueError("As and aInvs must be C-contiguous arrays of one dtype")
    if As.size < batchSize * n * n or aInvs.size < batchSize * n * n:
        raise ValueError("array smaller than batchSize*n*n")
    suffix = "" if _np_dtype_code(As.dtype) == F64 else "_f32"
    fn = getattr(_lib.lib(), name + suffix)
    fn(None, int(n), As.ctypes.data_as(ctypes.c_void_p), aInvs.ctypes.data_as(ctypes.c_void_p), int(batchSize))


def inverse_gauss_batched_gpu(n, As, aInvs, batchSize):
    """inverse_gpu.h:7 / src/gauss/batched_invert.cu:99."""
    _call_reference_gpu("inverse_gauss_batched_gpu", n, As, aInvs, batchSize)


def inverse_lu_cuda_batched_gpu(n, As, aInvs, batchSize):
    """inverse_gpu.h:8 / src/gauss/inverse_gpu.cu:60 (served by the pivoted Gauss-Jordan kernel)."""
    _call_reference_gpu("inverse_lu_cuda_batched_gpu", n, As, aInvs, batchSize)


def inverse_cholesky_batched_gpu(n, As, aInvs, batchSize):
    """inverse_gpu.h:27 / src/inverse_cholesky_gpu.cu:397. As is NOT clobbered (the reference does, :442)."""
    _call_reference_gpu("inverse_cholesky_batched_gpu", n, As, aInvs, batchSize)


def inverse_cholesky_mm_batched_gpu(n, As, aInvs, batchSize):
    _call_reference_gpu("inverse_cholesky_mm_batched_gpu", n, As, aInvs, batchSize)


def inverse_cholesky_mm2_batched_gpu(n, As, aInvs, batchSize):
    _call_reference_gpu("inverse_cholesky_mm2_batched_gpu", n, As, aInvs, batchSize)


def inverse_cholesky_stride_batched_gpu(n, As, aInvs, batchSize):
    _call_reference_gpu("inverse_cholesky_stride_batched_gpu", n, As, aInvs, batchSize)


def inverse_batched_host(As: np.ndarray, n: int, algo: int = ALGO_GAUSS_JORDAN):
    """matinv_inverse_batched_host: returns (aInvs, info) for a numpy batch."""
    As = np.ascontiguousarray(As)
    batch = As.size // (n * n)
    out = np.empty_like(As)
    info = np.zeros(batch, dtype=np.int32)
    _lib.check(_lib.lib().matinv_inverse_batched_host(
        algo, _np_dtype_code(As.dtype), n, As.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p),
        batch, info.ctypes.data_as(ctypes.c_void_p)))
    return out, info


def inverse_batched_host_multi(As: np.ndarray, n: int, algo: int = ALGO_GAUSS_JORDAN, nshards: int = 0):
    """matinv_inverse_batched_host_multi: the batch block-partitioned over `nshards` shards (0 = one per visible device),
    one host thread and one device per shard, results back in host memory; no collective. Returns (aInvs, info)."""
    As = np.ascontiguousarray(As)
    batch = As.size // (n * n)
    out = np.empty_like(As)
    info = np.zeros(batch, dtype=np.int32)
    _lib.check(_lib.lib().matinv_inverse_batched_host_multi(
        algo, _np_dtype_code(As.dtype), n, As.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p),
        batch, info.ctypes.data_as(ctypes.c_void_p), int(nshards)))
    return out, info


def device_count() -> int:
    k = _lib.lib().matinv_device_count()
    if k < 0:
        _lib.check(k)
    return k


def debug_rejects(reset: bool = False) -> int:
    """matinv_debug_rejects: matrices the first-pass kernels handed to a fallback since the last reset (needs
    MATINV_DEBUG_REJECTS=1 in the environment before the library is loaded; otherwise 0)."""
    return int(_lib.lib().matinv_debug_rejects(1 if reset else 0))


def set_gj_policy(policy: int) -> int:
    """matinv_set_gj_policy (GJ_NATURAL_FIRST / GJ_PIVOT / GJ_ADAPTIVE); returns the previous policy."""
    old = _lib.lib().matinv_set_gj_policy(int(policy))
    if old < 0:
        _lib.check(old)
    return old


# -------------------------------------------------------------------------------------------- device family
def _stream_ptr(t):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _require_cuda(*tensors):
    for t in tensors:
        if t is not None and not (t.is_cuda and t.is_contiguous()):
            raise ValueError("device family takes contiguous CUDA tensors")


def inverse_batched(As, n: int, algo: int = ALGO_GAUSS_JORDAN, out=None, info=None, kernel: int = KERNEL_AUTO,
                    batch: int | None = None, stride: int | None = None):
    """Invert a device-resident batch on torch's current stream (asynchronous).

    As: CUDA tensor holding `batch` matrices, matrix k at element offset k*stride (default n*n).
    out: optional result tensor of the same layout (allocated when None). info: optional int32[batch] tensor.
    Returns out.
    """
    import torch
    _require_cuda(As, out, info)
    stride = n * n if stride is None else int(stride)
    if batch is None:
        batch = As.numel() // stride
    if out is None:
        out = torch.empty_like(As)
    if out.dtype != As.dtype:
        raise TypeError("out dtype differs from input dtype")
    _check_info(info, batch, "batch")
    with torch.cuda.device(As.device):
        _lib.check(_lib.lib().matinv_inverse_batched_ex(
            algo, _torch_dtype_code(As), n, ctypes.c_void_p(As.data_ptr()), stride, ctypes.c_void_p(out.data_ptr()),
            stride, batch, ctypes.c_void_p(info.data_ptr()) if info is not None else None, _stream_ptr(As), kernel))
    return out


def inverse_gauss_batched_device(n, devAs, devAInvs, batchSize):
    """inverse_gpu.h:10 (declared there, never defined in the reference): Gauss-Jordan on device-resident batches."""
    return inverse_batched(devAs, n, ALGO_GAUSS_JORDAN, out=devAInvs, batch=batchSize)


def inverse_lu_cuda_batched_device(n, devAs, devAInvs, batchSize):
    """inverse_gpu.h:11 / src/gauss/inverse_gpu.cu:16 -- the dispatch point of gauss_bench's batchedInverse (:68-78)."""
    return inverse_batched(devAs, n, ALGO_GAUSS_JORDAN, out=devAInvs, batch=batchSize)


def inverse_cholesky_batched_device(n, devAs, devAInvs, batchSize):
    """inverse_gpu.h:20 / src/inverse_cholesky_gpu.cu:323."""
    return inverse_batched(devAs, n, ALGO_CHOLESKY, out=devAInvs, batch=batchSize)


def calcluateMean(n, As, Bs, Cs, Ds, Means=None, batchSize=None, info=None):
    """means[k] = a_k^T (B_k + diag c_k)^-1 d_k on device tensors (src/gauss_bench.cu:127-265; reference spelling).
    Unlike the reference CPU path (gauss_cpu.h:42) no input is destroyed."""
    import torch
    _require_cuda(As, Bs, Cs, Ds, Means, info)
    if batchSize is None:
        batchSize = Bs.numel() // (n * n)
    if Means is None:
        Means = torch.empty(batchSize, dtype=Bs.dtype, device=Bs.device)
    with torch.cuda.device(Bs.device):
        _lib.check(_lib.lib().matinv_mean_batched(
            _torch_dtype_code(Bs), n, ctypes.c_void_p(As.data_ptr()), ctypes.c_void_p(Bs.data_ptr()),
            ctypes.c_void_p(Cs.data_ptr()), ctypes.c_void_p(Ds.data_ptr()), ctypes.c_void_p(Means.data_ptr()),
            batchSize, ctypes.c_void_p(info.data_ptr()) if info is not None else None, _stream_ptr(Bs)))
    return Means


def calcluateVariance(n, As, Bs, Cs, Es, Variances=None, batchSize=None, info=None):
    """vars[k] = e_k - a_k^T (B_k + diag c_k)^-1 a_k (src/gauss_bench.cu:275-409; documented sign, gauss_cpu.h:34)."""
    import torch
    _require_cuda(As, Bs, Cs, Es, Variances, info)
    if batchSize is None:
        batchSize = Bs.numel() // (n * n)
    if Variances is None:
        Variances = torch.empty(batchSize, dtype=Bs.dtype, device=Bs.device)
    with torch.cuda.device(Bs.device):
        _lib.check(_lib.lib().matinv_variance_batched(
            _torch_dtype_code(Bs), n, ctypes.c_void_p(As.data_ptr()), ctypes.c_void_p(Bs.data_ptr()),
            ctypes.c_void_p(Cs.data_ptr()), ctypes.c_void_p(Es.data_ptr()), ctypes.c_void_p(Variances.data_ptr()),
            batchSize, ctypes.c_void_p(info.data_ptr()) if info is not None else None, _stream_ptr(Bs)))
    return Variances


def solve_batched(A, B, n: int, nrhs: int, algo: int = ALGO_GAUSS_JORDAN, info=None, out=None, kernel: int = KERNEL_AUTO,
                  batch: int | None = None, strideA: int | None = None, strideB: int | None = None, strideX: int | None = None):
    """X_k = A_k^-1 B_k on device tensors, torch's current stream, no copies (matinv_solve_batched_ex; asynchronous).

    A: `batch` n x n matrices, column-major, matrix k at element k*strideA (default n*n). B: n x nrhs column-major (column r
    at r*n), matrix k at k*strideB (default n*nrhs). out: X in B's layout with strideX (default strideB); may be B itself
    (solved in place); allocated when None. info: optional int32[batch]. ALGO_CHOLESKY reads A's lower triangle only.
    Returns out.
    """
    import torch
    _require_cuda(A, B, out, info)
    strideA = n * n if strideA is None else int(strideA)
    strideB = n * nrhs if strideB is None else int(strideB)
    if batch is None:
        batch = A.numel() // strideA
    if out is None:
        out = torch.empty_like(B)
    strideX = strideB if strideX is None else int(strideX)
    if A.dtype != B.dtype or out.dtype != B.dtype:
        raise TypeError("A, B and out must have one dtype")
    _check_info(info, batch, "batch")
    with torch.cuda.device(A.device):
        _lib.check(_lib.lib().matinv_solve_batched_ex(
            algo, _torch_dtype_code(A), n, nrhs, ctypes.c_void_p(A.data_ptr()), strideA, ctypes.c_void_p(B.data_ptr()), strideB,
            ctypes.c_void_p(out.data_ptr()), strideX, batch, ctypes.c_void_p(info.data_ptr()) if info is not None else None,
            _stream_ptr(A), kernel))
    return out


def solve_batched_host(As: np.ndarray, Bs: np.ndarray, n: int, nrhs: int, algo: int = ALGO_GAUSS_JORDAN):
    """matinv_solve_batched_host on numpy batches (packed, column-major): returns (X, info). Synchronous."""
    As = np.ascontiguousarray(As)
    Bs = np.ascontiguousarray(Bs)
    if As.dtype != Bs.dtype:
        raise TypeError("As and Bs must have one dtype")
    batch = As.size // (n * n)
    if Bs.size < batch * n * nrhs:
        raise ValueError("Bs smaller than batch*n*nrhs")
    out = np.empty_like(Bs)
    info = np.zeros(batch, dtype=np.int32)
    _lib.check(_lib.lib().matinv_solve_batched_host(
        algo, _np_dtype_code(As.dtype), n, nrhs, As.ctypes.data_as(ctypes.c_void_p), Bs.ctypes.data_as(ctypes.c_void_p),
        out.ctypes.data_as(ctypes.c_void_p), batch, info.ctypes.data_as(ctypes.c_void_p)))
    return out, info


def solve_kernel_name(algo: int, dtype, n: int, nrhs: int, kernel: int = KERNEL_AUTO) -> str:
    """matinv_solve_kernel_name: the first kernel a solve request launches ("" when the request would be refused)."""
    code = _dtype_code(dtype)
    return _lib.lib().matinv_solve_kernel_name(algo, code, n, nrhs, kernel).decode()


def logdet_batched(A, n: int, algo: int = ALGO_GAUSS_JORDAN, sign=None, out=None, info=None, kernel: int = KERNEL_AUTO,
                   batch: int | None = None, stride: int | None = None):
    """sign_k * exp(logabsdet_k) = det A_k on device tensors, torch's current stream, no copies (matinv_logdet_batched_ex; asynchronous).

    A: `batch` n x n matrices, column-major, matrix k at element k*stride (default n*n). ALGO_CHOLESKY reads the lower triangle only
    (SPD input, sign +1); ALGO_GAUSS_JORDAN serves general matrices. sign, out: optional result tensors of A's dtype with at least
    `batch` elements (allocated when None; elements beyond `batch` are left alone). info: optional int32[batch].
    Returns (sign, logabsdet).
    """
    import torch
    _require_cuda(A, sign, out, info)
    stride = n * n if stride is None else int(stride)
    if batch is None:
        batch = A.numel() // stride
    if out is None:
        out = torch.empty(batch, dtype=A.dtype, device=A.device)
    if sign is None:
        sign = torch.empty(batch, dtype=A.dtype, device=A.device)
    if out.dtype != A.dtype or sign.dtype != A.dtype:
        raise TypeError("sign and out must have the dtype of A")
    if out.numel() < batch or sign.numel() < batch:
        raise ValueError("sign and out need at least `batch` elements")
    _check_info(info, batch, "batch")
    with torch.cuda.device(A.device):
        _lib.check(_lib.lib().matinv_logdet_batched_ex(
            algo, _torch_dtype_code(A), n, ctypes.c_void_p(A.data_ptr()), stride, ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(sign.data_ptr()), batch, ctypes.c_void_p(info.data_ptr()) if info is not None else None,
            _stream_ptr(A), kernel))
    return sign, out


def logdet_batched_host(As: np.ndarray, n: int, algo: int = ALGO_GAUSS_JORDAN):
    """matinv_logdet_batched_host on a numpy batch (packed, column-major): returns (sign, logabsdet, info). Synchronous."""
    As = np.ascontiguousarray(As)
    batch = As.size // (n * n)
    sign = np.empty(batch, dtype=As.dtype)
    out = np.empty(batch, dtype=As.dtype)
    info = np.zeros(batch, dtype=np.int32)
    _lib.check(_lib.lib().matinv_logdet_batched_host(
        algo, _np_dtype_code(As.dtype), n, As.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p),
        sign.ctypes.data_as(ctypes.c_void_p), batch, info.ctypes.data_as(ctypes.c_void_p)))
    return sign, out, info


def logml_batched(n, Bs, Cs, Ds, out=None, batchSize=None, info=None):
    """logml[k] = -1/2 d_k^T M_k^-1 d_k - 1/2 log det M_k - n/2 log(2 pi), M_k = B_k + diag c_k, on device tensors
    (matinv_logml_batched; asynchronous on torch's current stream). Cs may be None (M = B). Only B's lower triangle is read and
    no input is modified. Returns out."""
    import torch
    _require_cuda(Bs, Cs, Ds, out, info)
    if batchSize is None:
        batchSize = Bs.numel() // (n * n)
    if out is None:
        out = torch.empty(batchSize, dtype=Bs.dtype, device=Bs.device)
    if Ds.dtype != Bs.dtype or out.dtype != Bs.dtype or (Cs is not None and Cs.dtype != Bs.dtype):
        raise TypeError("Bs, Cs, Ds and out must have one dtype")
    if Ds.numel() < batchSize * n or out.numel() < batchSize or (Cs is not None and Cs.numel() < batchSize * n):
        raise ValueError("Cs and Ds need batchSize*n elements, out batchSize")
    _check_info(info, batchSize)
    with torch.cuda.device(Bs.device):
        _lib.check(_lib.lib().matinv_logml_batched(
            _torch_dtype_code(Bs), n, ctypes.c_void_p(Bs.data_ptr()), ctypes.c_void_p(Cs.data_ptr()) if Cs is not None else None,
            ctypes.c_void_p(Ds.data_ptr()), ctypes.c_void_p(out.data_ptr()), batchSize,
            ctypes.c_void_p(info.data_ptr()) if info is not None else None, _stream_ptr(Bs)))
    return out


def logml_batched_host(n, Bs: np.ndarray, Cs, Ds: np.ndarray):
    """matinv_logml_batched_host on numpy batches (packed; Cs may be None): returns (logml, info). Synchronous."""
    Bs = np.ascontiguousarray(Bs)
    Ds = np.ascontiguousarray(Ds)
    Cs = None if Cs is None else np.ascontiguousarray(Cs)
    if Ds.dtype != Bs.dtype or (Cs is not None and Cs.dtype != Bs.dtype):
        raise TypeError("Bs, Cs and Ds must have one dtype")
    batch = Bs.size // (n * n)
    if Ds.size < batch * n or (Cs is not None and Cs.size < batch * n):
        raise ValueError("Cs and Ds smaller than batch*n")
    out = np.empty(batch, dtype=Bs.dtype)
    info = np.zeros(batch, dtype=np.int32)
    _lib.check(_lib.lib().matinv_logml_batched_host(
        _np_dtype_code(Bs.dtype), n, Bs.ctypes.data_as(ctypes.c_void_p), Cs.ctypes.data_as(ctypes.c_void_p) if Cs is not None else None,
        Ds.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), batch, info.ctypes.data_as(ctypes.c_void_p)))
    return out, info


def loo_batched(n, Bs, Cs, Ds, mean=None, var=None, logpl=None, batchSize=None, info=None):
    """Leave-one-out cross-validation of a GP on device tensors (matinv_loo_batched; asynchronous on torch's current stream). With
    M_k = B_k + diag c_k, kappa_i = [M^-1]_ii and alpha = M^-1 d: mean_i = d_i - alpha_i / kappa_i (the prediction at training point i
    from the other n - 1), var_i = 1 / kappa_i, logpl = sum_i (1/2 log kappa_i - 1/2 alpha_i^2 / kappa_i) - n/2 log(2 pi).
    Cs may be None (M = B). Only B's lower triangle is read and no input is modified. mean, var: optional tensors of at least
    batchSize*n elements, logpl: of at least batchSize (allocated when None; elements beyond are left alone).
    Returns (mean, var, logpl)."""
    import torch
    _require_cuda(Bs, Cs, Ds, mean, var, logpl, info)
    if batchSize is None:
        batchSize = Bs.numel() // (n * n)
    if mean is None:
        mean = torch.empty(batchSize * n, dtype=Bs.dtype, device=Bs.device)
    if var is None:
        var = torch.empty(batchSize * n, dtype=Bs.dtype, device=Bs.device)
    if logpl is None:
        logpl = torch.empty(batchSize, dtype=Bs.dtype, device=Bs.device)
    if any(t.dtype != Bs.dtype for t in (Ds, mean, var, logpl)) or (Cs is not None and Cs.dtype != Bs.dtype):
        raise TypeError("Bs, Cs, Ds, mean, var and logpl must have one dtype")
    if any(t.numel() < batchSize * n for t in (Ds, mean, var)) or logpl.numel() < batchSize or (Cs is not None and Cs.numel() < batchSize * n):
        raise ValueError("Cs, Ds, mean and var need batchSize*n elements, logpl batchSize")
    _check_info(info, batchSize)
    with torch.cuda.device(Bs.device):
        _lib.check(_lib.lib().matinv_loo_batched(
            _torch_dtype_code(Bs), n, ctypes.c_void_p(Bs.data_ptr()), ctypes.c_void_p(Cs.data_ptr()) if Cs is not None else None,
            ctypes.c_void_p(Ds.data_ptr()), ctypes.c_void_p(mean.data_ptr()), ctypes.c_void_p(var.data_ptr()),
            ctypes.c_void_p(logpl.data_ptr()), batchSize, ctypes.c_void_p(info.data_ptr()) if info is not None else None, _stream_ptr(Bs)))
    return mean, var, logpl


def loo_batched_host(n, Bs: np.ndarray, Cs, Ds: np.ndarray):
    """matinv_loo_batched_host on numpy batches (packed; Cs may be None): returns (mean, var, logpl, info). Synchronous."""
    Bs = np.ascontiguousarray(Bs)
    Ds = np.ascontiguousarray(Ds)
    Cs = None if Cs is None else np.ascontiguousarray(Cs)
    if Ds.dtype != Bs.dtype or (Cs is not None and Cs.dtype != Bs.dtype):
        raise TypeError("Bs, Cs and Ds must have one dtype")
    batch = Bs.size // (n * n)
    if Ds.size < batch * n or (Cs is not None and Cs.size < batch * n):
        raise ValueError("Cs and Ds smaller than batch*n")
    mean = np.empty(batch * n, dtype=Bs.dtype)
    var = np.empty(batch * n, dtype=Bs.dtype)
    logpl = np.empty(batch, dtype=Bs.dtype)
    info = np.zeros(batch, dtype=np.int32)
    _lib.check(_lib.lib().matinv_loo_batched_host(
        _np_dtype_code(Bs.dtype), n, Bs.ctypes.data_as(ctypes.c_void_p), Cs.ctypes.data_as(ctypes.c_void_p) if Cs is not None else None,
        Ds.ctypes.data_as(ctypes.c_void_p), mean.ctypes.data_as(ctypes.c_void_p), var.ctypes.data_as(ctypes.c_void_p),
        logpl.ctypes.data_as(ctypes.c_void_p), batch, info.ctypes.data_as(ctypes.c_void_p)))
    return mean, var, logpl, info


def loo_kernel_name(dtype, n: int) -> str:
    """matinv_loo_kernel_name: the kernel a leave-one-out request launches ("" when the request would be refused)."""
    code = _dtype_code(dtype)
    return _lib.lib().matinv_loo_kernel_name(code, n).decode()


_GRAD_OUTPUTS = ("grad", "gradc", "alpha")


def logml_grad_batched(n, Bs, Cs, Ds, dMs, grad=None, gradc=None, alpha=None, batchSize=None, info=None, want=("grad",)):
    """Gradients of the GP log marginal likelihood on device tensors (matinv_logml_grad_batched; asynchronous on torch's current stream).
    With M_k = B_k + diag c_k, K = M^-1 and alpha = K d:  grad[k, p] = 1/2 sum_ij (alpha_i alpha_j - K_ij) dM_p[i, j] for the P symmetric
    derivative matrices of matrix k (dMs: batchSize*P*n*n elements, matrix (k, p) at (k*P + p)*n*n, column-major, lower triangle read),
    gradc[k, i] = 1/2 (alpha_i^2 - K_ii) (the derivative w.r.t. c_i), alpha[k, i] = alpha_i.
    An output is computed when its tensor is given or its name is in `want` (then it is allocated); at least one. Cs may be None (M = B),
    dMs may be None when grad is not asked for. P is dMs.numel() // (batchSize*n*n). Only the lower triangles of B and dM are read and no
    input is modified. Returns (grad, gradc, alpha), None for what was not asked for."""
    import torch
    _require_cuda(Bs, Cs, Ds, dMs, grad, gradc, alpha, info)
    if batchSize is None:
        batchSize = Bs.numel() // (n * n)
    unknown = set(want) - set(_GRAD_OUTPUTS)
    if unknown:
        raise ValueError(f"want holds {sorted(unknown)}; the outputs are {_GRAD_OUTPUTS}")
    if grad is None and gradc is None and alpha is None and not want:
        raise ValueError("no output requested")
    nparam = 0
    if grad is not None or "grad" in want:
        if dMs is None:
            raise ValueError("grad needs the derivative matrices dMs")
        nparam = dMs.numel() // (batchSize * n * n) if batchSize else 0
        if batchSize and (nparam < 1 or dMs.numel() < batchSize * nparam * n * n):
            raise ValueError("dMs needs batchSize*P*n*n elements, P >= 1")
        if grad is None:
            grad = torch.empty(batchSize * nparam, dtype=Bs.dtype, device=Bs.device)
    if gradc is None and "gradc" in want:
        gradc = torch.empty(batchSize * n, dtype=Bs.dtype, device=Bs.device)
    if alpha is None and "alpha" in want:
        alpha = torch.empty(batchSize * n, dtype=Bs.dtype, device=Bs.device)
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Ds, dMs, grad, gradc, alpha)):
        raise TypeError("Bs, Cs, Ds, dMs, grad, gradc and alpha must have one dtype")
    if any(t is not None and t.numel() < batchSize * n for t in (Cs, Ds, gradc, alpha)) or (grad is not None and grad.numel() < batchSize * nparam):
        raise ValueError("Cs, Ds, gradc and alpha need batchSize*n elements, grad batchSize*P")
    _check_info(info, batchSize)
    p = _tensor_ptr
    with torch.cuda.device(Bs.device):
        _lib.check(_lib.lib().matinv_logml_grad_batched(
            _torch_dtype_code(Bs), n, nparam, p(Bs), p(Cs), p(Ds), p(dMs) if grad is not None else None, p(grad), p(gradc), p(alpha),
            batchSize, p(info), _stream_ptr(Bs)))
    return grad, gradc, alpha


def logml_grad_batched_host(n, Bs: np.ndarray, Cs, Ds: np.ndarray, dMs, want=_GRAD_OUTPUTS):
    """matinv_logml_grad_batched_host on numpy batches (packed; Cs may be None, dMs may be None without "grad" in want): returns
    (grad, gradc, alpha, info), None for the outputs not in want. Synchronous."""
    Bs = np.ascontiguousarray(Bs)
    Ds = np.ascontiguousarray(Ds)
    Cs = None if Cs is None else np.ascontiguousarray(Cs)
    dMs = None if dMs is None else np.ascontiguousarray(dMs)
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Ds, dMs)):
        raise TypeError("Bs, Cs, Ds and dMs must have one dtype")
    unknown = set(want) - set(_GRAD_OUTPUTS)
    if unknown or not want:
        raise ValueError(f"want must name at least one of {_GRAD_OUTPUTS}")
    batch = Bs.size // (n * n)
    if Ds.size < batch * n or (Cs is not None and Cs.size < batch * n):
        raise ValueError("Cs and Ds smaller than batch*n")
    nparam = 0
    grad = gradc = alpha = None
    if "grad" in want:
        if dMs is None:
            raise ValueError("grad needs the derivative matrices dMs")
        nparam = dMs.size // (batch * n * n) if batch else 0
        if batch and nparam < 1:
            raise ValueError("dMs needs batch*P*n*n elements, P >= 1")
        grad = np.empty(batch * nparam, dtype=Bs.dtype)
    if "gradc" in want:
        gradc = np.empty(batch * n, dtype=Bs.dtype)
    if "alpha" in want:
        alpha = np.empty(batch * n, dtype=Bs.dtype)
    info = np.zeros(batch, dtype=np.int32)
    p = _array_ptr
    _lib.check(_lib.lib().matinv_logml_grad_batched_host(
        _np_dtype_code(Bs.dtype), n, nparam, p(Bs), p(Cs), p(Ds), p(dMs) if grad is not None else None, p(grad), p(gradc), p(alpha), batch,
        p(info)))
    return grad, gradc, alpha, info


def logml_grad_kernel_name(dtype, n: int) -> str:
    """matinv_logml_grad_kernel_name: the kernel a gradient request launches ("" when the request would be refused)."""
    code = _dtype_code(dtype)
    return _lib.lib().matinv_logml_grad_kernel_name(code, n).decode()


_LOO_GRAD_OUTPUTS = ("grad", "gradc", "logpl")


def loo_grad_batched(n, Bs, Cs, Ds, dMs, grad=None, gradc=None, logpl=None, batchSize=None, info=None, want=("grad",)):
    """Gradients of the GP leave-one-out log pseudo-likelihood on device tensors (matinv_loo_grad_batched; asynchronous on torch's current
    stream). With M_k = B_k + diag c_k, K = M^-1, alpha = K d, kappa_i = K_ii, b_i = alpha_i / kappa_i, beta = K b,
    s_i = (1 + alpha_i^2 / kappa_i) / kappa_i and G = 1/2 (alpha beta^T + beta alpha^T) - 1/2 K diag(s) K:
    grad[k, p] = sum_ij G_ij dM_p[i, j] for the P symmetric derivative matrices of matrix k (dMs: batchSize*P*n*n elements, matrix (k, p)
    at (k*P + p)*n*n, column-major, lower triangle read), gradc[k, i] = G_ii (the derivative w.r.t. c_i), logpl[k] = the pseudo-likelihood
    itself, as loo_batched returns it.
    An output is computed when its tensor is given or its name is in `want` (then it is allocated); at least one. Cs may be None (M = B),
    dMs may be None when grad is not asked for. P is dMs.numel() // (batchSize*n*n). Only the lower triangles of B and dM are read and no
    input is modified. Returns (grad, gradc, logpl), None for what was not asked for."""
    import torch
    _require_cuda(Bs, Cs, Ds, dMs, grad, gradc, logpl, info)
    if batchSize is None:
        batchSize = Bs.numel() // (n * n)
    unknown = set(want) - set(_LOO_GRAD_OUTPUTS)
    if unknown:
        raise ValueError(f"want holds {sorted(unknown)}; the outputs are {_LOO_GRAD_OUTPUTS}")
    if grad is None and gradc is None and logpl is None and not want:
        raise ValueError("no output requested")
    nparam = 0
    if grad is not None or "grad" in want:
        if dMs is None:
            raise ValueError("grad needs the derivative matrices dMs")
        nparam = dMs.numel() // (batchSize * n * n) if batchSize else 0
        if batchSize and (nparam < 1 or dMs.numel() < batchSize * nparam * n * n):
            raise ValueError("dMs needs batchSize*P*n*n elements, P >= 1")
        if grad is None:
            grad = torch.empty(batchSize * nparam, dtype=Bs.dtype, device=Bs.device)
    if gradc is None and "gradc" in want:
        gradc = torch.empty(batchSize * n, dtype=Bs.dtype, device=Bs.device)
    if logpl is None and "logpl" in want:
        logpl = torch.empty(batchSize, dtype=Bs.dtype, device=Bs.device)
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Ds, dMs, grad, gradc, logpl)):
        raise TypeError("Bs, Cs, Ds, dMs, grad, gradc and logpl must have one dtype")
    if any(t is not None and t.numel() < batchSize * n for t in (Cs, Ds, gradc)) or (grad is not None and grad.numel() < batchSize * nparam) \
            or (logpl is not None and logpl.numel() < batchSize):
        raise ValueError("Cs, Ds and gradc need batchSize*n elements, grad batchSize*P, logpl batchSize")
    _check_info(info, batchSize)
    p = _tensor_ptr
    with torch.cuda.device(Bs.device):
        _lib.check(_lib.lib().matinv_loo_grad_batched(
            _torch_dtype_code(Bs), n, nparam, p(Bs), p(Cs), p(Ds), p(dMs) if grad is not None else None, p(grad), p(gradc), p(logpl),
            batchSize, p(info), _stream_ptr(Bs)))
    return grad, gradc, logpl


def loo_grad_batched_host(n, Bs: np.ndarray, Cs, Ds: np.ndarray, dMs, want=_LOO_GRAD_OUTPUTS):
    """matinv_loo_grad_batched_host on numpy batches (packed; Cs may be None, dMs may be None without "grad" in want): returns
    (grad, gradc, logpl, info), None for the outputs not in want. Synchronous."""
    Bs = np.ascontiguousarray(Bs)
    Ds = np.ascontiguousarray(Ds)
    Cs = None if Cs is None else np.ascontiguousarray(Cs)
    dMs = None if dMs is None else np.ascontiguousarray(dMs)
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Ds, dMs)):
        raise TypeError("Bs, Cs, Ds and dMs must have one dtype")
    unknown = set(want) - set(_LOO_GRAD_OUTPUTS)
    if unknown or not want:
        raise ValueError(f"want must name at least one of {_LOO_GRAD_OUTPUTS}")
    batch = Bs.size // (n * n)
    if Ds.size < batch * n or (Cs is not None and Cs.size < batch * n):
        raise ValueError("Cs and Ds smaller than batch*n")
    nparam = 0
    grad = gradc = logpl = None
    if "grad" in want:
        if dMs is None:
            raise ValueError("grad needs the derivative matrices dMs")
        nparam = dMs.size // (batch * n * n) if batch else 0
        if batch and nparam < 1:
            raise ValueError("dMs needs batch*P*n*n elements, P >= 1")
        grad = np.empty(batch * nparam, dtype=Bs.dtype)
    if "gradc" in want:
        gradc = np.empty(batch * n, dtype=Bs.dtype)
    if "logpl" in want:
        logpl = np.empty(batch, dtype=Bs.dtype)
    info = np.zeros(batch, dtype=np.int32)
    p = _array_ptr
    _lib.check(_lib.lib().matinv_loo_grad_batched_host(
        _np_dtype_code(Bs.dtype), n, nparam, p(Bs), p(Cs), p(Ds), p(dMs) if grad is not None else None, p(grad), p(gradc), p(logpl), batch,
        p(info)))
    return grad, gradc, logpl, info


def loo_grad_kernel_name(dtype, n: int) -> str:
    """matinv_loo_grad_kernel_name: the kernel a LOO-gradient request launches ("" when the request would be refused)."""
    code = _dtype_code(dtype)
    return _lib.lib().matinv_loo_grad_kernel_name(code, n).decode()


_PREDICT_OUTPUTS = ("mean", "var")


def predict_batched(n, Bs, Cs, Ds, As, Es, mean=None, var=None, batchSize=None, info=None, want=_PREDICT_OUTPUTS):
    """GP prediction at Q query points per covariance matrix on device tensors (matinv_predict_batched; asynchronous on torch's current
    stream). With M_k = B_k + diag c_k, K = M^-1 and alpha = K d:  mean[k, j] = a_kj^T alpha_k,  var[k, j] = e_kj - a_kj^T K_k a_kj  for the
    Q cross-covariance vectors of matrix k (As: batchSize*Q*n elements, vector (k, j) at (k*Q + j)*n) and their prior variances (Es:
    batchSize*Q elements, or None for e = 0). Q is As.numel() // (batchSize*n).
    An output is computed when its tensor is given or its name is in `want` (then it is allocated); at least one. Cs may be None (M = B),
    Ds may be None when mean is not asked for. Only B's lower triangle is read, no input is modified and var is not clamped.
    Returns (mean, var), None for what was not asked for."""
    import torch
    _require_cuda(Bs, Cs, Ds, As, Es, mean, var, info)
    if batchSize is None:
        batchSize = Bs.numel() // (n * n)
    unknown = set(want) - set(_PREDICT_OUTPUTS)
    if unknown:
        raise ValueError(f"want holds {sorted(unknown)}; the outputs are {_PREDICT_OUTPUTS}")
    if mean is None and var is None and not want:
        raise ValueError("no output requested")
    if As is None:
        raise ValueError("prediction needs the cross-covariance vectors As")
    nquery = As.numel() // (batchSize * n) if batchSize else 0
    if batchSize and (nquery < 1 or As.numel() < batchSize * nquery * n):
        raise ValueError("As needs batchSize*Q*n elements, Q >= 1")
    if mean is None and "mean" in want:
        mean = torch.empty(batchSize * nquery, dtype=Bs.dtype, device=Bs.device)
    if var is None and "var" in want:
        var = torch.empty(batchSize * nquery, dtype=Bs.dtype, device=Bs.device)
    if mean is not None and Ds is None:
        raise ValueError("mean needs the observations Ds")
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Ds, As, Es, mean, var)):
        raise TypeError("Bs, Cs, Ds, As, Es, mean and var must have one dtype")
    if any(t is not None and t.numel() < batchSize * n for t in (Cs, Ds)) or \
            any(t is not None and t.numel() < batchSize * nquery for t in (Es, mean, var)):
        raise ValueError("Cs and Ds need batchSize*n elements, Es, mean and var batchSize*Q")
    _check_info(info, batchSize)
    p = _tensor_ptr
    with torch.cuda.device(Bs.device):
        _lib.check(_lib.lib().matinv_predict_batched(
            _torch_dtype_code(Bs), n, nquery, p(Bs), p(Cs), p(Ds) if mean is not None else None, p(As), p(Es), p(mean), p(var), batchSize,
            p(info), _stream_ptr(Bs)))
    return mean, var


def predict_batched_host(n, Bs: np.ndarray, Cs, Ds, As: np.ndarray, Es, want=_PREDICT_OUTPUTS):
    """matinv_predict_batched_host on numpy batches (packed; Cs and Es may be None, Ds may be None without "mean" in want): returns
    (mean, var, info), None for the outputs not in want. Synchronous."""
    Bs = np.ascontiguousarray(Bs)
    As = np.ascontiguousarray(As)
    Cs, Ds, Es = (None if t is None else np.ascontiguousarray(t) for t in (Cs, Ds, Es))
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Ds, As, Es)):
        raise TypeError("Bs, Cs, Ds, As and Es must have one dtype")
    unknown = set(want) - set(_PREDICT_OUTPUTS)
    if unknown or not want:
        raise ValueError(f"want must name at least one of {_PREDICT_OUTPUTS}")
    batch = Bs.size // (n * n)
    nquery = As.size // (batch * n) if batch else 0
    if batch and nquery < 1:
        raise ValueError("As needs batch*Q*n elements, Q >= 1")
    if "mean" in want and Ds is None:
        raise ValueError("mean needs the observations Ds")
    if any(t is not None and t.size < batch * n for t in (Cs, Ds)) or (Es is not None and Es.size < batch * nquery):
        raise ValueError("Cs and Ds smaller than batch*n, or Es smaller than batch*Q")
    mean = np.empty(batch * nquery, dtype=Bs.dtype) if "mean" in want else None
    var = np.empty(batch * nquery, dtype=Bs.dtype) if "var" in want else None
    info = np.zeros(batch, dtype=np.int32)
    p = _array_ptr
    _lib.check(_lib.lib().matinv_predict_batched_host(
        _np_dtype_code(Bs.dtype), n, nquery, p(Bs), p(Cs), p(Ds) if mean is not None else None, p(As), p(Es), p(mean), p(var), batch,
        p(info)))
    return mean, var, info


def predict_kernel_name(dtype, n: int) -> str:
    """matinv_predict_kernel_name: the kernel a prediction request launches ("" when the request would be refused)."""
    code = _dtype_code(dtype)
    return _lib.lib().matinv_predict_kernel_name(code, n).decode()


_PREDICT_COV_OUTPUTS = ("mean", "cov")


def predict_cov_batched(n, Bs, Cs, Ds, As, Es, mean=None, cov=None, batchSize=None, info=None, want=_PREDICT_COV_OUTPUTS):
    """Joint predictive covariance between the Q query points of each covariance matrix on device tensors (matinv_predict_cov_batched;
    asynchronous on torch's current stream). With M_k = B_k + diag c_k, K = M^-1 and alpha = K d:  mean[k, i] = a_ki^T alpha_k,
    cov[k][j*Q + i] = E_k[i][j] - a_ki^T K_k a_kj  for the Q cross-covariance vectors of matrix k (As as in predict_batched) and the Q x Q
    prior covariance between them (Es: batchSize*Q*Q elements, column-major per matrix, only the lower triangle read, or None for E = 0).
    Q is As.numel() // (batchSize*n). cov (batchSize*Q*Q elements) has both triangles written and is exactly symmetric.
    An output is computed when its tensor is given or its name is in `want` (then it is allocated); at least one. Cs may be None (M = B),
    Ds may be None when mean is not asked for. Only B's lower triangle is read, no input is modified and cov is not clamped.
    Returns (mean, cov), None for what was not asked for."""
    import torch
    _require_cuda(Bs, Cs, Ds, As, Es, mean, cov, info)
    if batchSize is None:
        batchSize = Bs.numel() // (n * n)
    unknown = set(want) - set(_PREDICT_COV_OUTPUTS)
    if unknown:
        raise ValueError(f"want holds {sorted(unknown)}; the outputs are {_PREDICT_COV_OUTPUTS}")
    if mean is None and cov is None and not want:
        raise ValueError("no output requested")
    if As is None:
        raise ValueError("prediction needs the cross-covariance vectors As")
    nquery = As.numel() // (batchSize * n) if batchSize else 0
    if batchSize and (nquery < 1 or As.numel() < batchSize * nquery * n):
        raise ValueError("As needs batchSize*Q*n elements, Q >= 1")
    if mean is None and "mean" in want:
        mean = torch.empty(batchSize * nquery, dtype=Bs.dtype, device=Bs.device)
    if cov is None and "cov" in want:
        cov = torch.empty(batchSize * nquery * nquery, dtype=Bs.dtype, device=Bs.device)
    if mean is not None and Ds is None:
        raise ValueError("mean needs the observations Ds")
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Ds, As, Es, mean, cov)):
        raise TypeError("Bs, Cs, Ds, As, Es, mean and cov must have one dtype")
    if any(t is not None and t.numel() < batchSize * n for t in (Cs, Ds)) or (mean is not None and mean.numel() < batchSize * nquery) or \
            any(t is not None and t.numel() < batchSize * nquery * nquery for t in (Es, cov)):
        raise ValueError("Cs and Ds need batchSize*n elements, mean batchSize*Q, Es and cov batchSize*Q*Q")
    _check_info(info, batchSize)
    p = _tensor_ptr
    with torch.cuda.device(Bs.device):
        _lib.check(_lib.lib().matinv_predict_cov_batched(
            _torch_dtype_code(Bs), n, nquery, p(Bs), p(Cs), p(Ds) if mean is not None else None, p(As), p(Es) if cov is not None else None,
            p(mean), p(cov), batchSize, p(info), _stream_ptr(Bs)))
    return mean, cov


def predict_cov_batched_host(n, Bs: np.ndarray, Cs, Ds, As: np.ndarray, Es, want=_PREDICT_COV_OUTPUTS):
    """matinv_predict_cov_batched_host on numpy batches (packed; Cs and Es may be None, Ds may be None without "mean" in want): returns
    (mean, cov, info), None for the outputs not in want. Synchronous."""
    Bs = np.ascontiguousarray(Bs)
    As = np.ascontiguousarray(As)
    Cs, Ds, Es = (None if t is None else np.ascontiguousarray(t) for t in (Cs, Ds, Es))
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Ds, As, Es)):
        raise TypeError("Bs, Cs, Ds, As and Es must have one dtype")
    unknown = set(want) - set(_PREDICT_COV_OUTPUTS)
    if unknown or not want:
        raise ValueError(f"want must name at least one of {_PREDICT_COV_OUTPUTS}")
    batch = Bs.size // (n * n)
    nquery = As.size // (batch * n) if batch else 0
    if batch and nquery < 1:
        raise ValueError("As needs batch*Q*n elements, Q >= 1")
    if "mean" in want and Ds is None:
        raise ValueError("mean needs the observations Ds")
    if any(t is not None and t.size < batch * n for t in (Cs, Ds)) or (Es is not None and Es.size < batch * nquery * nquery):
        raise ValueError("Cs and Ds smaller than batch*n, or Es smaller than batch*Q*Q")
    mean = np.empty(batch * nquery, dtype=Bs.dtype) if "mean" in want else None
    cov = np.empty(batch * nquery * nquery, dtype=Bs.dtype) if "cov" in want else None
    info = np.zeros(batch, dtype=np.int32)
    p = _array_ptr
    _lib.check(_lib.lib().matinv_predict_cov_batched_host(
        _np_dtype_code(Bs.dtype), n, nquery, p(Bs), p(Cs), p(Ds) if mean is not None else None, p(As), p(Es) if cov is not None else None,
        p(mean), p(cov), batch, p(info)))
    return mean, cov, info


def predict_cov_kernel_name(dtype, n: int) -> str:
    """matinv_predict_cov_kernel_name: the kernel a predictive-covariance request launches ("" when the request would be refused)."""
    code = _dtype_code(dtype)
    return _lib.lib().matinv_predict_cov_kernel_name(code, n).decode()


_COLOUR_OUTPUTS = ("Y", "L")


def colour_batched(q, Cs, Ms, Zs, Y=None, L=None, batchSize=None, info=None, want=_COLOUR_OUTPUTS, strideC=None):
    """Lower Cholesky factors of batched SPD matrices and samples coloured by them on device tensors (matinv_colour_batched; asynchronous
    on torch's current stream):  C_k = L_k L_k^T,  Y_k[:, s] = m_k + L_k z_ks.  Cs: matrix k is q x q, column-major, at element
    k*strideC (default q*q), only the lower triangle read. Ms: batchSize*q elements or None (m = 0). Zs: batchSize*S*q elements, sample s
    of matrix k a run of q elements; S is Zs.numel() // (batchSize*q). Y has the layout of Zs; L is batchSize*q*q, column-major, with the
    strict upper triangle written as zeros.
    An output is computed when its tensor is given or its name is in `want` (then it is allocated); at least one. Zs may be None when Y is
    not asked for. No input is modified and the library draws no random numbers: Zs is the caller's. Not positive definite: info = the
    1-based column of the first non-positive pivot and every requested output of that matrix NaN; there is no jitter.
    Returns (Y, L), None for what was not asked for."""
    import torch
    _require_cuda(Cs, Ms, Zs, Y, L, info)
    if strideC is None:
        strideC = q * q
    if batchSize is None:
        batchSize = Cs.numel() // strideC
    unknown = set(want) - set(_COLOUR_OUTPUTS)
    if unknown:
        raise ValueError(f"want holds {sorted(unknown)}; the outputs are {_COLOUR_OUTPUTS}")
    if Y is None and L is None and not want:
        raise ValueError("no output requested")
    wants_y = Y is not None or "Y" in want
    if wants_y and Zs is None:
        raise ValueError("Y needs the samples Zs")
    nsample = Zs.numel() // (batchSize * q) if (wants_y and batchSize) else 0
    if wants_y and batchSize and (nsample < 1 or Zs.numel() < batchSize * nsample * q):
        raise ValueError("Zs needs batchSize*S*q elements, S >= 1")
    if Y is None and wants_y:
        Y = torch.empty(batchSize * nsample * q, dtype=Cs.dtype, device=Cs.device)
    if L is None and "L" in want:
        L = torch.empty(batchSize * q * q, dtype=Cs.dtype, device=Cs.device)
    if any(t is not None and t.dtype != Cs.dtype for t in (Ms, Zs, Y, L)):
        raise TypeError("Cs, Ms, Zs, Y and L must have one dtype")
    if batchSize and Cs.numel() < (batchSize - 1) * strideC + q * q:
        raise ValueError("Cs needs (batchSize-1)*strideC + q*q elements")
    if (Ms is not None and Ms.numel() < batchSize * q) or (Y is not None and Y.numel() < batchSize * nsample * q) or \
            (L is not None and L.numel() < batchSize * q * q):
        raise ValueError("Ms needs batchSize*q elements, Y batchSize*S*q, L batchSize*q*q")
    _check_info(info, batchSize)
    p = _tensor_ptr
    with torch.cuda.device(Cs.device):
        _lib.check(_lib.lib().matinv_colour_batched(
            _torch_dtype_code(Cs), q, nsample, p(Cs), strideC, p(Ms) if Y is not None else None, p(Zs) if Y is not None else None, p(Y), p(L),
            batchSize, p(info), _stream_ptr(Cs)))
    return Y, L


def colour_batched_host(q, Cs: np.ndarray, Ms, Zs, want=_COLOUR_OUTPUTS):
    """matinv_colour_batched_host on numpy batches (packed; Ms may be None, Zs may be None without "Y" in want): returns (Y, L, info), None
    for the outputs not in want. Synchronous."""
    Cs = np.ascontiguousarray(Cs)
    Ms, Zs = (None if t is None else np.ascontiguousarray(t) for t in (Ms, Zs))
    if any(t is not None and t.dtype != Cs.dtype for t in (Ms, Zs)):
        raise TypeError("Cs, Ms and Zs must have one dtype")
    unknown = set(want) - set(_COLOUR_OUTPUTS)
    if unknown or not want:
        raise ValueError(f"want must name at least one of {_COLOUR_OUTPUTS}")
    batch = Cs.size // (q * q)
    if "Y" in want and Zs is None:
        raise ValueError("Y needs the samples Zs")
    nsample = Zs.size // (batch * q) if ("Y" in want and batch) else 0
    if "Y" in want and batch and nsample < 1:
        raise ValueError("Zs needs batch*S*q elements, S >= 1")
    if Ms is not None and Ms.size < batch * q:
        raise ValueError("Ms smaller than batch*q")
    Y = np.empty(batch * nsample * q, dtype=Cs.dtype) if "Y" in want else None
    L = np.empty(batch * q * q, dtype=Cs.dtype) if "L" in want else None
    info = np.zeros(batch, dtype=np.int32)
    p = _array_ptr
    _lib.check(_lib.lib().matinv_colour_batched_host(
        _np_dtype_code(Cs.dtype), q, nsample, p(Cs), q * q, p(Ms) if Y is not None else None, p(Zs) if Y is not None else None, p(Y), p(L),
        batch, p(info)))
    return Y, L, info


def colour_kernel_name(dtype, q: int) -> str:
    """matinv_colour_kernel_name: the kernel a colour request launches ("" when the request would be refused)."""
    code = _dtype_code(dtype)
    return _lib.lib().matinv_colour_kernel_name(code, q).decode()


_WHITEN_OUTPUTS = ("W", "maha", "logdet", "logpdf")


def whiten_batched(q, Cs, Ms, Xs, W=None, maha=None, logdet=None, logpdf=None, batchSize=None, info=None, want=_WHITEN_OUTPUTS,
                   strideC=None):
    """Whitened points, squared Mahalanobis distances, log-determinants and Gaussian log-densities of batched SPD matrices on device tensors
    (matinv_whiten_batched; asynchronous on torch's current stream) -- the inverse map of colour_batched. With C_k = L_k L_k^T:
        W_k[:, s] = L_k^-1 (x_ks - m_k),  maha_k[s] = ||W_k[:, s]||^2,  logdet_k = log det C_k,
        logpdf_k[s] = -(maha_k[s] + logdet_k + q log 2 pi) / 2
    Cs: matrix k is q x q, column-major, at element k*strideC (default q*q), only the lower triangle read. Ms: batchSize*q elements or None
    (m = 0). Xs: batchSize*S*q elements, point s of matrix k a run of q elements; S is Xs.numel() // (batchSize*q). W has the layout of
    Xs; maha and logpdf are batchSize*S, logdet is batchSize.
    An output is computed when its tensor is given or its name is in `want` (then it is allocated); at least one; which are asked for
    changes no bit of the others. Xs may be None when only logdet is asked for. No input is modified. Not positive definite: info = the
    1-based column of the first non-positive pivot and every requested output of that matrix NaN; there is no jitter.
    Returns (W, maha, logdet, logpdf), None for what was not asked for."""
    import torch
    _require_cuda(Cs, Ms, Xs, W, maha, logdet, logpdf, info)
    if strideC is None:
        strideC = q * q
    if batchSize is None:
        batchSize = Cs.numel() // strideC
    unknown = set(want) - set(_WHITEN_OUTPUTS)
    if unknown:
        raise ValueError(f"want holds {sorted(unknown)}; the outputs are {_WHITEN_OUTPUTS}")
    given = dict(W=W, maha=maha, logdet=logdet, logpdf=logpdf)
    asked = {k: given[k] is not None or k in want for k in _WHITEN_OUTPUTS}
    if not any(asked.values()):
        raise ValueError("no output requested")
    points = asked["W"] or asked["maha"] or asked["logpdf"]
    if points and Xs is None:
        raise ValueError("W, maha and logpdf need the points Xs")
    npoint = Xs.numel() // (batchSize * q) if (points and batchSize) else 0
    if points and batchSize and (npoint < 1 or Xs.numel() < batchSize * npoint * q):
        raise ValueError("Xs needs batchSize*S*q elements, S >= 1")
    sizes = dict(W=batchSize * npoint * q, maha=batchSize * npoint, logdet=batchSize, logpdf=batchSize * npoint)
    for k in _WHITEN_OUTPUTS:
        if asked[k] and given[k] is None:
            given[k] = torch.empty(sizes[k], dtype=Cs.dtype, device=Cs.device)
    if any(t is not None and t.dtype != Cs.dtype for t in (Ms, Xs, *given.values())):
        raise TypeError("Cs, Ms, Xs, W, maha, logdet and logpdf must have one dtype")
    if batchSize and Cs.numel() < (batchSize - 1) * strideC + q * q:
        raise ValueError("Cs needs (batchSize-1)*strideC + q*q elements")
    if (Ms is not None and Ms.numel() < batchSize * q) or any(given[k] is not None and given[k].numel() < sizes[k] for k in _WHITEN_OUTPUTS):
        raise ValueError("Ms needs batchSize*q elements, W batchSize*S*q, maha and logpdf batchSize*S, logdet batchSize")
    _check_info(info, batchSize)
    p = _tensor_ptr
    with torch.cuda.device(Cs.device):
        _lib.check(_lib.lib().matinv_whiten_batched(
            _torch_dtype_code(Cs), q, npoint, p(Cs), strideC, p(Ms) if points else None, p(Xs) if points else None, p(given["W"]),
            p(given["maha"]), p(given["logdet"]), p(given["logpdf"]), batchSize, p(info), _stream_ptr(Cs)))
    return given["W"], given["maha"], given["logdet"], given["logpdf"]


def whiten_batched_host(q, Cs: np.ndarray, Ms, Xs, want=_WHITEN_OUTPUTS):
    """matinv_whiten_batched_host on numpy batches (packed; Ms may be None, Xs may be None when only "logdet" is in want): returns
    (W, maha, logdet, logpdf, info), None for the outputs not in want. Synchronous."""
    Cs = np.ascontiguousarray(Cs)
    Ms, Xs = (None if t is None else np.ascontiguousarray(t) for t in (Ms, Xs))
    if any(t is not None and t.dtype != Cs.dtype for t in (Ms, Xs)):
        raise TypeError("Cs, Ms and Xs must have one dtype")
    unknown = set(want) - set(_WHITEN_OUTPUTS)
    if unknown or not want:
        raise ValueError(f"want must name at least one of {_WHITEN_OUTPUTS}")
    batch = Cs.size // (q * q)
    points = bool(set(want) & {"W", "maha", "logpdf"})
    if points and Xs is None:
        raise ValueError("W, maha and logpdf need the points Xs")
    npoint = Xs.size // (batch * q) if (points and batch) else 0
    if points and batch and npoint < 1:
        raise ValueError("Xs needs batch*S*q elements, S >= 1")
    if Ms is not None and Ms.size < batch * q:
        raise ValueError("Ms smaller than batch*q")
    sizes = dict(W=batch * npoint * q, maha=batch * npoint, logdet=batch, logpdf=batch * npoint)
    out = {k: np.empty(sizes[k], dtype=Cs.dtype) if k in want else None for k in _WHITEN_OUTPUTS}
    info = np.zeros(batch, dtype=np.int32)
    p = _array_ptr
    _lib.check(_lib.lib().matinv_whiten_batched_host(
        _np_dtype_code(Cs.dtype), q, npoint, p(Cs), q * q, p(Ms) if points else None, p(Xs) if points else None, p(out["W"]), p(out["maha"]),
        p(out["logdet"]), p(out["logpdf"]), batch, p(info)))
    return out["W"], out["maha"], out["logdet"], out["logpdf"], info


def whiten_kernel_name(dtype, q: int) -> str:
    """matinv_whiten_kernel_name: the kernel a whiten request launches ("" when the request would be refused)."""
    code = _dtype_code(dtype)
    return _lib.lib().matinv_whiten_kernel_name(code, q).decode()


_MULTI_TARGET_OUTPUTS = ("alpha", "quad", "logdet", "logml", "mean")


def multi_target_batched(n, Bs, Cs, Ys, As=None, alpha=None, quad=None, logdet=None, logml=None, mean=None, batchSize=None, info=None,
                         want=_MULTI_TARGET_OUTPUTS, ntarget=None, nquery=None):
    """Multi-output GP solves on device tensors (matinv_multi_target_batched; asynchronous on torch's current stream): D target vectors and
    Q query points per covariance matrix, one factorisation. With M_k = B_k + diag c_k:
        alpha[k, t] = M_k^-1 y_kt,  quad[k, t] = y_kt^T alpha[k, t],  logdet[k] = log det M_k,
        logml[k, t] = -(quad[k, t] + logdet[k] + n log 2 pi) / 2,  mean[k, t, j] = a_kj^T alpha[k, t]
    Ys: batchSize*D*n elements, target (k, t) at (k*D + t)*n; alpha has its layout. As: batchSize*Q*n elements as in predict_batched. quad
    and logml are batchSize*D, logdet batchSize, mean batchSize*D*Q with element (k, t, j) at (k*D + t)*Q + j. D and Q are inferred from
    Ys.numel() and As.numel() unless `ntarget` / `nquery` are given.
    An output is computed when its tensor is given or its name is in `want` (then it is allocated); at least one; which are asked for
    changes no bit of the others. "mean" in the default `want` is dropped when As is None. Cs may be None (M = B); Ys may be None when only
    logdet is asked for. Only B's lower triangle is read and no input is modified. Not positive definite: info = the 1-based column of
    the first non-positive pivot and every requested output of that matrix NaN.
    Returns (alpha, quad, logdet, logml, mean), None for what was not asked for."""
    import torch
    _require_cuda(Bs, Cs, Ys, As, alpha, quad, logdet, logml, mean, info)
    if batchSize is None:
        batchSize = Bs.numel() // (n * n)
    unknown = set(want) - set(_MULTI_TARGET_OUTPUTS)
    if unknown:
        raise ValueError(f"want holds {sorted(unknown)}; the outputs are {_MULTI_TARGET_OUTPUTS}")
    if want is _MULTI_TARGET_OUTPUTS and As is None:
        want = _MULTI_TARGET_OUTPUTS[:-1]
    given = dict(alpha=alpha, quad=quad, logdet=logdet, logml=logml, mean=mean)
    asked = {k: given[k] is not None or k in want for k in _MULTI_TARGET_OUTPUTS}
    if not any(asked.values()):
        raise ValueError("no output requested")
    targets = asked["alpha"] or asked["quad"] or asked["logml"] or asked["mean"]
    if targets and Ys is None:
        raise ValueError("alpha, quad, logml and mean need the targets Ys")
    if asked["mean"] and As is None:
        raise ValueError("mean needs the cross-covariance vectors As")
    if not targets:
        ntarget = 0
    elif ntarget is None:
        ntarget = Ys.numel() // (batchSize * n) if batchSize else 0
    if not asked["mean"]:
        nquery = 0
    elif nquery is None:
        nquery = As.numel() // (batchSize * n) if batchSize else 0
    if targets and batchSize and (ntarget < 1 or Ys.numel() < batchSize * ntarget * n):
        raise ValueError("Ys needs batchSize*D*n elements, D >= 1")
    if asked["mean"] and batchSize and (nquery < 1 or As.numel() < batchSize * nquery * n):
        raise ValueError("As needs batchSize*Q*n elements, Q >= 1")
    sizes = dict(alpha=batchSize * ntarget * n, quad=batchSize * ntarget, logdet=batchSize, logml=batchSize * ntarget,
                 mean=batchSize * ntarget * nquery)
    for k in _MULTI_TARGET_OUTPUTS:
        if asked[k] and given[k] is None:
            given[k] = torch.empty(sizes[k], dtype=Bs.dtype, device=Bs.device)
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Ys, As, *given.values())):
        raise TypeError("Bs, Cs, Ys, As and the outputs must have one dtype")
    if (Cs is not None and Cs.numel() < batchSize * n) or \
            any(given[k] is not None and given[k].numel() < sizes[k] for k in _MULTI_TARGET_OUTPUTS):
        raise ValueError("Cs needs batchSize*n elements, alpha batchSize*D*n, quad and logml batchSize*D, logdet batchSize, "
                         "mean batchSize*D*Q")
    _check_info(info, batchSize)
    p = _tensor_ptr
    with torch.cuda.device(Bs.device):
        _lib.check(_lib.lib().matinv_multi_target_batched(
            _torch_dtype_code(Bs), n, ntarget, nquery, p(Bs), p(Cs), p(Ys) if targets else None, p(As) if asked["mean"] else None,
            p(given["alpha"]), p(given["quad"]), p(given["logdet"]), p(given["logml"]), p(given["mean"]), batchSize, p(info),
            _stream_ptr(Bs)))
    return given["alpha"], given["quad"], given["logdet"], given["logml"], given["mean"]


def multi_target_batched_host(n, Bs: np.ndarray, Cs, Ys, As=None, want=_MULTI_TARGET_OUTPUTS, ntarget=None, nquery=None):
    """matinv_multi_target_batched_host on numpy batches (packed; Cs may be None, Ys may be None when only "logdet" is in want, As may be
    None without "mean" in want, which the default `want` then drops): returns (alpha, quad, logdet, logml, mean, info), None for the
    outputs not in want. Synchronous."""
    Bs = np.ascontiguousarray(Bs)
    Cs, Ys, As = (None if t is None else np.ascontiguousarray(t) for t in (Cs, Ys, As))
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Ys, As)):
        raise TypeError("Bs, Cs, Ys and As must have one dtype")
    if want is _MULTI_TARGET_OUTPUTS and As is None:
        want = _MULTI_TARGET_OUTPUTS[:-1]
    unknown = set(want) - set(_MULTI_TARGET_OUTPUTS)
    if unknown or not want:
        raise ValueError(f"want must name at least one of {_MULTI_TARGET_OUTPUTS}")
    batch = Bs.size // (n * n)
    targets = bool(set(want) - {"logdet"})
    if targets and Ys is None:
        raise ValueError("alpha, quad, logml and mean need the targets Ys")
    if "mean" in want and As is None:
        raise ValueError("mean needs the cross-covariance vectors As")
    if not targets:
        ntarget = 0
    elif ntarget is None:
        ntarget = Ys.size // (batch * n) if batch else 0
    if "mean" not in want:
        nquery = 0
    elif nquery is None:
        nquery = As.size // (batch * n) if batch else 0
    if targets and batch and (ntarget < 1 or Ys.size < batch * ntarget * n):
        raise ValueError("Ys needs batch*D*n elements, D >= 1")
    if "mean" in want and batch and (nquery < 1 or As.size < batch * nquery * n):
        raise ValueError("As needs batch*Q*n elements, Q >= 1")
    if Cs is not None and Cs.size < batch * n:
        raise ValueError("Cs smaller than batch*n")
    sizes = dict(alpha=batch * ntarget * n, quad=batch * ntarget, logdet=batch, logml=batch * ntarget, mean=batch * ntarget * nquery)
    out = {k: np.empty(sizes[k], dtype=Bs.dtype) if k in want else None for k in _MULTI_TARGET_OUTPUTS}
    info = np.zeros(batch, dtype=np.int32)
    p = _array_ptr
    _lib.check(_lib.lib().matinv_multi_target_batched_host(
        _np_dtype_code(Bs.dtype), n, ntarget, nquery, p(Bs), p(Cs), p(Ys) if targets else None, p(As) if "mean" in want else None,
        p(out["alpha"]), p(out["quad"]), p(out["logdet"]), p(out["logml"]), p(out["mean"]), batch, p(info)))
    return out["alpha"], out["quad"], out["logdet"], out["logml"], out["mean"], info


def multi_target_kernel_name(dtype, n: int) -> str:
    """matinv_multi_target_kernel_name: the kernel a multi-target request launches ("" when the request would be refused)."""
    code = _dtype_code(dtype)
    return _lib.lib().matinv_multi_target_kernel_name(code, n).decode()


_MULTI_TARGET_GRAD_OUTPUTS = ("grad", "gradc", "logml", "alpha")


def multi_target_grad_batched(n, Bs, Cs, Ys, dMs, grad=None, gradc=None, logml=None, alpha=None, batchSize=None, info=None, want=("grad",),
                              ntarget=None, nparam=None):
    """Gradients of the multi-output GP log marginal likelihood on device tensors (matinv_multi_target_grad_batched; asynchronous on torch's
    current stream): the gradient of sum_t logml[k, t] of multi_target_batched, from one factorisation. With M_k = B_k + diag c_k,
    K = M_k^-1, alpha_t = K y_kt for the D targets and G = sum_t alpha_t alpha_t^T - D K:
        grad[k, p] = 1/2 sum_ij G_ij dM_p[i, j],  gradc[k, i] = 1/2 G_ii,  logml[k, t] and alpha[k, t] as multi_target_batched (bit for bit)
    Ys: batchSize*D*n elements, target (k, t) at (k*D + t)*n; alpha has its layout. dMs: batchSize*P*n*n elements, matrix (k, p) at
    (k*P + p)*n*n, column-major, lower triangle read. grad is batchSize*P, gradc batchSize*n, logml batchSize*D. D and P are inferred from
    Ys.numel() and dMs.numel() unless `ntarget` / `nparam` are given.
    An output is computed when its tensor is given or its name is in `want` (then it is allocated); at least one; which are asked for
    changes no bit of the others. Cs may be None (M = B), dMs may be None when grad is not asked for. Only the lower triangles of B and
    dM are read and no input is modified. Not positive definite: info = the 1-based column of the first non-positive pivot and every
    requested output of that matrix NaN.
    Returns (grad, gradc, logml, alpha), None for what was not asked for."""
    import torch
    _require_cuda(Bs, Cs, Ys, dMs, grad, gradc, logml, alpha, info)
    if batchSize is None:
        batchSize = Bs.numel() // (n * n)
    unknown = set(want) - set(_MULTI_TARGET_GRAD_OUTPUTS)
    if unknown:
        raise ValueError(f"want holds {sorted(unknown)}; the outputs are {_MULTI_TARGET_GRAD_OUTPUTS}")
    given = dict(grad=grad, gradc=gradc, logml=logml, alpha=alpha)
    asked = {k: given[k] is not None or k in want for k in _MULTI_TARGET_GRAD_OUTPUTS}
    if not any(asked.values()):
        raise ValueError("no output requested")
    if Ys is None:
        raise ValueError("every output needs the targets Ys")
    if asked["grad"] and dMs is None:
        raise ValueError("grad needs the derivative matrices dMs")
    if ntarget is None:
        ntarget = Ys.numel() // (batchSize * n) if batchSize else 0
    if not asked["grad"]:
        nparam = 0
    elif nparam is None:
        nparam = dMs.numel() // (batchSize * n * n) if batchSize else 0
    if batchSize and (ntarget < 1 or Ys.numel() < batchSize * ntarget * n):
        raise ValueError("Ys needs batchSize*D*n elements, D >= 1")
    if asked["grad"] and batchSize and (nparam < 1 or dMs.numel() < batchSize * nparam * n * n):
        raise ValueError("dMs needs batchSize*P*n*n elements, P >= 1")
    sizes = dict(grad=batchSize * nparam, gradc=batchSize * n, logml=batchSize * ntarget, alpha=batchSize * ntarget * n)
    for k in _MULTI_TARGET_GRAD_OUTPUTS:
        if asked[k] and given[k] is None:
            given[k] = torch.empty(sizes[k], dtype=Bs.dtype, device=Bs.device)
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Ys, dMs, *given.values())):
        raise TypeError("Bs, Cs, Ys, dMs and the outputs must have one dtype")
    if (Cs is not None and Cs.numel() < batchSize * n) or \
            any(given[k] is not None and given[k].numel() < sizes[k] for k in _MULTI_TARGET_GRAD_OUTPUTS):
        raise ValueError("Cs needs batchSize*n elements, grad batchSize*P, gradc batchSize*n, logml batchSize*D, alpha batchSize*D*n")
    _check_info(info, batchSize)
    p = _tensor_ptr
    with torch.cuda.device(Bs.device):
        _lib.check(_lib.lib().matinv_multi_target_grad_batched(
            _torch_dtype_code(Bs), n, ntarget, nparam, p(Bs), p(Cs), p(Ys), p(dMs) if asked["grad"] else None, p(given["grad"]),
            p(given["gradc"]), p(given["logml"]), p(given["alpha"]), batchSize, p(info), _stream_ptr(Bs)))
    return given["grad"], given["gradc"], given["logml"], given["alpha"]


def multi_target_grad_batched_host(n, Bs: np.ndarray, Cs, Ys, dMs, want=_MULTI_TARGET_GRAD_OUTPUTS, ntarget=None, nparam=None):
    """matinv_multi_target_grad_batched_host on numpy batches (packed; Cs may be None, dMs may be None without "grad" in want, which the
    default `want` then drops): returns (grad, gradc, logml, alpha, info), None for the outputs not in want. Synchronous."""
    Bs = np.ascontiguousarray(Bs)
    Cs, Ys, dMs = (None if t is None else np.ascontiguousarray(t) for t in (Cs, Ys, dMs))
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Ys, dMs)):
        raise TypeError("Bs, Cs, Ys and dMs must have one dtype")
    if want is _MULTI_TARGET_GRAD_OUTPUTS and dMs is None:
        want = _MULTI_TARGET_GRAD_OUTPUTS[1:]
    unknown = set(want) - set(_MULTI_TARGET_GRAD_OUTPUTS)
    if unknown or not want:
        raise ValueError(f"want must name at least one of {_MULTI_TARGET_GRAD_OUTPUTS}")
    batch = Bs.size // (n * n)
    if Ys is None:
        raise ValueError("every output needs the targets Ys")
    if "grad" in want and dMs is None:
        raise ValueError("grad needs the derivative matrices dMs")
    if ntarget is None:
        ntarget = Ys.size // (batch * n) if batch else 0
    if "grad" not in want:
        nparam = 0
    elif nparam is None:
        nparam = dMs.size // (batch * n * n) if batch else 0
    if batch and (ntarget < 1 or Ys.size < batch * ntarget * n):
        raise ValueError("Ys needs batch*D*n elements, D >= 1")
    if "grad" in want and batch and (nparam < 1 or dMs.size < batch * nparam * n * n):
        raise ValueError("dMs needs batch*P*n*n elements, P >= 1")
    if Cs is not None and Cs.size < batch * n:
        raise ValueError("Cs smaller than batch*n")
    sizes = dict(grad=batch * nparam, gradc=batch * n, logml=batch * ntarget, alpha=batch * ntarget * n)
    out = {k: np.empty(sizes[k], dtype=Bs.dtype) if k in want else None for k in _MULTI_TARGET_GRAD_OUTPUTS}
    info = np.zeros(batch, dtype=np.int32)
    p = _array_ptr
    _lib.check(_lib.lib().matinv_multi_target_grad_batched_host(
        _np_dtype_code(Bs.dtype), n, ntarget, nparam, p(Bs), p(Cs), p(Ys), p(dMs) if "grad" in want else None, p(out["grad"]),
        p(out["gradc"]), p(out["logml"]), p(out["alpha"]), batch, p(info)))
    return out["grad"], out["gradc"], out["logml"], out["alpha"], info


def multi_target_grad_kernel_name(dtype, n: int) -> str:
    """matinv_multi_target_grad_kernel_name: the kernel a multi-target gradient request launches ("" when the request would be refused)."""
    code = _dtype_code(dtype)
    return _lib.lib().matinv_multi_target_grad_kernel_name(code, n).decode()


_TREND_OUTPUTS = ("beta", "covbeta", "alpha", "quad", "logml", "mean", "var")
_TREND_TARGET_OUTPUTS = ("beta", "alpha", "quad", "logml", "mean")


def _trend_plan(n, batch, want, given, numel, Ys, As, Gs, Es, Hs, nbasis, ntarget, nquery):
    """what a trend request computes and its counts: (asked, nbasis, ntarget, nquery, sizes); `numel` counts a tensor's or array's elements"""
    unknown = set(want) - set(_TREND_OUTPUTS)
    if unknown:
        raise ValueError(f"want holds {sorted(unknown)}; the outputs are {_TREND_OUTPUTS}")
    if want is _TREND_OUTPUTS:  # the default: what the inputs given allow
        want = tuple(k for k in _TREND_OUTPUTS if not ((k in _TREND_TARGET_OUTPUTS and Ys is None)
                                                        or (k in ("mean", "var") and (As is None or Gs is None)) or (k == "var" and Es is None)))
    asked = {k: given[k] is not None or k in want for k in _TREND_OUTPUTS}
    if not any(asked.values()):
        raise ValueError("no output requested")
    targets = any(asked[k] for k in _TREND_TARGET_OUTPUTS)
    queries = asked["mean"] or asked["var"]
    if Hs is None:
        raise ValueError("the basis vectors Hs are needed")
    if targets and Ys is None:
        raise ValueError("beta, alpha, quad, logml and mean need the targets Ys")
    if queries and (As is None or Gs is None):
        raise ValueError("mean and var need the cross-covariance vectors As and the basis values Gs")
    if asked["var"] and Es is None:
        raise ValueError("var needs the prior variances Es")
    if nbasis is None:
        nbasis = numel(Hs) // (batch * n) if batch else 1
    if not 1 <= nbasis <= 16 or nbasis > n:
        raise ValueError(f"nbasis must be in 1 .. min(16, n) (got {nbasis})")
    if not targets:
        ntarget = 0
    elif ntarget is None:
        ntarget = numel(Ys) // (batch * n) if batch else 0
    if not queries:
        nquery = 0
    elif nquery is None:
        nquery = numel(As) // (batch * n) if batch else 0
    if batch and numel(Hs) < batch * nbasis * n:
        raise ValueError("Hs needs batch*K*n elements")
    if targets and batch and (ntarget < 1 or numel(Ys) < batch * ntarget * n):
        raise ValueError("Ys needs batch*D*n elements, D >= 1")
    if queries and batch and (nquery < 1 or numel(As) < batch * nquery * n or numel(Gs) < batch * nquery * nbasis):
        raise ValueError("As needs batch*Q*n elements and Gs batch*Q*K, Q >= 1")
    if asked["var"] and numel(Es) < batch * nquery:
        raise ValueError("Es needs batch*Q elements")
    sizes = dict(beta=batch * ntarget * nbasis, covbeta=batch * nbasis * nbasis, alpha=batch * ntarget * n, quad=batch * ntarget,
                 logml=batch * ntarget, mean=batch * ntarget * nquery, var=batch * nquery)
    return asked, nbasis, ntarget, nquery, sizes


def trend_batched(n, Bs, Cs, Hs, Ys=None, As=None, Gs=None, Es=None, beta=None, covbeta=None, alpha=None, quad=None, logml=None, mean=None,
                  var=None, batchSize=None, info=None, want=_TREND_OUTPUTS, nbasis=None, ntarget=None, nquery=None):
    """GP regression with a linear trend (universal kriging) on device tensors (matinv_trend_batched; asynchronous on torch's current
    stream): K basis vectors, D targets and Q query points per covariance matrix, one factorisation. With M_k = B_k + diag c_k,
    Kinv = M_k^-1, H = [h_1 .. h_K] and A = H^T Kinv H:
        beta[k, t] = A^-1 H^T Kinv y_kt,  covbeta[k] = A^-1,  alpha[k, t] = Kinv (y_kt - H beta[k, t]),  quad[k, t] = y_kt^T alpha[k, t],
        logml[k, t] = -(quad[k, t] + log det M_k + log det A + (n - K) log 2 pi) / 2,
        mean[k, t, j] = a_kj^T alpha[k, t] + g_kj^T beta[k, t],
        var[k, j] = e_kj - a_kj^T Kinv a_kj + r^T A^-1 r,  r = g_kj - H^T Kinv a_kj
    Hs: batchSize*K*n elements, basis vector (k, b) at (k*K + b)*n; Ys, As as in multi_target_batched; Gs: batchSize*Q*K, element
    (k, j, b) at (k*Q + j)*K + b; Es: batchSize*Q. beta is batchSize*D*K, covbeta batchSize*K*K, alpha has the layout of Ys, quad and logml
    are batchSize*D, mean batchSize*D*Q with element (k, t, j) at (k*D + t)*Q + j, var batchSize*Q. K, D and Q are inferred from
    Hs.numel(), Ys.numel() and As.numel() unless `nbasis` / `ntarget` / `nquery` are given; 1 <= K <= min(16, n).
    An output is computed when its tensor is given or its name is in `want` (then it is allocated); at least one; which are asked for
    changes no bit of the others. The default `want` holds every output the inputs given allow: those of the targets need Ys, mean and var
    need As and Gs, var needs Es. Cs may be None (M = B). Only B's lower triangle is read and no input is modified. info = the 1-based
    column of the first non-positive pivot of M, or n + b for the first non-positive pivot b of A (H rank deficient); every requested
    output of that matrix is then NaN.
    Returns (beta, covbeta, alpha, quad, logml, mean, var), None for what was not asked for."""
    import torch
    _require_cuda(Bs, Cs, Hs, Ys, As, Gs, Es, beta, covbeta, alpha, quad, logml, mean, var, info)
    if batchSize is None:
        batchSize = Bs.numel() // (n * n)
    given = dict(beta=beta, covbeta=covbeta, alpha=alpha, quad=quad, logml=logml, mean=mean, var=var)
    asked, nbasis, ntarget, nquery, sizes = _trend_plan(n, batchSize, want, given, lambda t: t.numel(), Ys, As, Gs, Es, Hs, nbasis, ntarget,
                                                        nquery)
    for k in _TREND_OUTPUTS:
        if asked[k] and given[k] is None:
            given[k] = torch.empty(sizes[k], dtype=Bs.dtype, device=Bs.device)
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Hs, Ys, As, Gs, Es, *given.values())):
        raise TypeError("Bs, Cs, Hs, Ys, As, Gs, Es and the outputs must have one dtype")
    if (Cs is not None and Cs.numel() < batchSize * n) or any(given[k] is not None and given[k].numel() < sizes[k] for k in _TREND_OUTPUTS):
        raise ValueError("Cs needs batchSize*n elements, beta batchSize*D*K, covbeta batchSize*K*K, alpha batchSize*D*n, quad and logml "
                         "batchSize*D, mean batchSize*D*Q, var batchSize*Q")
    _check_info(info, batchSize)
    targets = any(asked[k] for k in _TREND_TARGET_OUTPUTS)
    queries = asked["mean"] or asked["var"]
    p = _tensor_ptr
    with torch.cuda.device(Bs.device):
        _lib.check(_lib.lib().matinv_trend_batched(
            _torch_dtype_code(Bs), n, nbasis, ntarget, nquery, p(Bs), p(Cs), p(Hs), p(Ys) if targets else None, p(As) if queries else None,
            p(Gs) if queries else None, p(Es) if asked["var"] else None, *(p(given[k]) for k in _TREND_OUTPUTS), batchSize, p(info),
            _stream_ptr(Bs)))
    return tuple(given[k] for k in _TREND_OUTPUTS)


def trend_batched_host(n, Bs: np.ndarray, Cs, Hs, Ys=None, As=None, Gs=None, Es=None, want=_TREND_OUTPUTS, nbasis=None, ntarget=None,
                       nquery=None):
    """matinv_trend_batched_host on numpy batches (packed; Cs may be None; Ys, As, Gs, Es may be None when no output in want needs them, and
    the default `want` holds what the inputs given allow): returns (beta, covbeta, alpha, quad, logml, mean, var, info), None for the
    outputs not in want. Synchronous."""
    Bs = np.ascontiguousarray(Bs)
    Cs, Hs, Ys, As, Gs, Es = (None if t is None else np.ascontiguousarray(t) for t in (Cs, Hs, Ys, As, Gs, Es))
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Hs, Ys, As, Gs, Es)):
        raise TypeError("Bs, Cs, Hs, Ys, As, Gs and Es must have one dtype")
    batch = Bs.size // (n * n)
    none = dict.fromkeys(_TREND_OUTPUTS)
    asked, nbasis, ntarget, nquery, sizes = _trend_plan(n, batch, want, none, lambda a: a.size, Ys, As, Gs, Es, Hs, nbasis, ntarget, nquery)
    if Cs is not None and Cs.size < batch * n:
        raise ValueError("Cs smaller than batch*n")
    out = {k: np.empty(sizes[k], dtype=Bs.dtype) if asked[k] else None for k in _TREND_OUTPUTS}
    info = np.zeros(batch, dtype=np.int32)
    targets = any(asked[k] for k in _TREND_TARGET_OUTPUTS)
    queries = asked["mean"] or asked["var"]
    p = _array_ptr
    _lib.check(_lib.lib().matinv_trend_batched_host(
        _np_dtype_code(Bs.dtype), n, nbasis, ntarget, nquery, p(Bs), p(Cs), p(Hs), p(Ys) if targets else None, p(As) if queries else None,
        p(Gs) if queries else None, p(Es) if asked["var"] else None, *(p(out[k]) for k in _TREND_OUTPUTS), batch, p(info)))
    return (*(out[k] for k in _TREND_OUTPUTS), info)


def trend_kernel_name(dtype, n: int) -> str:
    """matinv_trend_kernel_name: the kernel a trend request launches ("" when the request would be refused)."""
    code = _dtype_code(dtype)
    return _lib.lib().matinv_trend_kernel_name(code, n).decode()


_TREND_GRAD_OUTPUTS = ("grad", "gradc", "logml", "alpha", "beta")


def _trend_grad_plan(n, batch, asked, numel, Hs, Ys, dMs, nbasis, ntarget, nparam):
    """the counts and output sizes of a trend gradient request: (nbasis, ntarget, nparam, sizes); `numel` counts a tensor's or array's
    elements"""
    if not any(asked.values()):
        raise ValueError("no output requested")
    if Hs is None:
        raise ValueError("the basis vectors Hs are needed")
    if Ys is None:
        raise ValueError("every output needs the targets Ys")
    if asked["grad"] and dMs is None:
        raise ValueError("grad needs the derivative matrices dMs")
    if nbasis is None:
        nbasis = numel(Hs) // (batch * n) if batch else 1
    if not 1 <= nbasis <= 16 or nbasis > n:
        raise ValueError(f"nbasis must be in 1 .. min(16, n) (got {nbasis})")
    if ntarget is None:
        ntarget = numel(Ys) // (batch * n) if batch else 0
    if not asked["grad"]:
        nparam = 0
    elif nparam is None:
        nparam = numel(dMs) // (batch * n * n) if batch else 0
    if batch and numel(Hs) < batch * nbasis * n:
        raise ValueError("Hs needs batch*K*n elements")
    if batch and (ntarget < 1 or numel(Ys) < batch * ntarget * n):
        raise ValueError("Ys needs batch*D*n elements, D >= 1")
    if asked["grad"] and batch and (nparam < 1 or numel(dMs) < batch * nparam * n * n):
        raise ValueError("dMs needs batch*P*n*n elements, P >= 1")
    sizes = dict(grad=batch * nparam, gradc=batch * n, logml=batch * ntarget, alpha=batch * ntarget * n, beta=batch * ntarget * nbasis)
    return nbasis, ntarget, nparam, sizes


def trend_grad_batched(n, Bs, Cs, Hs, Ys, dMs, grad=None, gradc=None, logml=None, alpha=None, beta=None, batchSize=None, info=None,
                       want=("grad",), nbasis=None, ntarget=None, nparam=None):
    """Gradients of the restricted (REML) log marginal likelihood of a GP with a linear trend on device tensors
    (matinv_trend_grad_batched; asynchronous on torch's current stream): the gradient of sum_t logml[k, t] of trend_batched, from one
    factorisation. With M_k = B_k + diag c_k, Kinv = M_k^-1, H the K basis vectors, A = H^T Kinv H, P = Kinv - Kinv H A^-1 H^T Kinv,
    alpha_t = P y_kt for the D targets and G = sum_t alpha_t alpha_t^T - D P:
        grad[k, p] = 1/2 sum_ij G_ij dM_p[i, j],  gradc[k, i] = 1/2 G_ii,  logml[k, t], alpha[k, t], beta[k, t] as trend_batched (bit for bit)
    Hs, Ys as in trend_batched; dMs: batchSize*P*n*n elements, matrix (k, p) at (k*P + p)*n*n, column-major, lower triangle read. grad is
    batchSize*P, gradc batchSize*n, logml batchSize*D, alpha batchSize*D*n, beta batchSize*D*K. K, D and P are inferred from Hs.numel(),
    Ys.numel() and dMs.numel() unless `nbasis` / `ntarget` / `nparam` are given; 1 <= K <= min(16, n).
    An output is computed when its tensor is given or its name is in `want` (then it is allocated); at least one; which are asked for
    changes no bit of the others. Cs may be None (M = B), dMs may be None when grad is not asked for. Only the lower triangles of B and
    dM are read and no input is modified. info = the 1-based column of the first non-positive pivot of M, or n + b for the first
    non-positive pivot b of A (H rank deficient); every requested output of that matrix is then NaN.
    Returns (grad, gradc, logml, alpha, beta), None for what was not asked for."""
    import torch
    _require_cuda(Bs, Cs, Hs, Ys, dMs, grad, gradc, logml, alpha, beta, info)
    if batchSize is None:
        batchSize = Bs.numel() // (n * n)
    unknown = set(want) - set(_TREND_GRAD_OUTPUTS)
    if unknown:
        raise ValueError(f"want holds {sorted(unknown)}; the outputs are {_TREND_GRAD_OUTPUTS}")
    given = dict(grad=grad, gradc=gradc, logml=logml, alpha=alpha, beta=beta)
    asked = {k: given[k] is not None or k in want for k in _TREND_GRAD_OUTPUTS}
    nbasis, ntarget, nparam, sizes = _trend_grad_plan(n, batchSize, asked, lambda t: t.numel(), Hs, Ys, dMs, nbasis, ntarget, nparam)
    for k in _TREND_GRAD_OUTPUTS:
        if asked[k] and given[k] is None:
            given[k] = torch.empty(sizes[k], dtype=Bs.dtype, device=Bs.device)
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Hs, Ys, dMs, *given.values())):
        raise TypeError("Bs, Cs, Hs, Ys, dMs and the outputs must have one dtype")
    if (Cs is not None and Cs.numel() < batchSize * n) or \
            any(given[k] is not None and given[k].numel() < sizes[k] for k in _TREND_GRAD_OUTPUTS):
        raise ValueError("Cs needs batchSize*n elements, grad batchSize*P, gradc batchSize*n, logml batchSize*D, alpha batchSize*D*n, "
                         "beta batchSize*D*K")
    _check_info(info, batchSize)
    p = _tensor_ptr
    with torch.cuda.device(Bs.device):
        _lib.check(_lib.lib().matinv_trend_grad_batched(
            _torch_dtype_code(Bs), n, nbasis, ntarget, nparam, p(Bs), p(Cs), p(Hs), p(Ys), p(dMs) if asked["grad"] else None,
            *(p(given[k]) for k in _TREND_GRAD_OUTPUTS), batchSize, p(info), _stream_ptr(Bs)))
    return tuple(given[k] for k in _TREND_GRAD_OUTPUTS)


def trend_grad_batched_host(n, Bs: np.ndarray, Cs, Hs, Ys, dMs, want=_TREND_GRAD_OUTPUTS, nbasis=None, ntarget=None, nparam=None):
    """matinv_trend_grad_batched_host on numpy batches (packed; Cs may be None, dMs may be None without "grad" in want, which the default
    `want` then drops): returns (grad, gradc, logml, alpha, beta, info), None for the outputs not in want. Synchronous."""
    Bs = np.ascontiguousarray(Bs)
    Cs, Hs, Ys, dMs = (None if t is None else np.ascontiguousarray(t) for t in (Cs, Hs, Ys, dMs))
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Hs, Ys, dMs)):
        raise TypeError("Bs, Cs, Hs, Ys and dMs must have one dtype")
    if want is _TREND_GRAD_OUTPUTS and dMs is None:
        want = _TREND_GRAD_OUTPUTS[1:]
    unknown = set(want) - set(_TREND_GRAD_OUTPUTS)
    if unknown or not want:
        raise ValueError(f"want must name at least one of {_TREND_GRAD_OUTPUTS}")
    batch = Bs.size // (n * n)
    asked = {k: k in want for k in _TREND_GRAD_OUTPUTS}
    nbasis, ntarget, nparam, sizes = _trend_grad_plan(n, batch, asked, lambda a: a.size, Hs, Ys, dMs, nbasis, ntarget, nparam)
    if Cs is not None and Cs.size < batch * n:
        raise ValueError("Cs smaller than batch*n")
    out = {k: np.empty(sizes[k], dtype=Bs.dtype) if asked[k] else None for k in _TREND_GRAD_OUTPUTS}
    info = np.zeros(batch, dtype=np.int32)
    p = _array_ptr
    _lib.check(_lib.lib().matinv_trend_grad_batched_host(
        _np_dtype_code(Bs.dtype), n, nbasis, ntarget, nparam, p(Bs), p(Cs), p(Hs), p(Ys), p(dMs) if asked["grad"] else None,
        *(p(out[k]) for k in _TREND_GRAD_OUTPUTS), batch, p(info)))
    return (*(out[k] for k in _TREND_GRAD_OUTPUTS), info)


def trend_grad_kernel_name(dtype, n: int) -> str:
    """matinv_trend_grad_kernel_name: the kernel a trend gradient request launches ("" when the request would be refused)."""
    code = _dtype_code(dtype)
    return _lib.lib().matinv_trend_grad_kernel_name(code, n).decode()


_TREND_LOO_OUTPUTS = ("mean", "var", "logpl")


def _trend_loo_plan(n, batch, want, given, numel, Hs, Ys, nbasis, ntarget):
    """what a trend leave-one-out request computes and its counts: (asked, nbasis, ntarget, sizes)"""
    unknown = set(want) - set(_TREND_LOO_OUTPUTS)
    if unknown:
        raise ValueError(f"want holds {sorted(unknown)}; the outputs are {_TREND_LOO_OUTPUTS}")
    if want is _TREND_LOO_OUTPUTS and Ys is None:  # the default: what the inputs given allow
        want = ("var",)
    asked = {k: given[k] is not None or k in want for k in _TREND_LOO_OUTPUTS}
    if not any(asked.values()):
        raise ValueError("no output requested")
    targets = asked["mean"] or asked["logpl"]
    if Hs is None:
        raise ValueError("the basis vectors Hs are needed")
    if targets and Ys is None:
        raise ValueError("mean and logpl need the targets Ys")
    if nbasis is None:
        nbasis = numel(Hs) // (batch * n) if batch else 1
    if not 1 <= nbasis <= 16 or nbasis >= n:
        raise ValueError(f"nbasis must be in 1 .. min(16, n - 1) (got {nbasis}): n - 1 points must carry the basis")
    if not targets:
        ntarget = 0
    elif ntarget is None:
        ntarget = numel(Ys) // (batch * n) if batch else 0
    if batch and numel(Hs) < batch * nbasis * n:
        raise ValueError("Hs needs batch*K*n elements")
    if targets and batch and (ntarget < 1 or numel(Ys) < batch * ntarget * n):
        raise ValueError("Ys needs batch*D*n elements, D >= 1")
    sizes = dict(mean=batch * ntarget * n, var=batch * n, logpl=batch * ntarget)
    return asked, nbasis, ntarget, sizes


def trend_loo_batched(n, Bs, Cs, Hs, Ys=None, mean=None, var=None, logpl=None, batchSize=None, info=None, want=_TREND_LOO_OUTPUTS,
                      nbasis=None, ntarget=None):
    """Leave-one-out cross-validation of a GP with a linear trend (universal kriging) on device tensors (matinv_trend_loo_batched;
    asynchronous on torch's current stream): all n held-out predictions of each of the D targets from one factorisation. With
    M_k = B_k + diag c_k, Kinv = M_k^-1, H the K basis vectors, A = H^T Kinv H, P = Kinv - Kinv H A^-1 H^T Kinv and alpha_t = P y_kt:
        var[k, i] = 1 / P_ii,  mean[k, t, i] = y_kti - alpha_ti / P_ii,
        logpl[k, t] = sum_i (1/2 log P_ii - 1/2 alpha_ti^2 / P_ii) - n/2 log 2 pi
    Hs, Ys as in trend_batched. mean has the layout of Ys, var is batchSize*n, logpl batchSize*D. K and D are inferred from Hs.numel() and
    Ys.numel() unless `nbasis` / `ntarget` are given; 1 <= K <= min(16, n - 1).
    An output is computed when its tensor is given or its name is in `want` (then it is allocated); at least one; which are asked for
    changes no bit of the others. var needs no targets: the default `want` is ("var",) when Ys is None. Cs may be None (M = B). Only B's
    lower triangle is read and no input is modified. info = the 1-based column of the first non-positive pivot of M, n + b for the first
    non-positive pivot b of A (both as trend_batched), or n + K + i for the first point i (1-based) whose P_ii is not > 0 (holding it out
    leaves the basis rank deficient); every requested output of that matrix is then NaN. A tiny positive P_ii is returned as it is.
    Returns (mean, var, logpl), None for what was not asked for."""
    import torch
    _require_cuda(Bs, Cs, Hs, Ys, mean, var, logpl, info)
    if batchSize is None:
        batchSize = Bs.numel() // (n * n)
    given = dict(mean=mean, var=var, logpl=logpl)
    asked, nbasis, ntarget, sizes = _trend_loo_plan(n, batchSize, want, given, lambda t: t.numel(), Hs, Ys, nbasis, ntarget)
    for k in _TREND_LOO_OUTPUTS:
        if asked[k] and given[k] is None:
            given[k] = torch.empty(sizes[k], dtype=Bs.dtype, device=Bs.device)
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Hs, Ys, *given.values())):
        raise TypeError("Bs, Cs, Hs, Ys and the outputs must have one dtype")
    if (Cs is not None and Cs.numel() < batchSize * n) or \
            any(given[k] is not None and given[k].numel() < sizes[k] for k in _TREND_LOO_OUTPUTS):
        raise ValueError("Cs and var need batchSize*n elements, mean batchSize*D*n, logpl batchSize*D")
    _check_info(info, batchSize)
    targets = asked["mean"] or asked["logpl"]
    p = _tensor_ptr
    with torch.cuda.device(Bs.device):
        _lib.check(_lib.lib().matinv_trend_loo_batched(
            _torch_dtype_code(Bs), n, nbasis, ntarget, p(Bs), p(Cs), p(Hs), p(Ys) if targets else None,
            *(p(given[k]) for k in _TREND_LOO_OUTPUTS), batchSize, p(info), _stream_ptr(Bs)))
    return tuple(given[k] for k in _TREND_LOO_OUTPUTS)


def trend_loo_batched_host(n, Bs: np.ndarray, Cs, Hs, Ys=None, want=_TREND_LOO_OUTPUTS, nbasis=None, ntarget=None):
    """matinv_trend_loo_batched_host on numpy batches (packed; Cs may be None; Ys may be None when only "var" is wanted, which the default
    `want` then is): returns (mean, var, logpl, info), None for the outputs not in want. Synchronous."""
    Bs = np.ascontiguousarray(Bs)
    Cs, Hs, Ys = (None if t is None else np.ascontiguousarray(t) for t in (Cs, Hs, Ys))
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Hs, Ys)):
        raise TypeError("Bs, Cs, Hs and Ys must have one dtype")
    batch = Bs.size // (n * n)
    none = dict.fromkeys(_TREND_LOO_OUTPUTS)
    asked, nbasis, ntarget, sizes = _trend_loo_plan(n, batch, want, none, lambda a: a.size, Hs, Ys, nbasis, ntarget)
    if Cs is not None and Cs.size < batch * n:
        raise ValueError("Cs smaller than batch*n")
    out = {k: np.empty(sizes[k], dtype=Bs.dtype) if asked[k] else None for k in _TREND_LOO_OUTPUTS}
    info = np.zeros(batch, dtype=np.int32)
    targets = asked["mean"] or asked["logpl"]
    p = _array_ptr
    _lib.check(_lib.lib().matinv_trend_loo_batched_host(
        _np_dtype_code(Bs.dtype), n, nbasis, ntarget, p(Bs), p(Cs), p(Hs), p(Ys) if targets else None,
        *(p(out[k]) for k in _TREND_LOO_OUTPUTS), batch, p(info)))
    return (*(out[k] for k in _TREND_LOO_OUTPUTS), info)


def trend_loo_kernel_name(dtype, n: int) -> str:
    """matinv_trend_loo_kernel_name: the kernel a trend leave-one-out request launches ("" when the request would be refused)."""
    code = _dtype_code(dtype)
    return _lib.lib().matinv_trend_loo_kernel_name(code, n).decode()


_ARD_OUTPUTS = ("logml", "grad", "alpha")


def _ard_plan(n, X, y, theta, ndim, batch, numel, Xq=None):
    """(ndim, batch, xstride, ystride) of an ARD request: ndim is the last axis of a 2-D or 3-D X unless given, the batch is what theta
    holds, and an X of n*ndim elements (a y of n) beside a larger batch is ONE shared point set (target vector): stride 0.
    With Xq (a prediction request) the tuple goes on with (nquery, xqstride) by the same rule: Xq is (batch, nquery, ndim) or
    (nquery, ndim), nquery its last axis but one, and an Xq of nquery*ndim elements beside a larger batch is ONE shared query set. y may
    then be None (no mean; ystride n)."""
    if ndim is None:
        if len(X.shape) < 2:
            raise ValueError("ndim is needed with a flat X")
        ndim = int(X.shape[-1])
    if ndim < 1:
        raise ValueError(f"ndim must be >= 1 (got {ndim})")
    if batch is None:
        batch = numel(theta) // (ndim + 2)
    if numel(theta) < batch * (ndim + 2):
        raise ValueError("theta needs batch*(ndim + 2) elements: log sf2, log l_1 .. log l_ndim, log sn2")
    xstride = 0 if numel(X) == n * ndim and batch > 1 else n * ndim
    ystride = 0 if y is not None and numel(y) == n and batch > 1 else n
    if numel(X) < (batch * n * ndim if xstride else n * ndim) or (y is not None and numel(y) < (batch * n if ystride else n)):
        raise ValueError("X needs batch*n*ndim elements (or n*ndim: one shared point set), y batch*n (or n)")
    if Xq is None:
        return ndim, batch, xstride, ystride
    if len(Xq.shape) < 2 or int(Xq.shape[-1]) != ndim or int(Xq.shape[-2]) < 1:
        raise ValueError("Xq must be (batch, nquery, ndim), or (nquery, ndim) for one shared query set, with nquery >= 1")
    nquery = int(Xq.shape[-2])
    xqstride = 0 if numel(Xq) == nquery * ndim and batch > 1 else nquery * ndim
    if numel(Xq) < (batch * nquery * ndim if xqstride else nquery * ndim):
        raise ValueError("Xq needs batch*nquery*ndim elements (or nquery*ndim: one shared query set)")
    return ndim, batch, xstride, ystride, nquery, xqstride


def ard_logml_batched(n, X, y, theta, kind=COV_SE, logml=None, grad=None, alpha=None, ndim=None, batchSize=None, info=None,
                      want=_ARD_OUTPUTS):
    """GP log marginal likelihood and its gradient from coordinates on device tensors (matinv_ard_logml_batched; asynchronous on torch's
    current stream): the covariance matrices are generated inside the kernel and never reach memory. X: the points, point-major
    (batch, n, ndim) -- or (n, ndim) for one point set shared by the batch; y: (batch, n) or (n,) likewise; theta: (batch, ndim + 2) =
    (log sf2, log l_1 .. log l_ndim, log sn2) per matrix; kind: COV_SE or COV_MATERN52. A flat X needs ndim. An output is computed when
    its tensor is given or its name is in `want` (then it is allocated); at least one. Returns (logml, grad, alpha): batch, batch*(ndim+2)
    and batch*n elements, None for what was not asked for. grad is with respect to theta."""
    import torch
    _require_cuda(X, y, theta, logml, grad, alpha, info)
    unknown = set(want) - set(_ARD_OUTPUTS)
    if unknown:
        raise ValueError(f"want holds {sorted(unknown)}; the outputs are {_ARD_OUTPUTS}")
    if logml is None and grad is None and alpha is None and not want:
        raise ValueError("no output requested")
    ndim, batch, xstride, ystride = _ard_plan(n, X, y, theta, ndim, batchSize, lambda t: t.numel())
    if logml is None and "logml" in want:
        logml = torch.empty(batch, dtype=X.dtype, device=X.device)
    if grad is None and "grad" in want:
        grad = torch.empty(batch * (ndim + 2), dtype=X.dtype, device=X.device)
    if alpha is None and "alpha" in want:
        alpha = torch.empty(batch * n, dtype=X.dtype, device=X.device)
    if any(t is not None and t.dtype != X.dtype for t in (y, theta, logml, grad, alpha)):
        raise TypeError("X, y, theta, logml, grad and alpha must have one dtype")
    if (logml is not None and logml.numel() < batch) or (grad is not None and grad.numel() < batch * (ndim + 2)) or \
            (alpha is not None and alpha.numel() < batch * n):
        raise ValueError("logml needs batch elements, grad batch*(ndim + 2), alpha batch*n")
    _check_info(info, batch)
    p = _tensor_ptr
    with torch.cuda.device(X.device):
        _lib.check(_lib.lib().matinv_ard_logml_batched(
            _torch_dtype_code(X), kind, n, ndim, p(X), xstride, p(y), ystride, p(theta), p(logml), p(grad), p(alpha), batch, p(info),
            _stream_ptr(X)))
    return logml, grad, alpha


def ard_logml_batched_host(n, X: np.ndarray, y: np.ndarray, theta: np.ndarray, kind=COV_SE, want=_ARD_OUTPUTS, ndim=None):
    """matinv_ard_logml_batched_host on numpy arrays (shapes as ard_logml_batched): returns (logml, grad, alpha, info), None for the
    outputs not in want. Synchronous."""
    X, y, theta = np.ascontiguousarray(X), np.ascontiguousarray(y), np.ascontiguousarray(theta)
    if y.dtype != X.dtype or theta.dtype != X.dtype:
        raise TypeError("X, y and theta must have one dtype")
    unknown = set(want) - set(_ARD_OUTPUTS)
    if unknown or not want:
        raise ValueError(f"want must name at least one of {_ARD_OUTPUTS}")
    ndim, batch, xstride, ystride = _ard_plan(n, X, y, theta, ndim, None, lambda a: a.size)
    logml = np.empty(batch, dtype=X.dtype) if "logml" in want else None
    grad = np.empty(batch * (ndim + 2), dtype=X.dtype) if "grad" in want else None
    alpha = np.empty(batch * n, dtype=X.dtype) if "alpha" in want else None
    info = np.zeros(batch, dtype=np.int32)
    p = _array_ptr
    _lib.check(_lib.lib().matinv_ard_logml_batched_host(
        _np_dtype_code(X.dtype), kind, n, ndim, p(X), xstride, p(y), ystride, p(theta), p(logml), p(grad), p(alpha), batch, p(info)))
    return logml, grad, alpha, info


def ard_logml_kernel_name(dtype, kind: int, n: int) -> str:
    """matinv_ard_logml_kernel_name: the kernel such a request launches ("" when the request would be refused)."""
    code = _dtype_code(dtype)
    return _lib.lib().matinv_ard_logml_kernel_name(code, kind, n).decode()


_ARD_PREDICT_OUTPUTS = ("mean", "var")


def ard_predict_batched(n, X, y, theta, Xq, kind=COV_SE, mean=None, var=None, ndim=None, batchSize=None, info=None,
                        want=_ARD_PREDICT_OUTPUTS):
    """GP prediction from coordinates on device tensors (matinv_ard_predict_batched; asynchronous on torch's current stream): the
    covariance matrices and the cross-covariance vectors of the queries are generated inside the kernel and never reach memory. X, y,
    theta, kind as in ard_logml_batched; Xq: the query points, (batch, nquery, ndim) -- or (nquery, ndim) for one query set shared by
    the batch; nquery comes from it. An output is computed when its tensor is given or its name is in `want` (then it is allocated); at
    least one. y may be None when mean is not asked for. Returns (mean, var): batch*nquery elements each, None for what was not asked
    for. var is the variance of the latent function: add exp(theta[:, ndim + 1]) for that of a noisy observation."""
    import torch
    _require_cuda(X, y, theta, Xq, mean, var, info)
    unknown = set(want) - set(_ARD_PREDICT_OUTPUTS)
    if unknown:
        raise ValueError(f"want holds {sorted(unknown)}; the outputs are {_ARD_PREDICT_OUTPUTS}")
    if mean is None and var is None and not want:
        raise ValueError("no output requested")
    ndim, batch, xstride, ystride, nquery, xqstride = _ard_plan(n, X, y, theta, ndim, batchSize, lambda t: t.numel(), Xq)
    if mean is None and "mean" in want:
        mean = torch.empty(batch * nquery, dtype=X.dtype, device=X.device)
    if var is None and "var" in want:
        var = torch.empty(batch * nquery, dtype=X.dtype, device=X.device)
    if mean is not None and y is None:
        raise ValueError("mean needs y")
    if any(t is not None and t.dtype != X.dtype for t in (y, theta, Xq, mean, var)):
        raise TypeError("X, y, theta, Xq, mean and var must have one dtype")
    if any(t is not None and t.numel() < batch * nquery for t in (mean, var)):
        raise ValueError("mean and var need batch*nquery elements")
    _check_info(info, batch)
    p = _tensor_ptr
    with torch.cuda.device(X.device):
        _lib.check(_lib.lib().matinv_ard_predict_batched(
            _torch_dtype_code(X), kind, n, ndim, nquery, p(X), xstride, p(y), ystride, p(theta), p(Xq), xqstride, p(mean), p(var), batch,
            p(info), _stream_ptr(X)))
    return mean, var


def ard_predict_batched_host(n, X: np.ndarray, y, theta: np.ndarray, Xq: np.ndarray, kind=COV_SE, want=_ARD_PREDICT_OUTPUTS, ndim=None):
    """matinv_ard_predict_batched_host on numpy arrays (shapes as ard_predict_batched): returns (mean, var, info), None for the outputs
    not in want. Synchronous."""
    X, theta, Xq = np.ascontiguousarray(X), np.ascontiguousarray(theta), np.ascontiguousarray(Xq)
    y = None if y is None else np.ascontiguousarray(y)
    if theta.dtype != X.dtype or Xq.dtype != X.dtype or (y is not None and y.dtype != X.dtype):
        raise TypeError("X, y, theta and Xq must have one dtype")
    unknown = set(want) - set(_ARD_PREDICT_OUTPUTS)
    if unknown or not want:
        raise ValueError(f"want must name at least one of {_ARD_PREDICT_OUTPUTS}")
    if "mean" in want and y is None:
        raise ValueError("mean needs y")
    ndim, batch, xstride, ystride, nquery, xqstride = _ard_plan(n, X, y, theta, ndim, None, lambda a: a.size, Xq)
    mean = np.empty(batch * nquery, dtype=X.dtype) if "mean" in want else None
    var = np.empty(batch * nquery, dtype=X.dtype) if "var" in want else None
    info = np.zeros(batch, dtype=np.int32)
    p = _array_ptr
    _lib.check(_lib.lib().matinv_ard_predict_batched_host(
        _np_dtype_code(X.dtype), kind, n, ndim, nquery, p(X), xstride, p(y), ystride, p(theta), p(Xq), xqstride, p(mean), p(var), batch,
        p(info)))
    return mean, var, info


def ard_predict_kernel_name(dtype, kind: int, n: int) -> str:
    """matinv_ard_predict_kernel_name: the kernel such a request launches ("" when the request would be refused)."""
    code = _dtype_code(dtype)
    return _lib.lib().matinv_ard_predict_kernel_name(code, kind, n).decode()


_SAMPLE_OUTPUTS = ("Y", "mean", "cov")


def sample_batched(n, Bs, Cs, Ds, As, Es, Zs, Y=None, mean=None, cov=None, batchSize=None, info=None, want=("Y",)):
    """Joint posterior samples of a GP at the Q query points of each covariance matrix on device tensors (matinv_sample_batched;
    asynchronous on torch's current stream):  Y_k[:, s] = mean_k + chol(cov_k) z_ks  with mean and cov as predict_cov_batched returns
    them for the same Bs, Cs, Ds, As, Es. Zs: batchSize*S*Q elements, sample s of matrix k a run of Q elements; Y has the same layout.
    Y is always computed; mean (batchSize*Q) and cov (batchSize*Q*Q) are extra outputs, computed when their tensor is given or their name is
    in `want`, and they do not change a bit of Y. Ds = None means the zero-mean posterior (and mean cannot be asked for). There is no
    jitter parameter: Es is the caller's, and jitter goes on its diagonal. info: 0; 1 .. n when M is not positive definite (everything
    NaN); n + j when column j of cov has the first non-positive pivot (Y NaN, mean and cov valid).
    Returns (Y, mean, cov), None for what was not asked for."""
    import torch
    _require_cuda(Bs, Cs, Ds, As, Es, Zs, Y, mean, cov, info)
    if batchSize is None:
        batchSize = Bs.numel() // (n * n)
    unknown = set(want) - set(_SAMPLE_OUTPUTS)
    if unknown:
        raise ValueError(f"want holds {sorted(unknown)}; the outputs are {_SAMPLE_OUTPUTS}")
    if As is None or Zs is None:
        raise ValueError("sampling needs the cross-covariance vectors As and the samples Zs")
    nquery = As.numel() // (batchSize * n) if batchSize else 0
    if batchSize and (nquery < 1 or As.numel() < batchSize * nquery * n):
        raise ValueError("As needs batchSize*Q*n elements, Q >= 1")
    nsample = Zs.numel() // (batchSize * nquery) if batchSize else 0
    if batchSize and (nsample < 1 or Zs.numel() < batchSize * nsample * nquery):
        raise ValueError("Zs needs batchSize*S*Q elements, S >= 1")
    if Y is None:
        Y = torch.empty(batchSize * nsample * nquery, dtype=Bs.dtype, device=Bs.device)
    if mean is None and "mean" in want:
        mean = torch.empty(batchSize * nquery, dtype=Bs.dtype, device=Bs.device)
    if cov is None and "cov" in want:
        cov = torch.empty(batchSize * nquery * nquery, dtype=Bs.dtype, device=Bs.device)
    if mean is not None and Ds is None:
        raise ValueError("mean needs the observations Ds")
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Ds, As, Es, Zs, Y, mean, cov)):
        raise TypeError("Bs, Cs, Ds, As, Es, Zs, Y, mean and cov must have one dtype")
    if any(t is not None and t.numel() < batchSize * n for t in (Cs, Ds)) or (mean is not None and mean.numel() < batchSize * nquery) or \
            any(t is not None and t.numel() < batchSize * nquery * nquery for t in (Es, cov)) or Y.numel() < batchSize * nsample * nquery:
        raise ValueError("Cs and Ds need batchSize*n elements, mean batchSize*Q, Es and cov batchSize*Q*Q, Y batchSize*S*Q")
    _check_info(info, batchSize)
    p = _tensor_ptr
    with torch.cuda.device(Bs.device):
        _lib.check(_lib.lib().matinv_sample_batched(
            _torch_dtype_code(Bs), n, nquery, nsample, p(Bs), p(Cs), p(Ds), p(As), p(Es), p(Zs), p(Y), p(mean), p(cov), batchSize, p(info),
            _stream_ptr(Bs)))
    return Y, mean, cov


def sample_batched_host(n, Bs: np.ndarray, Cs, Ds, As: np.ndarray, Es, Zs: np.ndarray, want=("Y",)):
    """matinv_sample_batched_host on numpy batches (packed; Cs, Ds and Es may be None): returns (Y, mean, cov, info), None for the outputs
    not in want. Synchronous."""
    Bs, As, Zs = np.ascontiguousarray(Bs), np.ascontiguousarray(As), np.ascontiguousarray(Zs)
    Cs, Ds, Es = (None if t is None else np.ascontiguousarray(t) for t in (Cs, Ds, Es))
    if any(t is not None and t.dtype != Bs.dtype for t in (Cs, Ds, As, Es, Zs)):
        raise TypeError("Bs, Cs, Ds, As, Es and Zs must have one dtype")
    unknown = set(want) - set(_SAMPLE_OUTPUTS)
    if unknown:
        raise ValueError(f"want holds {sorted(unknown)}; the outputs are {_SAMPLE_OUTPUTS}")
    batch = Bs.size // (n * n)
    nquery = As.size // (batch * n) if batch else 0
    if batch and nquery < 1:
        raise ValueError("As needs batch*Q*n elements, Q >= 1")
    nsample = Zs.size // (batch * nquery) if batch else 0
    if batch and nsample < 1:
        raise ValueError("Zs needs batch*S*Q elements, S >= 1")
    if "mean" in want and Ds is None:
        raise ValueError("mean needs the observations Ds")
    if any(t is not None and t.size < batch * n for t in (Cs, Ds)) or (Es is not None and Es.size < batch * nquery * nquery):
        raise ValueError("Cs and Ds smaller than batch*n, or Es smaller than batch*Q*Q")
    Y = np.empty(batch * nsample * nquery, dtype=Bs.dtype)
    mean = np.empty(batch * nquery, dtype=Bs.dtype) if "mean" in want else None
    cov = np.empty(batch * nquery * nquery, dtype=Bs.dtype) if "cov" in want else None
    info = np.zeros(batch, dtype=np.int32)
    p = _array_ptr
    _lib.check(_lib.lib().matinv_sample_batched_host(
        _np_dtype_code(Bs.dtype), n, nquery, nsample, p(Bs), p(Cs), p(Ds), p(As), p(Es), p(Zs), p(Y), p(mean), p(cov), batch, p(info)))
    return Y, mean, cov, info


def logdet_kernel_name(algo: int, dtype, n: int, kernel: int = KERNEL_AUTO) -> str:
    """matinv_logdet_kernel_name: the kernel a logdet request launches ("" when the request would be refused)."""
    code = _dtype_code(dtype)
    return _lib.lib().matinv_logdet_kernel_name(algo, code, n, kernel).decode()


def gp_kernel_name(dtype, n: int, variance: bool = False) -> str:
    """matinv_gp_kernel_name: the first kernel a fused mean / variance request launches ("" when the request would be refused)."""
    code = _dtype_code(dtype)
    return _lib.lib().matinv_gp_kernel_name(code, n, 1 if variance else 0).decode()


def logml_kernel_name(dtype, n: int) -> str:
    """matinv_logml_kernel_name: the first kernel a logml request launches ("" when the request would be refused)."""
    code = _dtype_code(dtype)
    return _lib.lib().matinv_logml_kernel_name(code, n).decode()


mean_batched = calcluateMean
variance_batched = calcluateVariance


def tile_stats() -> dict:
    """matinv_tile_stats: how the adaptive natural-order / pivoting dispatch of the tile family went since load."""
    v = [ctypes.c_ulonglong(0) for _ in range(4)]
    _lib.check(_lib.lib().matinv_tile_stats(*[ctypes.byref(x) for x in v]))
    return dict(zip(("natural_launches", "pivot_launches", "last_rejected", "last_batch"), (int(x.value) for x in v)))


def sym_front_stats() -> dict:
    """matinv_sym_front_stats: which route the unscreened 64 x 64 fp64 Gauss-Jordan launches took since load (symmetric-only kernel in
    front / two-arm kernel alone) and what the last completed front launch found."""
    v = [ctypes.c_ulonglong(0) for _ in range(4)]
    _lib.check(_lib.lib().matinv_sym_front_stats(*[ctypes.byref(x) for x in v]))
    return dict(zip(("front_launches", "direct_launches", "last_not_symmetric", "last_batch"), (int(x.value) for x in v)))


def select_kernel(algo: int, dtype, n: int) -> int:
    code = _dtype_code(dtype)
    k = _lib.lib().matinv_select_kernel(algo, code, n)
    if k < 0:
        _lib.check(k)
    return k


def kernel_name(algo: int, dtype, n: int, kernel: int = KERNEL_AUTO) -> str:
    code = _dtype_code(dtype)
    return _lib.lib().matinv_kernel_name(algo, code, n, kernel).decode()
